"""Songcast sender frames on the device against tests/ohm_textbook.py (every header field by struct.pack; the sender's channel
selection and 24-bit cap) with the fragments' audio from tests/pcm_textbook.py -- no oracle in the expected bytes.  Frames of 1
sample and of the 5 ms maximum at each rate (capped by OhmMsgAudio::kMaxSampleBytes), 8/16/24/32 bits, 1..10 channels, both source
byte orders, codec names of 0..29 bytes (header sizes 58..87: prefixes of every length mod 4), plain / ramped / silent / attenuated
fragments, several fragments per frame, halt, timestamped and resent frames, destination alignment 0..3 with no gap between frames.
NOT covered: prefixes of 4..8 and of 255 bytes -- the line kernel admits them, but no exported call produces one (a Songcast header
is 58..87 bytes), so only a test inside the library could reach them.

Every test first asks ohgpu_batch_paths_info which route the batch was planned onto -- mono and stereo streams: audio and header in
one pass of the line kernel (prefixed chunks, ohm_headers_fused); wider streams: the channel-selecting kernel
(ohm_wide_fragments) -- and the same batch is then run on the fused route and on the generic route (kernel variant 1: the generic
pcm kernel and ohm_header_kernel for EVERY header), which must give equal bytes.

Mutations of the library these tests were seen to fail under on an MI355X (one build each, never committed; wrong bytes only):
  * csrc/ohm_frame_kernel.hip: kFlagTimestamped2 no longer set with kFlagTimestamped (`flags |= 0x10u` dropped): all eight
    test_mono_and_stereo_frames_every_field cases and test_one_batch_that_mixes_everything fail.
  * csrc/ohm_frame_kernel.hip: `first_ch = channels < 10 ? 0 : 8` replaced by `channels <= 10 ? 0 : 8` (a ten-channel stream sends
    channels 0 and 1): test_wider_streams_every_channel_count and test_one_batch_that_mixes_everything fail.
"""
import itertools

import pytest

from ohpipeline_amd import capi
from ohm_cases import LE, BE, Batch        # (the builder: shared with the far-offset tests)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


RATES = [7350, 44100, 48000, 96000, 192000, 384000]


@pytest.mark.parametrize("bits,ch", list(itertools.product([8, 16, 24, 32], [1, 2])))
def test_mono_and_stereo_frames_every_field(ctx, bits, ch):
    """The fused route: header and audio in one pass.  Every header field takes several values with bits in every byte; codec
    names of every length mod 4 put the audio at every alignment behind headers of 58..87 bytes; no gap between frames."""
    w = Batch(100 + bits + ch)
    n_frames = 0
    for k, rate in enumerate(RATES):
        st = w.stream(rate, bits, ch, endian=LE if k % 2 else BE, codec=b"abcdefghijklmnopqrstuvwxyz012"[:(k * 7 + bits // 8 + ch) % 30],
                      volume=(-32768, -3, 0, 255, 32767, -256)[k], total=(0, 1, 2 ** 40 + 5, 2 ** 63 + 7, 0x0102030405060708, 2 ** 64 - 1)[k])
        kinds = ["plain", "ramp", "silence"] + (["att"] if bits == 16 else [])
        for j, n in enumerate([1, 2, 3, 5, st["max_samples"] - 1, st["max_samples"]]):
            flags = capi.OHM_FLAG_LOSSLESS * (j % 2) | capi.OHM_FLAG_TIMESTAMPED * (j % 3 == 0) | capi.OHM_FLAG_HALT * (j == 5) | capi.OHM_FLAG_RESENT * (j == 2)
            w.frame(st, [(n, kinds[(j + k) % len(kinds)])], flags=flags, frame_no=(0, 1, 0x01020304, 2 ** 32 - 1, 77, 0x80000000)[j],
                    net=0xa0b0c0d0 + j, latency=(0, 0x00112233, 2 ** 32 - 1)[j % 3], start=(0, 2 ** 33 + j, 2 ** 64 - 1)[j % 3])
            n_frames += 1
        w.frame(st, [(1, "plain"), (7, "ramp"), (2, "silence"), (st["max_samples"] // 2, kinds[-1])], frame_no=9, start=12345)
        n_frames += 1
    paths = w.run(ctx)
    assert paths["line_planned"] == 1 and paths["ohm_wide_fragments"] == 0 and paths["ohm_staged_fragments"] == 0, paths
    assert paths["ohm_headers_fused"] == n_frames == paths["prefixed_chunks"] and paths["ohm_headers_separate"] == 0, paths


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_wider_streams_every_channel_count(ctx, bits):
    """3..10 channels: the first two channels (8 and 9 of ten), at most three bytes each; ramped, silent and attenuated fragments up
    to eight channels (beyond that the library takes plain big-endian fragments only and says so: ohgpu.h did not name the
    little-endian case and the error text blamed a ramp for it until this test met it)."""
    w = Batch(200 + bits)
    for ch in range(3, 11):
        st = w.stream(RATES[ch % 6], bits, ch, endian=LE if ch % 2 and ch <= 8 else BE, codec=b"PCM" * (ch % 4))
        kinds = (["plain", "ramp", "silence"] + (["att"] if bits == 16 else [])) if ch <= 8 else ["plain"]
        for j, n in enumerate([1, 2, 5, st["max_samples"]]):
            w.frame(st, [(n, kinds[(j + ch) % len(kinds)])], frame_no=j, start=j * 1000, flags=capi.OHM_FLAG_LOSSLESS | capi.OHM_FLAG_HALT * (j == 3), gap=j % 4)
        w.frame(st, [(3, kinds[0]), (4, kinds[-1]), (1, kinds[len(kinds) // 2])], frame_no=4)
    paths = w.run(ctx)
    assert paths["ohm_wide_fragments"] > 0 and paths["ohm_headers_fused"] == 0, paths
    if bits >= 16:                                               # nine channels: ramps and little-endian sources are refused, not guessed
        for endian, kind in ((BE, "ramp"), (LE, "plain"), (BE, "silence")):
            bad = Batch(1)
            bad.frame(bad.stream(48000, bits, 9, endian=endian), [(5, kind)])
            with pytest.raises(capi.OhGpuError) as e:
                bad.run(ctx)
            assert e.value.code == capi.ERR_UNSUPPORTED, (endian, kind)


def test_one_batch_that_mixes_everything(ctx):
    """Mono, stereo and wide streams of every depth and both byte orders in one batch, frames interleaved stream by stream, every
    destination alignment: both routes serve their share of the same batch."""
    w = Batch(300)
    sts = [w.stream(RATES[k % 6], bits, ch, endian=LE if k % 2 and ch <= 8 else BE, codec=b"FLAC"[:k % 5])
           for k, (bits, ch) in enumerate(itertools.product([8, 16, 24, 32], [1, 2, 4, 6, 8, 10]))]
    for j in range(4):
        for k, st in enumerate(sts):
            kind = "plain" if st["ch"] > 8 else ["plain", "ramp", "silence", "ramp"][(j + k) % 4]
            n = [1, 5, st["max_samples"], 43][(j + k) % 4]
            w.frame(st, [(n, kind)], frame_no=j, start=j * 240, net=k, latency=1000 + k, flags=capi.OHM_FLAG_LOSSLESS | capi.OHM_FLAG_TIMESTAMPED * (k % 2))
    paths = w.run(ctx)
    assert paths["ohm_wide_fragments"] > 0 and paths["ohm_headers_fused"] > 0 and paths["prefixed_chunks"] > 0, paths
