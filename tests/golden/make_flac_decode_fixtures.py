"""Writes tests/golden/flac_decode/*.flac + index.json: handmade FLAC streams (tests/flac_frames.py's writer) that, together with
the five encoder-made streams under tests/golden/flac/, cover every form the device decoder reads -- the census
tests/test_flac_textbook.py asserts -- and, with eight short streams entered far into their audio, every length of coded number and
first samples up to 2^36 - 48.  Each stream's STREAMINFO carries the MD5 of the PCM that went in; index.json records what each
holds and the model's census of it.  Where oracle/_ref exists (the reference's own libFLAC 1.2.1, tests/flac_ref.py) every stream is
decoded with it before it is written -- frames equal, MD5 accepted -- and the padding question of flac_textbook's docstring is put to
it.  Run from the repository root:  python tests/golden/make_flac_decode_fixtures.py"""
import json
import math
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import flac_frames as W          # noqa: E402
import flac_textbook as T        # noqa: E402

OUT = os.path.join(HERE, "flac_decode")


def tone(n, bits, seed, channels, scale=0.4, noise=3):
    """[n][channels]: a couple of sines per channel plus a little noise, right-justified at `bits`."""
    rnd = random.Random(seed)
    top = (1 << (bits - 1)) - 1
    f = [(0.01 + 0.013 * c + 0.002 * seed, 0.037 + 0.011 * c) for c in range(channels)]
    return [[max(-top - 1, min(top, int(round(scale * top * (0.7 * math.sin(2 * math.pi * f[c][0] * i) + 0.3 * math.sin(2 * math.pi * f[c][1] * i + c)))
                                   + rnd.randint(-noise, noise)))) for c in range(channels)] for i in range(n)]


def planes(pcm, lo, hi):
    return [[row[c] for row in pcm[lo:hi]] for c in range(len(pcm[0]))]


def cut(pcm, sizes):
    at = 0
    for n in sizes:
        yield at, planes(pcm, at, at + n)
        at += n
    assert at == len(pcm)


FIXED2 = dict(type="fixed", order=2)


def lpc(order, precision, shift, seed):
    """A stable, unremarkable predictor of the given order: a decaying mix (the fixtures are about forms, not compression)."""
    rnd = random.Random(seed)
    limit = (1 << (precision - 1)) - 1
    coefs = [max(-limit, min(limit, int((1 << shift) * (0.9 if j == 0 else rnd.uniform(-0.5, 0.5) / (j + 1))))) for j in range(order)]
    if order == 32:
        coefs[-1] = -limit            # (the last coefficient at the precision's full width)
    return dict(type="lpc", order=order, coefs=coefs, precision=precision, shift=shift)


def build():
    out = {}

    # 1. mono 16-bit, blocks of 16 (the 8-bit trailer), rate in kHz (trailer): CONSTANT, VERBATIM, FIXED 0..4
    pcm = tone(16 * 8, 16, 1, 1)
    for i in range(16):
        pcm[i][0] = -1234
    specs = [dict(type="constant"), dict(type="verbatim")] + [dict(type="fixed", order=k) for k in range(5)] + [dict(type="fixed", order=1, rice2=True)]
    frames = [W.frame(p, 16, 11000, k, [specs[k]], rate_form="khz") for k, (_, p) in enumerate(cut(pcm, [16] * 8))]
    out["forms_s16_mono_11k_b16"] = dict(data=W.stream(frames, pcm, 16, 11000, 1, min_blocksize=16, max_blocksize=16), blocksize=16)

    # 2. stereo 16-bit, blocks of 192, rate in Hz (trailer): LPC 1, 8, 12, 32 (precision 15), all four assignments, RICE2, partition order 6
    pcm = tone(192 * 6 + 50, 16, 2, 2)
    sizes = [192] * 6 + [50]
    spec_rows = [
        ([lpc(1, 12, 10, 1), lpc(8, 12, 9, 2)], None),
        ([lpc(12, 13, 10, 3), lpc(32, 15, 12, 4)], "left_side"),
        ([dict(lpc(8, 10, 8, 5), rice2=True), FIXED2], "right_side"),
        ([dict(FIXED2, partition_order=6), dict(type="fixed", order=3, partition_order=6, rice2=True)], "mid_side"),
        ([dict(type="fixed", order=1, partition_order=2, params={0: 0, 1: 14, 2: 3}), lpc(32, 15, 13, 6)], "mid_side"),
        ([lpc(2, 15, 14, 7), dict(type="verbatim")], None),
        ([FIXED2, FIXED2], "left_side"),
    ]
    frames = [W.frame(p, 16, 44056, k, spec_rows[k][0], stereo=spec_rows[k][1], rate_form="hz") for k, (_, p) in enumerate(cut(pcm, sizes))]
    out["lpc_s16_stereo_44056_b192"] = dict(data=W.stream(frames, pcm, 16, 44056, 2, min_blocksize=192, max_blocksize=192), blocksize=192)

    # 3. stereo 24-bit, blocks of 576, rate in tens of Hz (trailer), depth taken from STREAMINFO in one frame: escapes with 0 and with
    #    more raw bits, wasted bits on one channel of the pair
    pcm = tone(576 * 3, 24, 3, 2)
    for i in range(576, 576 * 2):
        pcm[i][1] = (pcm[i][1] >> 5) << 5                       # the right channel of frame 1: five wasted bits
    for i in range(576 * 2, 576 * 2 + 144 + 10):
        pcm[i][0] = 1000                                        # frame 2, left: FIXED 1 residuals all zero in partition 0
    spec_rows = [
        ([dict(FIXED2, partition_order=2, escapes=(1, 3)), FIXED2], None, {}),
        ([FIXED2, dict(FIXED2, wasted=5)], None, {"size_from_streaminfo": True}),
        ([dict(type="fixed", order=1, partition_order=2, escapes=(0, 2), rice2=True), dict(type="fixed", order=3, partition_order=3, rice2=True)], None, {}),
    ]
    frames = [W.frame(p, 24, 44100, k, spec_rows[k][0], stereo=spec_rows[k][1], rate_form="tens", **spec_rows[k][2]) for k, (_, p) in enumerate(cut(pcm, [576] * 3))]
    out["escape_wasted_s24_stereo_44k1_b576"] = dict(data=W.stream(frames, pcm, 24, 44100, 2, min_blocksize=576, max_blocksize=576), blocksize=576)

    # 4. variable blocking from sample 3 000 000 on (five bytes of coded number): 4096, 4608, 1000 (16-bit trailer), 100 (8-bit trailer)
    sizes = [4096, 4608, 1000, 100, 192, 37]
    pcm = tone(sum(sizes), 16, 4, 2, scale=0.05, noise=1)
    first = 3000000
    frames = [W.frame(p, 16, 48000, first + at, [dict(FIXED2, partition_order=6 if n == 4096 else 0), FIXED2], variable=True, stereo="mid_side", rate_form="streaminfo")
              for at, p in cut(pcm, sizes) for n in [len(p[0])]]
    out["variable_s16_stereo_48k"] = dict(data=W.stream(frames, pcm, 16, 48000, 2, min_blocksize=37, max_blocksize=4608, total_samples=0), blocksize=0, first_sample=first,
                                          samples=len(pcm))      # (total unknown: the reference's decoder stops where a known total is passed)

    # 5. eight channels, 16 bits, and six channels of 8 bits
    pcm = tone(576 * 2 + 100, 16, 5, 8, scale=0.1)
    frames = [W.frame(p, 16, 96000, k, [dict(type="fixed", order=c % 5) for c in range(8)]) for k, (_, p) in enumerate(cut(pcm, [576, 576, 100]))]
    out["wide_s16_8ch_96k_b576"] = dict(data=W.stream(frames, pcm, 16, 96000, 8, min_blocksize=576, max_blocksize=576), blocksize=576)
    pcm = tone(192 * 3, 8, 6, 6, noise=1)
    frames = [W.frame(p, 8, 32000, k, [dict(type="fixed", order=1)] * 6) for k, (_, p) in enumerate(cut(pcm, [192] * 3))]
    out["wide_s8_6ch_32k_b192"] = dict(data=W.stream(frames, pcm, 8, 32000, 6, min_blocksize=192, max_blocksize=192), blocksize=192)

    # 6. a planted false candidate: frame 1's left channel is VERBATIM and its first sample bytes spell a legal header of this very
    #    stream (fixed blocking, 576 samples, 44.1 kHz, two independent 16-bit channels, frame number 1) with a correct CRC-8
    pcm = tone(576 * 3, 16, 7, 2, scale=0.1)
    fake = W.header_bytes(576, 44100, 1, variable=False, assignment=1, bits=16)
    assert len(fake) == 6
    for j in range(3):
        v = int.from_bytes(fake[2 * j:2 * j + 2], "big")
        pcm[576 + j][0] = v - 65536 if v >= 32768 else v
    frames = [W.frame(p, 16, 44100, k, [dict(type="verbatim") if k == 1 else FIXED2, FIXED2]) for k, (_, p) in enumerate(cut(pcm, [576] * 3))]
    out["false_candidate_s16_stereo_44k1_b576"] = dict(data=W.stream(frames, pcm, 16, 44100, 2, min_blocksize=576, max_blocksize=576), blocksize=576)

    # 7. full-scale 24-bit audio through an LPC whose 64-bit sums pass 2^32: an alternating full-scale signal, coefficient -16383
    top = (1 << 23) - 1
    pcm = [[(top if i % 2 else -top - 1) - (i % 7) * (1 if i % 2 else -1), (-top - 1 if i % 2 else top - (i % 5))] for i in range(192 * 2)]
    big = dict(type="lpc", order=2, coefs=[-16383, 120], precision=15, shift=14)
    frames = [W.frame(p, 24, 48000, k, [big, dict(type="lpc", order=1, coefs=[-16383], precision=15, shift=14)]) for k, (_, p) in enumerate(cut(pcm, [192] * 2))]
    out["fullscale_lpc_s24_stereo_48k_b192"] = dict(data=W.stream(frames, pcm, 24, 48000, 2, min_blocksize=192, max_blocksize=192), blocksize=192)

    # 8. six short frames (mid/side, FIXED 1): the stream the malformed-input tests cut, flip and splice
    pcm = tone(16 * 6, 16, 8, 2, scale=0.02, noise=1)
    frames = [W.frame(p, 16, 44100, k, [dict(type="fixed", order=1)] * 2, stereo="mid_side") for k, (_, p) in enumerate(cut(pcm, [16] * 6))]
    out["tiny_s16_stereo_44k1_b16"] = dict(data=W.stream(frames, pcm, 16, 44100, 2, min_blocksize=16, max_blocksize=16), blocksize=16)

    # 9. far stream positions: three stereo frames of 16 samples each, entered where the coded number changes its length.  Variable
    #    blocking from sample 2^31 - 32 (six bytes, then seven at 2^31) and from 2^36 - 48 (the last 36-bit numbers); fixed blocking
    #    from the frame numbers at which the number grows from 1 to 2, 2 to 3 ... 5 to 6 bytes, and from 2^31 - 3 (the last 31-bit
    #    numbers): first_sample = number * 16 up to about 2^35.  Totals unknown, as for the variable stream above.
    for k, first in enumerate(FAR_VARIABLE):
        pcm = tone(16 * 3, 16, 10 + k, 2, scale=0.02, noise=1)
        frames = [W.frame(p, 16, 48000, first + at, [dict(type="fixed", order=1), FIXED2], variable=True, stereo="mid_side") for at, p in cut(pcm, [16] * 3)]
        out["variable_from_%s_s16_stereo_48k_b16" % FAR_VARIABLE[first]] = dict(
            data=W.stream(frames, pcm, 16, 48000, 2, min_blocksize=16, max_blocksize=16, total_samples=0), blocksize=0, first_sample=first, samples=48)
    for k, number in enumerate(FAR_FIXED):
        pcm = tone(16 * 3, 16, 20 + k, 2, scale=0.02, noise=1)
        frames = [W.frame(p, 16, 44100, number + j, [FIXED2, dict(type="fixed", order=1)], stereo="left_side" if k % 2 else None)
                  for j, (_, p) in enumerate(cut(pcm, [16] * 3))]
        out["fixed_from_frame_%s_s16_stereo_44k1_b16" % FAR_FIXED[number]] = dict(
            data=W.stream(frames, pcm, 16, 44100, 2, min_blocksize=16, max_blocksize=16, total_samples=0), blocksize=16, first_sample=number * 16, samples=48)
    return out


FAR_VARIABLE = {(1 << 31) - 32: "2p31m32", (1 << 36) - 48: "2p36m48"}
FAR_FIXED = {127: "127", 2047: "2047", 65535: "65535", (1 << 21) - 1: "2p21m1", (1 << 26) - 1: "2p26m1", (1 << 31) - 3: "2p31m3"}


def ask_the_reference_about_padding():
    """A frame whose padding bits are ones, CRC-16 right: does libFLAC 1.2.1 deliver it?"""
    import flac_ref as F
    pcm = tone(16 * 2, 16, 9, 1)
    good = [W.frame(p, 16, 44100, k, [dict(type="fixed", order=1)]) for k, (_, p) in enumerate(cut(pcm, [16, 16]))]
    bad = [W.frame(p, 16, 44100, k, [dict(type="fixed", order=1)], padding=0xff if k == 1 else 0) for k, (_, p) in enumerate(cut(pcm, [16, 16]))]
    if good[1] == bad[1]:
        return None                                              # (the frame happened to end on a byte boundary)
    F.decode(W.stream(good, pcm, 16, 44100, 1, min_blocksize=16, max_blocksize=16))
    try:
        frames, _ = F.decode(W.stream(bad, pcm, 16, 44100, 1, min_blocksize=16, max_blocksize=16))
        return "delivered %d frames without complaint" % len(frames)
    except AssertionError as e:
        return "refused: (ok, error statuses) = %s" % (e.args[0],)


def main():
    os.makedirs(OUT, exist_ok=True)
    try:
        import flac_ref as F
        ref = F if F.available() else None
    except Exception:
        ref = None
    index = {}
    for name, item in sorted(build().items()):
        data = item["data"]
        assert len(data) <= 65536, (name, len(data))
        info, audio = T.streaminfo(data)
        first = item.get("first_sample", 0)
        samples = item.get("samples", info["total_samples"])
        res = T.decode_range(data, audio, len(data) - audio, channels=info["channels"], bits=info["bits"], sample_rate=info["sample_rate"],
                             max_blocksize=info["max_blocksize"], max_samples=samples, blocksize=item["blocksize"],
                             first_sample=first, at_frame=True)
        assert res.status == T.OK and res.samples == samples and res.bytes_consumed == len(data) - audio, (name, res.status, res.samples)
        assert T.md5_of(res.frames, info["bits"]) == info["md5"], name
        if ref is not None:
            frames, md5_ok = ref.decode(data)
            assert md5_ok, name
            assert len(frames) == len(res.frames), name
            for (n, ch, bits, rate, pl), f in zip(frames, res.frames):
                assert (n, ch, bits, rate) == (f.header.blocksize, f.header.channels, f.header.bits, f.header.rate), name
                assert pl.tolist() == f.planes, name
        with open(os.path.join(OUT, name + ".flac"), "wb") as fh:
            fh.write(data)
        index[name] = dict(bytes=len(data), channels=info["channels"], bits=info["bits"], rate=info["sample_rate"], frames=len(res.frames),
                           samples=samples, blocksize=item["blocksize"], max_blocksize=info["max_blocksize"], first_sample=first,
                           candidates=res.candidates, md5=info["md5"].hex(), checked_with_reference=ref is not None,
                           census=dict(sorted(res.census.items())))
        print(name, len(data), "bytes,", len(res.frames), "frames,", res.candidates, "candidates")
    if ref is not None:
        print("non-zero padding bits in front of the CRC-16:", ask_the_reference_about_padding())
    with open(os.path.join(OUT, "index.json"), "w") as fh:
        json.dump(index, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
