"""Fragmented MPEG-4 end to end on the device.  fLaC (ohgpu_mp4f_flac_process_host): the committed FLAC fixtures -- encoded by the
reference's libFLAC, each with the MD5 of its PCM in STREAMINFO -- cut into fragments by the tests' own muxer (tests/mp4f_cases.py),
demultiplexed and gathered into a device-only middle arena and decoded from there; the PCM must have the stream's MD5 and be the bytes
the native stream decodes to.  alac (ohgpu_mp4f_alac_process_host): byte for byte what ohgpu_mp4_alac_process_host gives for the same
packets in a plain .m4a.  A prefix of a stream plays its whole fragments; a seek to a frame in the third fragment delivers from that
sample's first frame; fLaC, alac, a refused stream and an empty one share a batch."""
import hashlib

import numpy as np
import pytest

import alac_cases as AC
import flac_cases as FLC
import mp4_cases as MC
import mp4f_cases as FC
import mp4f_textbook as FX
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

ENCODED = ["s16_stereo_44k1_b1152_l5", "s24_stereo_44k1_b576_l0", "s8_mono_8k_b256_l2", "s24_6ch_48k_b4608_l3"]
FILL = 0xa5


@pytest.fixture(scope="module", params=[0, 1], ids=["phases", "plain"])
def vctx(request):
    c = capi.Context(0)
    c.set_kernel_variant(request.param)
    yield c
    c.set_kernel_variant(0)
    c.close()


def frame_bytes(fx):
    return fx.info["channels"] * (fx.info["bits"] // 8)


def md5_of_packed_be(pcm, fx):
    """STREAMINFO's MD5 is over the interleaved samples, little-endian: the packed big-endian output with every sample reversed."""
    w = fx.info["bits"] // 8
    return hashlib.md5(np.frombuffer(pcm, dtype=np.uint8).reshape(-1, w)[:, ::-1].tobytes()).digest()


def native_pcm(ctx, fx):
    case = FLC.whole(fx, packed=True)
    d = np.zeros(1, dtype=capi.FLAC_STREAM_DESC)
    d["src_offset"], d["src_bytes"], d["max_samples"], d["sample_rate"] = case.offset, case.src_bytes, case.max_samples, case.rate
    d["blocksize"], d["max_blocksize"], d["channels"], d["bits"], d["flags"] = case.blocksize, case.max_blocksize, case.channels, case.bits, case.flags
    dst = np.zeros(case.max_samples * frame_bytes(fx), dtype=np.uint8)
    res = ctx.flac_process_host(d, np.frombuffer(fx.data, dtype=np.uint8), dst)
    assert int(res[0]["status"]) == capi.FLAC_OK and int(res[0]["samples"]) == fx.samples
    return dst.tobytes()


class Call:
    """lanes: [(Fragmented with .fixture or None, bytes, gather_first_row, first_sample)] -> the descriptors of one fused fLaC call.  The
    FLAC descriptor is filled from ohgpu_mp4f_head, as a caller would."""

    def __init__(self, lanes):
        n = len(lanes)
        self.lanes = lanes
        self.mp4f, self.flac = np.zeros(n, dtype=capi.MP4F_STREAM_DESC), np.zeros(n, dtype=capi.FLAC_STREAM_DESC)
        src, mid, dst, row, run_row = bytearray(), 0, 0, 0, 0
        for i, (m, data, first_row, first_sample) in enumerate(lanes):
            src += bytes(i % 3)
            d, f = self.mp4f[i], self.flac[i]
            rows, runs = (m.n, len(m.runs)) if m is not None else (4, 2)
            d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = len(src), len(data), 3, capi.MP4F_GATHER
            d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = row, rows, run_row, runs
            d["gather_first_row"], d["dst_offset"], d["dst_capacity"] = first_row, mid, len(data)
            head = capi.mp4f_head(data)
            flac = int(head["status"]) == capi.MP4F_OK and int(head["codec"]) == FX.code(b"fLaC")
            info = head["flac"]
            left = int(info["total_samples"]) - first_sample if flac else 0
            f["src_offset"], f["dst_offset"], f["first_sample"], f["max_samples"] = mid, dst, first_sample, left
            f["sample_rate"], f["max_blocksize"] = (int(info["sample_rate"]), int(info["max_blocksize"])) if flac else (44100, 4096)
            f["blocksize"] = int(info["max_blocksize"]) if flac and int(info["min_blocksize"]) == int(info["max_blocksize"]) else 0
            f["channels"], f["bits"] = (int(info["channels"]), int(info["bits"])) if flac else (1, 16)
            f["flags"] = capi.FLAC_FLAG_AT_FRAME | capi.FLAC_OUT_PACKED_BE
            self_bytes = left * int(info["channels"]) * (int(info["bits"]) // 8) if flac else 0
            src += data
            mid += len(data) + 5 + i
            dst += (self_bytes + 3) // 4 * 4
            row += rows
            run_row += runs
        while len(src) % 4:
            src.append(0)
        self.src, self.mid_bytes, self.n_packets, self.n_runs = np.frombuffer(bytes(src), dtype=np.uint8), mid, row, run_row
        self.dst = np.full(max(dst, 4), FILL, dtype=np.uint8)

    def run(self, ctx):
        self.res, self.runs, self.packets, self.samples, self.fres, self.frames = ctx.mp4f_flac_process_host(self.mp4f, self.flac, self.n_packets, self.n_runs, self.src,
                                                                                                              self.mid_bytes, self.dst, 4096)
        return self

    def pcm(self, i, width):
        a = int(self.flac[i]["dst_offset"])
        return self.dst[a:a + int(self.fres[i]["samples"]) * width].tobytes()


def test_every_encoded_fixture_has_its_md5_and_its_native_pcm(vctx):
    files = [FC.flac_file(name, per_fragment=(3, 5, 1, 2)[i]) for i, name in enumerate(ENCODED)]
    call = Call([(m, m.data, 0, 0) for m in files]).run(vctx)
    for i, m in enumerate(files):
        fx = m.fixture
        assert int(call.res[i]["status"]) == capi.MP4F_OK and int(call.res[i]["samples_available"]) == m.n == len(FLC.frame_spans(fx.name)), fx.name
        assert int(call.res[i]["bytes_gathered"]) == len(fx.data) - fx.audio and int(call.res[i]["frames"]) == fx.samples == int(call.res[i]["duration"]), fx.name
        assert int(call.fres[i]["status"]) == capi.FLAC_OK and int(call.fres[i]["samples"]) == fx.samples, fx.name
        pcm = call.pcm(i, frame_bytes(fx))
        assert md5_of_packed_be(pcm, fx) == bytes(call.res[i]["flac"]["md5"]) == bytes(fx.info["md5"]), fx.name
        assert pcm == native_pcm(vctx, fx), fx.name
        frames = call.frames[call.frames["stream"] == i]
        assert [int(f["first_sample"]) for f in frames] == m.first_frames and [int(f["blocksize"]) for f in frames] == m.frames, fx.name


def test_a_prefix_plays_its_whole_fragments_and_a_seek_lands_in_the_third(vctx):
    m = FC.flac_file("s16_stereo_44k1_b1152_l5", per_fragment=2)
    fx = m.fixture
    whole = native_pcm(vctx, fx)
    w = frame_bytes(fx)
    prefix = m.data[:m.segment_ends[2] + (m.segment_ends[3] - m.segment_ends[2]) // 2]      # three fragments and half of the fourth: its moof is whole, its frames are not
    # the seek: a frame in the middle of the third fragment's second sample
    model = FX.demux(m.data)
    frame = m.first_frames[5] + m.frames[5] // 2
    samples = np.array(model["samples_rows"], dtype=capi.MP4_SAMPLE)
    index, first = capi.mp4_seek(samples, frame)
    assert (index, first) == (5, m.first_frames[5]) and m.run_of[5] == 2
    call = Call([(m, prefix, 0, 0), (m, m.data, index, first)]).run(vctx)
    assert int(call.res[0]["samples_available"]) == 6 and int(call.res[0]["samples"]) == 8 and int(call.res[0]["samples_refused"]) == 2
    assert int(call.fres[0]["samples"]) == m.first_frames[6] and call.pcm(0, w) == whole[:m.first_frames[6] * w]
    assert int(call.fres[1]["first_sample_decoded"]) == first and int(call.fres[1]["samples"]) == fx.samples - first
    assert call.pcm(1, w) == whole[first * w:]


def alac_descs(fx, at, form, n):
    a = np.zeros(n, dtype=capi.ALAC_STREAM_DESC)
    span = len(fx["packets"]) * fx["cfg"]["frame_length"] * fx["cfg"]["channels"] * (fx["cfg"]["bit_depth"] // 8)
    a[0]["dst_offset"], a[0]["flags"] = at, form
    return a, (span + 3) // 4 * 4


def test_fragmented_alac_is_what_the_plain_file_decodes_to(vctx):
    for name in ("stereo16_fl1024", "six16_fl256"):
        fx = AC.load_fixture(name)
        m = FC.alac_file(name, per_fragment=3)
        plain = MC.fixture_file(fx, per_chunk=[2])
        a, span = alac_descs(fx, 0, capi.ALAC_OUT_PACKED_LE, 1)
        d = np.zeros(1, dtype=capi.MP4F_STREAM_DESC)
        d["src_bytes"], d["codecs"], d["packet_capacity"], d["run_capacity"] = len(m.data), 3, m.n, len(m.runs)
        src = np.frombuffer(m.data + bytes(-len(m.data) % 4), dtype=np.uint8)
        dst = np.full(span, FILL, dtype=np.uint8)
        res, runs, packets, samples, ares, pres = vctx.mp4f_alac_process_host(d, a, m.n, len(m.runs), src, dst)
        p = np.zeros(1, dtype=capi.MP4_STREAM_DESC)
        p["src_bytes"], p["packet_capacity"] = len(plain.data), plain.n
        want = np.full(span, FILL, dtype=np.uint8)
        pres_plain = vctx.mp4_alac_process_host(p, a, plain.n, np.frombuffer(plain.data + bytes(-len(plain.data) % 4), dtype=np.uint8), want)
        assert int(res[0]["status"]) == capi.MP4F_OK and int(res[0]["samples_available"]) == m.n and int(res[0]["frames"]) == fx["meta"]["frames"]
        assert np.array_equal(dst, want) and dst[:len(fx["pcm"])].tobytes() == fx["pcm"]
        assert ares.tobytes() == pres_plain[3].tobytes() and pres.tobytes() == pres_plain[4].tobytes()
        assert [(int(s["first_frame"]), int(s["frames"])) for s in samples] == [(int(s["first_frame"]), int(s["frames"])) for s in pres_plain[2]]


def test_flac_alac_a_refused_stream_and_an_empty_one_together(vctx):
    m = FC.flac_file("s8_mono_8k_b256_l2", per_fragment=4)
    alac = FC.alac_file("stereo16_fl1024")
    refused = FC.named_malformed()["trun_entries_leave_the_box"][0]
    call = Call([(m, m.data, 0, 0), (alac, alac.data, 0, 0), (None, refused, 0, 0), (None, b"", 0, 0), (m, m.data, 0, 0)]).run(vctx)
    assert [int(r["status"]) for r in call.res] == [capi.MP4F_OK, capi.MP4F_OK, capi.MP4F_INVALID, capi.MP4F_TRUNCATED, capi.MP4F_OK]
    assert int(call.res[1]["codec"]) == FX.code(b"alac") and int(call.res[1]["samples_available"]) == alac.n and int(call.res[1]["bytes_gathered"]) == sum(alac.sizes)
    assert [int(f["samples"]) for f in call.fres] == [m.fixture.samples, 0, 0, 0, m.fixture.samples]
    whole = native_pcm(vctx, m.fixture)
    assert call.pcm(0, 1) == whole and call.pcm(4, 1) == whole
