"""Protected MPEG-4 end to end on the device.  fLaC (ohgpu_cenc_flac_process_host): the committed FLAC fixtures -- each with the MD5 of its
PCM in STREAMINFO -- cut into fragments, encrypted by the tests' own muxer (tests/cenc_cases.py), decrypted into a device-only middle
arena and decoded from there; the PCM must be what the clear fragmented stream decodes to (ohgpu_mp4f_flac_process_host) and have the
stream's MD5.  alac (ohgpu_cenc_alac_process_host): the committed Apple Lossless fixtures' PCM.  A wrong key under the right kid leaves
its neighbours exact and its own lane corrupt with nothing delivered; a stream without its key and a clear stream share the batch."""
import hashlib

import numpy as np
import pytest

import alac_cases as AC
import cenc_cases as CC
import cenc_textbook as CX
import mp4f_cases as FC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

ENCODED = ["s16_stereo_44k1_b1152_l5", "s24_stereo_44k1_b576_l0", "s8_mono_8k_b256_l2"]
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


class Call:
    """lanes: [(data, rows, runs, key or None, kid)] -> the descriptors of one fused fLaC call, filled from ohgpu_cenc_head as a caller
    would; clear=True makes the sibling's descriptors of the same layout"""

    def __init__(self, lanes, clear=False):
        n = len(lanes)
        self.descs = np.zeros(n, dtype=capi.MP4F_STREAM_DESC if clear else capi.CENC_STREAM_DESC)
        self.flac, self.clear = np.zeros(n, dtype=capi.FLAC_STREAM_DESC), clear
        src, mid, dst, row, run_row = bytearray(), 0, 0, 0, 0
        for i, (data, rows, runs, key, kid) in enumerate(lanes):
            src += bytes(i % 3)
            d, f = self.descs[i], self.flac[i]
            d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = len(src), len(data), 3, capi.MP4F_GATHER
            d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = row, rows, run_row, runs
            d["dst_offset"], d["dst_capacity"] = mid, len(data)
            if not clear:
                d["kid"] = np.frombuffer(kid, dtype=np.uint8)
                if key is not None:
                    d["key_flags"], d["key"] = capi.CENC_HAVE_KEY, np.frombuffer(key, dtype=np.uint8)
            head = capi.mp4f_head(data) if clear else capi.cenc_head(data)["mp4f"]
            flac = int(head["status"]) == capi.MP4F_OK and int(head["codec"]) == CX.code(b"fLaC")
            info = head["flac"]
            left = int(info["total_samples"]) if flac else 0
            f["src_offset"], f["dst_offset"], f["max_samples"] = mid, dst, left
            f["sample_rate"], f["max_blocksize"] = (int(info["sample_rate"]), int(info["max_blocksize"])) if flac else (44100, 4096)
            f["blocksize"] = int(info["max_blocksize"]) if flac and int(info["min_blocksize"]) == int(info["max_blocksize"]) else 0
            f["channels"], f["bits"] = (int(info["channels"]), int(info["bits"])) if flac else (1, 16)
            f["flags"] = capi.FLAC_FLAG_AT_FRAME | capi.FLAC_OUT_PACKED_BE
            src += data
            mid += len(data) + 5 + i
            dst += (left * int(f["channels"]) * (int(f["bits"]) // 8) + 3) // 4 * 4
            row += rows
            run_row += runs
        while len(src) % 4:
            src.append(0)
        self.src, self.mid_bytes, self.n_packets, self.n_runs = np.frombuffer(bytes(src), dtype=np.uint8), mid, row, run_row
        self.dst = np.full(max(dst, 4), FILL, dtype=np.uint8)

    def run(self, ctx):
        call = ctx.mp4f_flac_process_host if self.clear else ctx.cenc_flac_process_host
        self.res, self.runs, self.packets, self.samples, self.fres, self.frames = call(self.descs, self.flac, self.n_packets, self.n_runs, self.src, self.mid_bytes, self.dst, 4096)
        return self

    def pcm(self, i, width):
        a = int(self.flac[i]["dst_offset"])
        return self.dst[a:a + int(self.fres[i]["samples"]) * width].tobytes()


def test_protected_flac_decodes_to_the_clear_streams_pcm_and_its_md5(vctx):
    files = [CC.flac_file(name, per_fragment=(3, 5, 2)[i], key=CC.key_of(i), kid=CC.kid_of(i), iv_size=(8, 16)[i % 2]) for i, name in enumerate(ENCODED)]
    clear = [FC.flac_file(name, per_fragment=(3, 5, 2)[i]) for i, name in enumerate(ENCODED)]
    got = Call([(m.data, m.n, len(m.runs), m.key, m.kid) for m in files]).run(vctx)
    want = Call([(m.data, m.n, len(m.runs), None, None) for m in clear], clear=True).run(vctx)
    for i, m in enumerate(files):
        fx = m.fixture
        assert int(got.res[i]["mp4f"]["status"]) == capi.MP4F_OK and int(got.res[i]["mp4f"]["samples_available"]) == m.n and int(got.res[i]["is_protected"]) == 1, fx.name
        assert int(got.res[i]["mp4f"]["bytes_gathered"]) == len(fx.data) - fx.audio == int(want.res[i]["bytes_gathered"]), fx.name
        assert int(got.fres[i]["status"]) == capi.FLAC_OK and int(got.fres[i]["samples"]) == fx.samples, fx.name
        pcm = got.pcm(i, frame_bytes(fx))
        assert pcm == want.pcm(i, frame_bytes(fx)), fx.name
        assert md5_of_packed_be(pcm, fx) == bytes(got.res[i]["mp4f"]["flac"]["md5"]) == bytes(fx.info["md5"]), fx.name
    assert got.fres.tobytes() == want.fres.tobytes() and got.frames.tobytes() == want.frames.tobytes()


def test_a_wrong_key_corrupts_its_own_lane_alone(vctx):
    m = CC.flac_file("s16_stereo_44k1_b1152_l5", per_fragment=3)
    other = CC.flac_file("s8_mono_8k_b256_l2", per_fragment=4, key=CC.key_of(2), kid=CC.kid_of(2))
    clear = FC.flac_file("s8_mono_8k_b256_l2", per_fragment=4)
    lanes = [(m.data, m.n, len(m.runs), m.key, m.kid), (m.data, m.n, len(m.runs), CC.key_of(5), m.kid), (other.data, other.n, len(other.runs), other.key, other.kid),
             (other.data, other.n, len(other.runs), None, other.kid), (clear.data, clear.n, len(clear.runs), None, bytes(16))]
    call = Call(lanes).run(vctx)
    assert [int(r["mp4f"]["status"]) for r in call.res] == [capi.MP4F_OK, capi.MP4F_OK, capi.MP4F_OK, capi.CENC_NO_KEY, capi.MP4F_OK]
    w = frame_bytes(m.fixture)
    assert int(call.fres[0]["samples"]) == m.fixture.samples and md5_of_packed_be(call.pcm(0, w), m.fixture) == bytes(m.fixture.info["md5"])
    assert int(call.res[1]["mp4f"]["bytes_gathered"]) == int(call.res[0]["mp4f"]["bytes_gathered"])          # the demultiplexer cannot know ...
    assert int(call.fres[1]["status"]) != capi.FLAC_OK and int(call.fres[1]["samples"]) == 0                  # ... the decoder finds no frame: nothing delivered
    a = int(call.flac[1]["dst_offset"])
    assert (call.dst[a:int(call.flac[2]["dst_offset"])] == FILL).all()
    for i in (2, 4):
        assert int(call.fres[i]["samples"]) == other.fixture.samples and md5_of_packed_be(call.pcm(i, 1), other.fixture) == bytes(other.fixture.info["md5"]), i
    assert int(call.fres[3]["samples"]) == 0 and int(call.res[3]["mp4f"]["bytes_gathered"]) == 0 and bytes(call.res[3]["kid"]) == other.kid


def test_protected_alac_decodes_to_the_fixtures_pcm(vctx):
    names = ("stereo16_fl1024", "six16_fl256")
    files = [CC.alac_file(name, per_fragment=3, key=CC.key_of(i + 1), kid=CC.kid_of(i + 1), iv_size=(16, 8)[i]) for i, name in enumerate(names)]
    files.append(FC.alac_file(names[0], per_fragment=2))                                                  # a clear stream beside them
    keys = [(m.key, m.kid) for m in files[:2]] + [(None, bytes(16))]
    n = len(files)
    d, a = np.zeros(n, dtype=capi.CENC_STREAM_DESC), np.zeros(n, dtype=capi.ALAC_STREAM_DESC)
    src, mid, dst, row, run_row, spans = bytearray(), 0, 0, 0, 0, []
    for i, m in enumerate(files):
        src += bytes(1 + i)
        fx = m.fixture
        d[i]["src_offset"], d[i]["src_bytes"], d[i]["codecs"], d[i]["flags"] = len(src), len(m.data), 3, capi.MP4F_GATHER
        d[i]["packet_first"], d[i]["packet_capacity"], d[i]["run_first"], d[i]["run_capacity"] = row, m.n, run_row, len(m.runs)
        d[i]["dst_offset"], d[i]["dst_capacity"] = mid, sum(m.sizes)
        d[i]["kid"] = np.frombuffer(keys[i][1], dtype=np.uint8)
        if keys[i][0] is not None:
            d[i]["key_flags"], d[i]["key"] = capi.CENC_HAVE_KEY, np.frombuffer(keys[i][0], dtype=np.uint8)
        span = (len(fx["packets"]) * fx["cfg"]["frame_length"] * fx["cfg"]["channels"] * (fx["cfg"]["bit_depth"] // 8) + 3) // 4 * 4
        a[i]["dst_offset"], a[i]["flags"] = dst, capi.ALAC_OUT_PACKED_LE
        spans.append((dst, span))
        src += m.data
        mid += sum(m.sizes) + 3 + i
        dst += span
        row += m.n
        run_row += len(m.runs)
    src += bytes(-len(src) % 4)
    out = np.full(dst, FILL, dtype=np.uint8)
    res, runs, packets, samples, ares, pres = vctx.cenc_alac_process_host(d, a, row, run_row, np.frombuffer(bytes(src), dtype=np.uint8), mid, out)
    for i, m in enumerate(files):
        fx = m.fixture
        assert int(res[i]["mp4f"]["status"]) == capi.MP4F_OK and int(res[i]["mp4f"]["samples_available"]) == m.n and int(res[i]["mp4f"]["frames"]) == fx["meta"]["frames"]
        assert int(res[i]["is_protected"]) == (1 if i < 2 else 0) and int(res[i]["blocks"]) == (sum((s + 15) // 16 for s in m.sizes) if i < 2 else 0)
        at, span = spans[i]
        assert out[at:at + len(fx["pcm"])].tobytes() == fx["pcm"], fx["name"] if "name" in fx else i
        first = int(d[i]["packet_first"])
        assert [int(p["bytes"]) for p in packets[first:first + m.n]] == m.sizes and int(packets[first]["src_offset"]) == int(d[i]["dst_offset"])
