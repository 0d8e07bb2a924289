"""Apple Lossless in an MPEG-4 container end to end on the device (ohgpu_mp4_alac_process_host): the committed encoder-made fixtures
wrapped into .m4a files by the tests' own muxer (tests/mp4_cases.py) -- moov first and last, stco and co64, three chunkings -- go in as
file bytes and must come out as the PCM they were encoded from, byte for byte and by SHA-256, in the decoder's packed little-endian
form and as planes, with every byte of the destination arena that is no sample left as it was.  A file cut in the middle of mdat
delivers exactly samples_available packets' worth; a file with a damaged stsz is reported and its neighbours stay exact.  Both routes."""
import struct

import numpy as np
import pytest

import alac_cases as AC
import mp4_cases as MC
import mp4_textbook as MX
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xa5
CHUNKINGS = ([1 << 20], [1], [3])


@pytest.fixture(scope="module", params=[0, 1], ids=["fused", "plain"])
def vctx(request):
    c = capi.Context(0)
    c.set_kernel_variant(request.param)
    yield c
    c.set_kernel_variant(0)
    c.close()


def expected(fx, form, packets_decoded):
    """the fixture's own PCM for its first packets_decoded packets, in the output form: bytes (packed) or a list of planes"""
    fl = fx["cfg"]["frame_length"]
    frames = min(packets_decoded * fl, fx["meta"]["frames"])
    if form == capi.ALAC_OUT_PACKED_LE:
        return fx["pcm"][:frames * fx["cfg"]["channels"] * (fx["cfg"]["bit_depth"] // 8)]
    return [struct.pack("<%di" % frames, *[row[c] for row in fx["samples"][:frames]]) for c in range(fx["cfg"]["channels"])]


class Call:
    """lanes: [(fixture, file bytes, packets that must decode)] -> the descriptors of one fused call and the arena it must leave"""

    def __init__(self, lanes, form):
        n = len(lanes)
        self.lanes, self.form = lanes, form
        self.mp4, self.alac = np.zeros(n, dtype=capi.MP4_STREAM_DESC), np.zeros(n, dtype=capi.ALAC_STREAM_DESC)
        src, at, row = bytearray(), GUARD, 0
        want = bytearray()
        for i, (fx, data, decoded) in enumerate(lanes):
            src += bytes(i % 5)                                               # (files at different alignments)
            cap = len(fx["packets"])
            self.mp4[i]["src_offset"], self.mp4[i]["src_bytes"], self.mp4[i]["packet_first"], self.mp4[i]["packet_capacity"] = len(src), len(data), row, cap
            src += data
            row += cap
            cfg = fx["cfg"]
            span = cap * cfg["frame_length"]
            self.alac[i]["dst_offset"], self.alac[i]["flags"] = at, form
            want += bytes([FILL]) * (at - len(want))
            exp = expected(fx, form, decoded)
            if form:
                want += exp
                at += (span * cfg["channels"] * (cfg["bit_depth"] // 8) + 3) // 4 * 4 + GUARD
            else:
                stride = span * 4 + GUARD
                self.alac[i]["dst_plane_stride"] = stride
                for c, plane in enumerate(exp):
                    want += bytes([FILL]) * (at + c * stride - len(want)) + plane
                at += cfg["channels"] * stride
        want += bytes([FILL]) * (at - len(want))
        self.src, self.n_packets, self.want = np.frombuffer(bytes(src), dtype=np.uint8), row, bytes(want)

    def run(self, ctx):
        dst = np.full(len(self.want), FILL, dtype=np.uint8)
        out = ctx.mp4_alac_process_host(self.mp4, self.alac, self.n_packets, self.src, dst)
        bad = np.flatnonzero(dst != np.frombuffer(self.want, dtype=np.uint8))
        assert bad.size == 0, f"{bad.size} bytes of the destination arena differ, the first at {bad[0]}"
        return out, dst


@pytest.mark.parametrize("form", [capi.ALAC_OUT_PACKED_LE, 0], ids=["packed_le", "planes"])
def test_every_fixture_in_every_wrapping_comes_out_as_its_pcm(vctx, form):
    lanes = []
    for fx in AC.fixtures():
        for moov_last in (False, True):
            for co64 in (False, True):
                for per_chunk in CHUNKINGS:
                    lanes.append((fx, MC.fixture_file(fx, moov_last=moov_last, co64=co64, per_chunk=per_chunk).data, len(fx["packets"])))
    assert len(lanes) == 11 * 2 * 2 * 3
    call = Call(lanes, form)
    (mres, packets, samples, ares, pres), dst = call.run(vctx)
    assert all(int(r["status"]) == capi.MP4_OK and int(r["samples_refused"]) == 0 for r in mres)
    for i, (fx, _, _) in enumerate(lanes):
        assert int(ares[i]["packets_ok"]) == len(fx["packets"]) and int(ares[i]["samples"]) == fx["meta"]["frames"] == int(mres[i]["frames"])
        if form:
            at = int(call.alac[i]["dst_offset"])
            assert AC.sha256(dst[at:at + len(fx["pcm"])].tobytes()) == fx["meta"]["pcm_sha256"] == AC.sha256(fx["pcm"])
    assert all(int(p["status"]) == capi.ALAC_OK for p in pres)


def test_a_file_cut_in_mdat_and_a_damaged_stsz_between_exact_neighbours(vctx):
    fx, other = AC.load_fixture("stereo16_fl1024"), AC.load_fixture("stereo24_fl1024")
    m = MC.fixture_file(fx, per_chunk=[2])
    cut = m.data[:m.offsets[2] + m.sizes[2] // 2]                             # the middle of the third packet
    stsz = m.find("stsz")
    damaged = MC.patched(m, stsz[1] + 12 + 4, m.sizes[1] - 9)                 # the second sample nine bytes short; it is the last of its chunk, so nothing behind it moves
    broken = MC.patched(m, stsz[1] + 8, 0x00ffffff)                           # a sample count the box has no room for
    whole = MC.fixture_file(other, moov_last=True, co64=True)
    model_cut, model_damaged = MX.demux(cut, 4), MX.demux(damaged, 4)
    assert (model_cut["status"], model_cut["samples_available"], model_cut["samples_refused"]) == (MX.OK, 2, 2)
    assert model_damaged["status"] == MX.OK and MX.demux(broken, 4)["status"] == MX.INVALID
    call = Call([(other, whole.data, 4), (fx, cut, 2), (other, whole.data, 4), (fx, broken, 0), (fx, m.data, 4)], capi.ALAC_OUT_PACKED_LE)
    (mres, packets, samples, ares, pres), _ = call.run(vctx)
    assert [int(r["status"]) for r in mres] == [MX.OK, MX.OK, MX.OK, MX.INVALID, MX.OK]
    assert int(mres[1]["samples_available"]) == 2 == int(ares[1]["packets_ok"]) and int(ares[1]["samples"]) == 2 * 1024
    assert int(ares[1]["first_bad_status"]) == capi.ALAC_CORRUPT                # the zero-byte row of a refused sample
    assert int(ares[3]["packets_ok"]) == 0 and int(ares[3]["samples"]) == 0 and int(mres[3]["error_offset"]) == stsz[0]
    assert [int(a["packets_ok"]) for a in ares[[0, 2, 4]]] == [4, 4, 4]
    one = Call([(fx, damaged, 1)], capi.ALAC_OUT_PACKED_LE)
    mp4 = vctx.mp4_process_host(one.mp4, one.n_packets, one.src)
    assert int(mp4[0][0]["status"]) == MX.OK and int(mp4[1][1]["bytes"]) == m.sizes[1] - 9
