"""The second protected MPEG-4 family end to end on the device.  fLaC (ohgpu_cbcs_flac_process_host): committed FLAC fixtures -- each with
the MD5 of its PCM in STREAMINFO -- cut into fragments and encrypted by the tests' own muxer (tests/cbcs_cases.py) under `cbcs` with pattern
1:9 and a constant IV, under `cbcs` with subsample entries, and under `cenc` with subsample entries; decrypted into a device-only middle
arena and decoded from there.  The PCM must be what the same audio muxed clear decodes to (ohgpu_mp4f_flac_process_host) and have the
stream's MD5.  alac (ohgpu_cbcs_alac_process_host): the committed Apple Lossless fixtures' PCM, under `cbcs` 1:9 and under `cbcs` with
entries, a clear stream beside them."""
import hashlib

import numpy as np
import pytest

import cbcs_cases as BC
import cenc_textbook as CX
import mp4f_cases as FC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

ENCODED = ["s16_stereo_44k1_b1152_l5", "s24_stereo_44k1_b576_l0", "s8_mono_8k_b256_l2"]
FILL = 0xa5
HOW = [dict(pattern=(1, 9), constant_iv=bytes(range(0x70, 0x80)), senc=None),
       dict(iv_size=8, pattern=(1, 1), layout=lambda i, size: [(min(size, 9), max(size - 9 - 4, 0)), (min(max(size - 9, 0), 4), 0)]),
       dict(scheme=BC.CENC, iv_size=16, layout=lambda i, size: [(min(size, 4), (size - min(size, 4)) // 2), (0, size - min(size, 4) - (size - min(size, 4)) // 2)])]


@pytest.fixture(scope="module", params=[0, 1], ids=["phases", "plain"])
def vctx(request):
    c = capi.Context(0)
    c.set_kernel_variant(request.param)
    yield c
    c.set_kernel_variant(0)
    c.close()


flac_file, alac_file = BC.flac_file, BC.alac_file


def md5_of_packed_be(pcm, fx):
    w = fx.info["bits"] // 8
    return hashlib.md5(np.frombuffer(pcm, dtype=np.uint8).reshape(-1, w)[:, ::-1].tobytes()).digest()


def flac_call(ctx, files, clear):
    n = len(files)
    descs = np.zeros(n, dtype=capi.MP4F_STREAM_DESC if clear else capi.CBCS_STREAM_DESC)
    flac = np.zeros(n, dtype=capi.FLAC_STREAM_DESC)
    src, mid, dst, row, run_row, sub_row = bytearray(), 0, 0, 0, 0, 0
    for i, m in enumerate(files):
        src += bytes(i % 3)
        d, f = descs[i], flac[i]
        d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = len(src), len(m.data), 3, capi.MP4F_GATHER
        d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = row, m.n, run_row, len(m.runs)
        d["dst_offset"], d["dst_capacity"] = mid, len(m.data)
        if not clear:
            d["kid"], d["key_flags"], d["key"] = np.frombuffer(m.kid, dtype=np.uint8), capi.CENC_HAVE_KEY, np.frombuffer(m.key, dtype=np.uint8)
            d["subsample_first"], d["subsample_capacity"] = sub_row, m.subsamples
            sub_row += m.subsamples
        head = capi.mp4f_head(m.data) if clear else capi.cbcs_head(m.data)["cenc"]["mp4f"]
        assert int(head["status"]) == capi.MP4F_OK and int(head["codec"]) == CX.code(b"fLaC")
        info = head["flac"]
        f["src_offset"], f["dst_offset"], f["max_samples"] = mid, dst, int(info["total_samples"])
        f["sample_rate"], f["max_blocksize"], f["blocksize"] = int(info["sample_rate"]), int(info["max_blocksize"]), int(info["max_blocksize"]) if int(info["min_blocksize"]) == int(info["max_blocksize"]) else 0
        f["channels"], f["bits"], f["flags"] = int(info["channels"]), int(info["bits"]), capi.FLAC_FLAG_AT_FRAME | capi.FLAC_OUT_PACKED_BE
        src += m.data
        mid += len(m.data) + 5 + i
        dst += (int(info["total_samples"]) * int(f["channels"]) * (int(f["bits"]) // 8) + 3) // 4 * 4
        row += m.n
        run_row += len(m.runs)
    src += bytes(-len(src) % 4)
    out = np.full(max(dst, 4), FILL, dtype=np.uint8)
    source = np.frombuffer(bytes(src), dtype=np.uint8)
    if clear:
        res, _, _, _, fres, frames = ctx.mp4f_flac_process_host(descs, flac, row, run_row, source, mid, out, 4096)
    else:
        res, _, _, _, fres, frames = ctx.cbcs_flac_process_host(descs, flac, row, run_row, sub_row, source, mid, out, 4096)
    pcm = [out[int(f["dst_offset"]):int(f["dst_offset"]) + int(r["samples"]) * int(f["channels"]) * (int(f["bits"]) // 8)].tobytes() for f, r in zip(flac, fres)]
    return res, fres, frames, pcm


def test_protected_flac_decodes_to_the_clear_streams_pcm_and_its_md5(vctx):
    made = [flac_file(name, (3, 5, 2)[i], 1 + i, **HOW[i]) for i, name in enumerate(ENCODED)]
    files, clear = [m for m, _ in made], [base for _, base in made]
    assert [m.subsamples for m in files] == [0, 2 * files[1].n, 2 * files[2].n] and [m.pattern for m in files] == [(1, 9), (1, 1), (0, 0)]
    res, fres, frames, pcm = flac_call(vctx, files, False)
    cres, cfres, cframes, cpcm = flac_call(vctx, clear, True)
    for i, m in enumerate(files):
        fx = m.fixture
        r = res[i]
        assert int(r["cenc"]["mp4f"]["status"]) == capi.MP4F_OK and int(r["cenc"]["mp4f"]["samples_available"]) == m.n and int(r["cenc"]["is_protected"]) == 1, fx.name
        assert int(r["cenc"]["scheme"]) == CX.code(m.scheme) and (int(r["crypt_blocks"]), int(r["skip_blocks"])) == m.pattern and int(r["subsamples"]) == m.subsamples
        assert int(r["cenc"]["mp4f"]["bytes_gathered"]) == int(cres[i]["bytes_gathered"]) and int(r["cenc"]["blocks"]) > 0, fx.name
        assert int(fres[i]["status"]) == capi.FLAC_OK and int(fres[i]["samples"]) == fx.samples, fx.name
        assert pcm[i] == cpcm[i] and md5_of_packed_be(pcm[i], fx) == bytes(fx.info["md5"]), fx.name
    assert fres.tobytes() == cfres.tobytes() and frames.tobytes() == cframes.tobytes()


def test_protected_alac_decodes_to_the_fixtures_pcm(vctx):
    names = ("stereo16_fl1024", "six16_fl256")
    files = [alac_file(names[0], 3, 4, **HOW[0]), alac_file(names[1], 3, 5, **HOW[1]), FC.alac_file(names[0], per_fragment=2)]
    n = len(files)
    d, a = np.zeros(n, dtype=capi.CBCS_STREAM_DESC), np.zeros(n, dtype=capi.ALAC_STREAM_DESC)
    src, mid, dst, row, run_row, sub_row, spans = bytearray(), 0, 0, 0, 0, 0, []
    for i, m in enumerate(files):
        src += bytes(1 + i)
        fx = m.fixture
        d[i]["src_offset"], d[i]["src_bytes"], d[i]["codecs"], d[i]["flags"] = len(src), len(m.data), 3, capi.MP4F_GATHER
        d[i]["packet_first"], d[i]["packet_capacity"], d[i]["run_first"], d[i]["run_capacity"] = row, m.n, run_row, len(m.runs)
        d[i]["dst_offset"], d[i]["dst_capacity"] = mid, sum(m.sizes)
        if i < 2:
            d[i]["kid"], d[i]["key_flags"], d[i]["key"] = np.frombuffer(m.kid, dtype=np.uint8), capi.CENC_HAVE_KEY, np.frombuffer(m.key, dtype=np.uint8)
            d[i]["subsample_first"], d[i]["subsample_capacity"] = sub_row, m.subsamples
            sub_row += m.subsamples
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
    res, runs, packets, samples, ares, pres = vctx.cbcs_alac_process_host(d, a, row, run_row, sub_row, np.frombuffer(bytes(src), dtype=np.uint8), mid, out)
    for i, m in enumerate(files):
        fx = m.fixture
        r = res[i]["cenc"]
        assert int(r["mp4f"]["status"]) == capi.MP4F_OK and int(r["mp4f"]["samples_available"]) == m.n and int(r["mp4f"]["frames"]) == fx["meta"]["frames"]
        assert int(r["is_protected"]) == (1 if i < 2 else 0) and (int(r["blocks"]) > 0) == (i < 2) and int(res[i]["subsamples"]) == (2 * m.n if i == 1 else 0)
        at, span = spans[i]
        assert out[at:at + len(fx["pcm"])].tobytes() == fx["pcm"], i
        first = int(d[i]["packet_first"])
        assert [int(p["bytes"]) for p in packets[first:first + m.n]] == m.sizes and int(packets[first]["src_offset"]) == int(d[i]["dst_offset"])
