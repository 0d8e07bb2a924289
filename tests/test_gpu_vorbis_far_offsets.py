"""The Vorbis decoder at arena offsets of 2^31 and more, in the manner of tests/test_gpu_ts_far_offsets.py: a small job laid twice into one
batch -- copy 0 near the arenas' start, copy 1 across byte 2^31, across byte 2^32 or beyond it -- inside the far blocks of
tests/far_cases.py, on either route and in both output forms.  Both copies' records must be the model's, and both destination windows
byte for byte what the same job writes into an arena of its own size (tests/test_gpu_vorbis_textbook.py holds that to the model), with
the guards and the alias windows untouched: the packets' src_offset, dst_offset and the plane stride are the 64-bit arithmetic at stake."""
import numpy as np
import pytest

import far_cases as FAR
import vorbis_cases as VC
import vorbis_frames as VF
import vorbis_textbook as TB
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu
FILL = 0xA5
JOB = [("stereo_256_2048", (3, 9)), ("six_128_512", (0, 16)), ("mono_64_128", (10, 40))]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arenas(ctx):
    a = FAR.FarArenas(ctx)                                   # (a failed allocation is an error here, not a skip)
    try:
        yield a
    finally:
        a.close()


def near_run(ctx, variant, blob, descs, packets, src, dst_bytes):
    ctx.set_kernel_variant(variant)
    try:
        b = ctx.vorbis_batch(descs, packets, blob, src.size, dst_bytes)
    finally:
        ctx.set_kernel_variant(0)
    d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
    ctx.memset(d_dst, FILL, dst_bytes)
    ctx.vorbis_run(b, d_src, d_dst)
    res, pres = ctx.vorbis_results(b, descs.size, packets.size)
    got = ctx.download(d_dst, dst_bytes)
    ctx.batch_destroy(b)
    ctx.free(d_src)
    ctx.free(d_dst)
    return res, pres, got


@pytest.mark.parametrize("pair", FAR.PAIRS)
@pytest.mark.parametrize("planar", [False, True], ids=["s16be", "planes"])
@pytest.mark.parametrize("variant", [0, 1], ids=["fft", "plain"])
def test_vorbis(ctx, arenas, variant, planar, pair):
    streams = [VC.stream(name) for name, _ in JOB]
    blob, descs, packets, src, dst_bytes, _ = VF.batch_tables(capi, streams, planar=planar, ranges=[r for _, r in JOB])
    res, pres, want = near_run(ctx, variant, blob, descs, packets, src, dst_bytes)
    assert (want != FILL).sum() > want.size // 3
    twin = FAR.Twin(arenas, src, np.full(dst_bytes, FILL, np.uint8), pair, 1, 4, FILL)
    twin.prepare()
    both_d, both_p = [], []
    for k in (0, 1):
        d, p = descs.copy(), packets.copy()
        d["dst_offset"] += np.uint64(twin.dst_at[k])
        d["first_packet"] += np.uint32(k * packets.size)
        p["src_offset"] += np.uint64(twin.src_at[k])
        both_d.append(d)
        both_p.append(p)
    d2, p2 = np.concatenate(both_d), np.concatenate(both_p)
    capi.vorbis_batch_check(d2, p2, blob, FAR.SPAN, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.vorbis_batch(d2, p2, blob, FAR.SPAN, FAR.SPAN)
    finally:
        ctx.set_kernel_variant(0)
    try:
        assert ctx.batch_paths(batch)["vorbis_route"] == (2 if variant else 1)
        ctx.vorbis_run(batch, arenas.src, arenas.dst)
        res2, pres2 = ctx.vorbis_results(batch, d2.size, p2.size)
    finally:
        ctx.batch_destroy(batch)
    for k in (0, 1):
        assert res2[k * descs.size:(k + 1) * descs.size].tobytes() == res.tobytes() and pres2[k * packets.size:(k + 1) * packets.size].tobytes() == pres.tobytes()
    for i, (name, (first, count)) in enumerate(JOB):
        recs = TB.decode_stream(streams[i].model, streams[i].packets[first:first + count])[0]
        at = int(descs["first_packet"][i])
        assert [(int(r["status"]), int(r["mode"]), int(r["blocksize"]), int(r["samples"]), int(r["position"])) for r in pres[at:at + count]] == [tuple(int(v) for v in r) for r in recs]
    twin.check(want, f"vorbis {pair}")
