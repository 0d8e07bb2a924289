"""Both layers at arena offsets of 2^31 and more, in the manner of tests/test_gpu_raop_rx_far_offsets.py: a small job laid twice into one
batch -- copy 0 near the arenas' start, copy 1 across byte 2^31, across byte 2^32 or beyond it -- inside the far blocks of
tests/far_cases.py, run once on either route.  Both copies' results and records must be the model's of the near layout, both
destination windows the model's arena with the guards and the alias windows untouched.  The ADTS layer writes to no arena: its
destination window comes back as it went in."""
import numpy as np
import pytest

import far_cases as FAR
import ts_cases as TC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu
FILL = 0xA5


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


def both(descs, twin, src_only=False):
    out = []
    for k in (0, 1):
        d = descs.copy()
        d["src_offset"] += np.uint64(twin.src_at[k])
        if not src_only:
            d["dst_offset"] += np.uint64(twin.dst_at[k])
        out.append(d)
    return np.concatenate(out)


@pytest.mark.parametrize("pair", FAR.PAIRS)
@pytest.mark.parametrize("variant", [0, 1], ids=["launches", "plain"])
def test_ts(ctx, arenas, variant, pair):
    named = TC.named()
    job = TC.Job([named["ten_pes"], named["every_payload_length"], named["counter_jumps"], named["before_first_start_open_less"], named["corrupt"]])
    n = len(job.streams)
    twin = FAR.Twin(arenas, job.src, job.dst0, pair, 1, 1, FILL)
    twin.prepare()
    descs = both(job.descs, twin)
    descs["pes_first"][n:] += job.n_pes
    capi.ts_batch_check(descs, 2 * job.n_pes, FAR.SPAN, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.ts_batch(descs, 2 * job.n_pes, FAR.SPAN, FAR.SPAN)
    finally:
        ctx.set_kernel_variant(0)
    try:
        assert ctx.ts_paths(batch)["route"] == (2 if variant else 1)
        ctx.ts_run(batch, arenas.src, arenas.dst)
        results, pes = ctx.ts_results(batch, 2 * n, 2 * job.n_pes)
    finally:
        ctx.batch_destroy(batch)
    for k in (0, 1):
        TC.assert_same(results[k * n:(k + 1) * n], pes[k * job.n_pes:(k + 1) * job.n_pes], job.want, job)   # (es_offset is from the run's start: unmoved)
    twin.check(job.want, f"ts {pair}")


@pytest.mark.parametrize("pair", FAR.PAIRS)
@pytest.mark.parametrize("variant", [0, 1], ids=["launches", "plain"])
def test_adts(ctx, arenas, variant, pair):
    named = TC.adts_named()
    job = TC.AdtsJob([named["plain"], named["junk_between"], named["recognise_four_then_five"], named["start_at_2049"], named["largest"]])
    n = len(job.streams)
    untouched = np.full(64, FILL, np.uint8)
    twin = FAR.Twin(arenas, job.src, untouched, pair, 1, 1, FILL)
    twin.prepare()
    descs = both(job.descs, twin, src_only=True)
    descs["frame_first"][n:] += job.n_frames
    capi.adts_batch_check(descs, 2 * job.n_frames, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.adts_batch(descs, 2 * job.n_frames, FAR.SPAN)
    finally:
        ctx.set_kernel_variant(0)
    try:
        assert ctx.adts_paths(batch)["route"] == (2 if variant else 1)
        ctx.adts_run(batch, arenas.src)
        results, frames = ctx.adts_results(batch, 2 * n, 2 * job.n_frames)
    finally:
        ctx.batch_destroy(batch)
    for k in (0, 1):
        TC.assert_same_adts(results[k * n:(k + 1) * n], frames[k * job.n_frames:(k + 1) * job.n_frames], job)
    twin.check(untouched, f"adts {pair}")
