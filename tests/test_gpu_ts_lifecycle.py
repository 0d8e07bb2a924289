"""The transport stream and ADTS batches' lives on the device, the pins tests/test_gpu_raop_rx_lifecycle.py makes for its family: results
before a run, create / run / run / destroy with ohgpu_device_allocations unchanged by the second run, runs and results in any order, a
run on a second HIP stream behind one on the first, a batch of another kind, and the context's block cache over create / destroy
cycles.  Both routes of both layers."""
import numpy as np
import pytest

import ts_cases as TC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def job():
    named = TC.named()
    return TC.Job([named["ten_pes"], named["packets_0"], named["counter_jumps"], named["corrupt"], named["every_payload_length"]])


@pytest.fixture(scope="module")
def ajob():
    named = TC.adts_named()
    return TC.AdtsJob([named["plain"], named["empty"], named["junk_between"], named["recognise_four_then_five"], named["start_at_2049"]])


def create(ctx, variant, make):
    ctx.set_kernel_variant(variant)
    try:
        return make()
    finally:
        ctx.set_kernel_variant(0)


def refused(call, text):
    with pytest.raises(capi.OhGpuError) as e:
        call()
    assert e.value.code == capi.ERR_INVALID and text in str(e.value), str(e.value)


def same(ctx, b, job, d_dst):
    results, pes = ctx.ts_results(b, len(job.streams), job.n_pes)
    TC.assert_same(results, pes, ctx.download(d_dst, job.dst0.size).tobytes(), job)


def same_adts(ctx, b, job):
    results, frames = ctx.adts_results(b, len(job.streams), job.n_frames)
    TC.assert_same_adts(results, frames, job)


@pytest.mark.parametrize("variant", [0, 1], ids=["launches", "plain"])
def test_create_run_run_destroy(ctx, job, ajob, variant):
    d_src, d_dst, d_aac = ctx.upload(job.src), ctx.upload(job.dst0), ctx.upload(ajob.src)
    b = create(ctx, variant, lambda: ctx.ts_batch(job.descs, job.n_pes, job.src.size, job.dst0.size))
    a = create(ctx, variant, lambda: ctx.adts_batch(ajob.descs, ajob.n_frames, ajob.src.size))
    try:
        assert ctx.ts_paths(b)["route"] == ctx.adts_paths(a)["route"] == (2 if variant else 1)
        refused(lambda: ctx.ts_results(b, len(job.streams), job.n_pes), "the batch has not run")
        refused(lambda: ctx.ts_phase_ms(b), "the batch has not run")
        refused(lambda: ctx.adts_results(a, len(ajob.streams), ajob.n_frames), "the batch has not run")
        refused(lambda: ctx.adts_phase_ms(a), "the batch has not run")
        ctx.ts_run(b, d_src, d_dst)
        ctx.adts_run(a, d_aac)
        same(ctx, b, job, d_dst)
        same_adts(ctx, a, ajob)
        before = ctx.device_allocations()
        ctx.ts_run(b, d_src, d_dst)                    # a run behind a run, no results between
        ctx.ts_run(b, d_src, d_dst)
        ctx.adts_run(a, d_aac)
        ctx.adts_run(a, d_aac)
        same(ctx, b, job, d_dst)
        same(ctx, b, job, d_dst)                       # results twice
        same_adts(ctx, a, ajob)
        assert ctx.device_allocations() == before      # the second run allocated nothing on the device
        refused(lambda: ctx.ts_results(b, len(job.streams) + 1, job.n_pes), "the batch has %d streams" % len(job.streams))
        refused(lambda: ctx.ts_results(b, len(job.streams), job.n_pes - 1), "room for")
        refused(lambda: ctx.adts_results(a, len(ajob.streams), ajob.n_frames + 1), "room for")
        refused(lambda: ctx.ts_run(a, d_src, d_dst), "not a transport stream batch")
        refused(lambda: ctx.adts_run(b, d_src), "not an ADTS batch")
        refused(lambda: ctx.ts_results(a, 0, 0), "not a transport stream batch")
        refused(lambda: ctx.adts_results(b, 0, 0), "not an ADTS batch")
        refused(lambda: ctx.ogg_run(b, d_src, d_dst), "not a Ogg batch")
    finally:
        ctx.batch_destroy(b)
        ctx.batch_destroy(a)
        for p in (d_src, d_dst, d_aac):
            ctx.free(p)


@pytest.mark.parametrize("variant", [0, 1], ids=["launches", "plain"])
def test_a_run_on_a_second_stream_waits_for_the_run_on_the_first(ctx, job, ajob, variant):
    d_src, d_dst, d_aac = ctx.upload(job.src), ctx.upload(job.dst0), ctx.upload(ajob.src)
    s1, s2 = ctx.stream_create(), ctx.stream_create()
    b = create(ctx, variant, lambda: ctx.ts_batch(job.descs, job.n_pes, job.src.size, job.dst0.size))
    a = create(ctx, variant, lambda: ctx.adts_batch(ajob.descs, ajob.n_frames, ajob.src.size))
    try:
        for s in (s1, s2, s1, None, s2):
            ctx.ts_run(b, d_src, d_dst, s)
            ctx.adts_run(a, d_aac, s)
        same(ctx, b, job, d_dst)
        same_adts(ctx, a, ajob)
    finally:
        ctx.sync()
        ctx.batch_destroy(b)
        ctx.batch_destroy(a)
        ctx.stream_destroy(s1)
        ctx.stream_destroy(s2)
        for p in (d_src, d_dst, d_aac):
            ctx.free(p)


def test_create_and_destroy_cycles_live_off_the_block_cache(ctx, job, ajob):
    d_src, d_dst, d_aac = ctx.upload(job.src), ctx.upload(job.dst0), ctx.upload(ajob.src)
    try:
        counts = []
        for variant in (0, 1, 0, 1, 0, 1):
            b = create(ctx, variant, lambda: ctx.ts_batch(job.descs, job.n_pes, job.src.size, job.dst0.size))
            a = create(ctx, variant, lambda: ctx.adts_batch(ajob.descs, ajob.n_frames, ajob.src.size))
            ctx.ts_run(b, d_src, d_dst)
            ctx.adts_run(a, d_aac)
            same(ctx, b, job, d_dst)
            same_adts(ctx, a, ajob)
            ctx.batch_destroy(b)
            ctx.batch_destroy(a)
            counts.append(ctx.device_allocations())
        assert counts[1] == counts[-1], counts         # once both routes have run, nothing more is allocated
    finally:
        for p in (d_src, d_dst, d_aac):
            ctx.free(p)
