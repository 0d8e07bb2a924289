"""The RAOP receiver batch's life on the device, the pins tests/test_gpu_demux_lifecycle.py and tests/test_gpu_stream_switch.py make for
the other families: results before a run, runs and results in any order, a run on a second HIP stream behind one on the first, the empty
batch, a batch of another kind, a misaligned base, and the context's block cache over create / destroy cycles.  Both routes."""
import ctypes

import numpy as np
import pytest

import raop_rx_cases as RC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def job():
    return RC.Job(RC.lossy_streams()[:5] + [RC.stream([])] + RC.shape_streams()[:6])


@pytest.fixture(params=[0, 1], ids=["wave", "plain"])
def make(request, ctx, job):
    made = []

    def create(j=job):
        ctx.set_kernel_variant(request.param)
        try:
            b = ctx.raop_rx_batch(j.d_streams, j.d_grams, len(j.src))
        finally:
            ctx.set_kernel_variant(0)
        made.append(b)
        return b

    yield create
    for b in made:
        ctx.batch_destroy(b)


def same(ctx, b, job):
    sres, recs = ctx.raop_rx_results(b, len(job.streams), len(job.table))
    RC.assert_same(sres, recs, ctx.raop_rx_packets(b, len(job.table)), job)


def refused(call, text):
    with pytest.raises(capi.OhGpuError) as e:
        call()
    assert e.value.code == capi.ERR_INVALID and text in str(e.value), str(e.value)


def test_results_need_a_run_and_runs_and_results_come_in_any_order(ctx, job, make):
    d_src = ctx.upload(np.frombuffer(job.src, dtype=np.uint8))
    try:
        b = make()
        refused(lambda: ctx.raop_rx_results(b, len(job.streams), len(job.table)), "the batch has not run")
        refused(lambda: ctx.raop_rx_packets(b, len(job.table)), "the batch has not run")
        refused(lambda: ctx.raop_rx_phase_ms(b), "the batch has not run")
        ctx.raop_rx_run(b, d_src)
        ctx.raop_rx_run(b, d_src)                      # a run behind a run, no results between
        same(ctx, b, job)
        same(ctx, b, job)                              # results twice
        refused(lambda: ctx.raop_rx_results(b, len(job.streams) + 1, len(job.table)), "the batch has %d streams" % len(job.streams))
        refused(lambda: ctx.raop_rx_packets(b, len(job.table) - 1), "room for")
        sres, recs = ctx.raop_rx_results(b, len(job.streams), 0)           # the stream results alone
        assert sres.tobytes() == job.want_results.tobytes() and recs.size == 0
        refused(lambda: ctx.raop_rx_run(b, ctypes.c_void_p(d_src.value + 2)), "4-byte aligned")
        other = make()                                 # two batches of one shape live side by side
        ctx.raop_rx_run(other, d_src)
        same(ctx, other, job)
        same(ctx, b, job)
    finally:
        ctx.free(d_src)


def test_a_run_on_a_second_stream_waits_for_the_run_on_the_first(ctx, job, make):
    d_src = ctx.upload(np.frombuffer(job.src, dtype=np.uint8))
    s1, s2 = ctx.stream_create(), ctx.stream_create()
    try:
        b = make()
        for s in (s1, s2, s1, None, s2):
            ctx.raop_rx_run(b, d_src, s)
        same(ctx, b, job)
    finally:
        ctx.sync()
        ctx.stream_destroy(s1)
        ctx.stream_destroy(s2)
        ctx.free(d_src)


def test_the_empty_batch_and_a_batch_of_streams_without_datagrams(ctx, make):
    none = RC.Job([])
    b = make(none)
    ctx.raop_rx_run(b, None)                           # nothing to launch, whatever the arena
    sres, recs = ctx.raop_rx_results(b, 0, 0)
    assert sres.size == 0 and recs.size == 0 and ctx.raop_rx_packets(b, 0).size == 0
    hollow = RC.Job([RC.stream([]), RC.stream([], RC.running_state(7))])
    b = make(hollow)
    ctx.raop_rx_run(b, None)                           # no source byte is touched: no arena needed
    same(ctx, b, hollow)
    assert hollow.want_results["frame"][1] == 7 and hollow.want_results["running"][1] == 1


def test_a_batch_of_another_kind_is_refused_both_ways(ctx, job, make):
    b = make()
    d_src = ctx.upload(np.frombuffer(job.src, dtype=np.uint8))
    ohm = ctx.ohm_rx_batch(np.zeros(0, dtype=capi.OHM_RX_STREAM), np.zeros(0, dtype=capi.OHM_RX_DATAGRAM), 0, 0)
    try:
        refused(lambda: ctx.raop_rx_run(ohm, d_src), "not a RAOP receiver batch")
        refused(lambda: ctx.raop_rx_results(ohm, 0, 0), "not a RAOP receiver batch")
        refused(lambda: ctx.raop_rx_packets(ohm, 0), "not a RAOP receiver batch")
        refused(lambda: ctx.ohm_rx_run(b, d_src, d_src), "not a Songcast receiver batch")
    finally:
        ctx.batch_destroy(ohm)
        ctx.free(d_src)


def test_create_and_destroy_cycles_live_off_the_block_cache(ctx, job):
    d_src = ctx.upload(np.frombuffer(job.src, dtype=np.uint8))
    try:
        counts = []
        for variant in (0, 1, 0, 1, 0, 1):
            ctx.set_kernel_variant(variant)
            try:
                b = ctx.raop_rx_batch(job.d_streams, job.d_grams, len(job.src))
            finally:
                ctx.set_kernel_variant(0)
            ctx.raop_rx_run(b, d_src)
            same(ctx, b, job)
            ctx.batch_destroy(b)
            counts.append(ctx.device_allocations())
        assert counts[1] == counts[-1], counts         # once both routes have run, nothing more is allocated
    finally:
        ctx.free(d_src)
