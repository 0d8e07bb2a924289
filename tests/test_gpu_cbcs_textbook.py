"""The second protected MPEG-4 family on the device (ohgpu_cbcs_*, csrc/cbcs_kernel.hip) against the independent model
(tests/cbcs_textbook.py), byte for byte and on both routes (the phases, and the plain one a batch created under kernel variant 1 takes,
each first asserted through ohgpu_cbcs_batch_paths): every result, the three whole tables -- pre-filled with 0xA5 by the batch, with guard
rows round the streams' ranges -- and the whole destination arena, 0xA5 before the run and with guard bytes round every stream's room.
The jobs are tests/cbcs_jobs.py's, each asserted from its models to reach what it is for before it runs, and each has passed
tests/test_cbcs_core_cpu.py's sanitised driver first:

  named        every named good and malformed file (tests/cbcs_cases.py): both schemes, tenc versions 0 and 1, per-sample IVs of 8 and
               16 bytes and constant IVs of 8 and 16, patterns 0:0, 1:0, 1:9, 1:1, 5:5 and 15:15 over parts of crypt - 1 to
               2 (crypt + skip) + 1 blocks, entry counts 0, 1, 2, 3 and 17, entries with clear 0 or protected 0, a `cenc` sample whose
               parts enter the keystream at offsets 0, 5, 16, 32 and 33 under a low half that wraps, a traf without senc under a constant
               IV, senc before and behind the truns, two truns under one senc; every malformed file's status and error_offset
  alignments   protected parts of 0 to 33 bytes and of 63 to 129 blocks at four source by four destination alignments
  capacities   gather_first_row in mid-traf, subsample_capacity one short, prefixes of a stream cut inside a senc
  tiles        1025, 2049 and 3077 samples with entries; a tile with no work between two that have some
  mixed        `cbcs`, `cenc` with and without entries, clear, NO_KEY and malformed streams under five keys, run twice, and a second
               batch of the same shape that allocates nothing
  many trips   five times as many chunk slots as the capped launch has waves, for this device's CU count
  damage       150 files of fixed-seed damage"""
import numpy as np
import pytest

import cbcs_cases as BC
import cbcs_jobs as BJ
from device_shape import compute_units
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["phases", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.cbcs_route = capi.MP4F_ROUTE_PLAIN if request.param else capi.MP4F_ROUTE_PHASES
    yield ctx
    ctx.set_kernel_variant(0)


def run(ctx, job, runs=2, slots=None):
    capi.cbcs_batch_check(job.descs, job.n_packets, job.n_runs, job.n_subsamples, job.src.size, job.dst_bytes)
    d_src, d_dst = ctx.upload(job.src), ctx.malloc(max(job.dst_bytes, 4))
    b = ctx.cbcs_batch(job.descs, job.n_packets, job.n_runs, job.n_subsamples, job.src.size, job.dst_bytes)
    try:
        paths = ctx.cbcs_paths(b)
        assert paths["route"] == ctx.cbcs_route
        # the persistent decrypt-gather launch, restated (tests/cbcs_jobs.py has the constants): a wave per chunk slot of 64 work units,
        # four waves a workgroup, at most 8 workgroups a CU
        chunks = sum(BJ.slots_of(d) for d in job.descs)
        assert paths["wave_blocks"] == (0 if ctx.cbcs_route == capi.MP4F_ROUTE_PLAIN else min((chunks + 3) // 4, 8 * compute_units()))
        assert slots is None or (chunks == slots and (ctx.cbcs_route == capi.MP4F_ROUTE_PLAIN or paths["wave_blocks"] * 4 * BJ.TRIPS <= slots))
        allocs = []
        for _ in range(runs):
            ctx.memset(d_dst, BC.FILL, max(job.dst_bytes, 4))
            ctx.cbcs_run(b, d_src, d_dst)
            results, run_rows, packets, samples = ctx.cbcs_results(b, len(job.streams), job.n_packets, job.n_runs)
            dst = ctx.download(d_dst, max(job.dst_bytes, 4))[:job.dst_bytes]
            BC.assert_same(results, run_rows, packets, samples, dst, job)
            allocs.append(ctx.device_allocations())
        assert len(set(allocs)) == 1                                   # a second run allocates nothing on the device
        ms = ctx.cbcs_phase_ms(b)
        assert all(v >= 0 for v in ms) and (ctx.cbcs_route == capi.MP4F_ROUTE_PHASES or ms[1:] == (0.0,) * 5)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return results


def test_every_named_file(vctx):
    job = BJ.named_job()
    BJ.assert_named(job, run(vctx, job))


def test_every_part_size_at_four_by_four_alignments(vctx):
    job = BJ.alignment_job()
    BJ.assert_alignments(job)
    run(vctx, job, runs=1)


def test_capacities_prefixes_and_seek_rows(vctx):
    job = BJ.capacity_job()
    BJ.assert_capacities(job)
    run(vctx, job)


def test_streams_of_more_than_one_tile(vctx):
    job = BJ.tile_job()
    BJ.assert_tiles(job)
    run(vctx, job, runs=1)


def test_the_interleaved_batch_twice_and_a_second_batch_that_allocates_nothing(vctx):
    job = BJ.mixed_job()
    BJ.assert_mixed(job)
    run(vctx, job, runs=2)
    before = vctx.device_allocations()
    again = vctx.cbcs_batch(job.descs, job.n_packets, job.n_runs, job.n_subsamples, job.src.size, job.dst_bytes)
    try:
        assert vctx.device_allocations() == before
    finally:
        vctx.batch_destroy(again)


def test_an_empty_batch_and_the_host_buffer_call(vctx):
    b = vctx.cbcs_batch(np.zeros(0, dtype=capi.CBCS_STREAM_DESC), 0, 0, 0, 0, 0)
    try:
        vctx.cbcs_run(b, None, None)
        assert all(t.size == 0 for t in vctx.cbcs_results(b, 0, 0, 0))
    finally:
        vctx.batch_destroy(b)
    good = BC.named_good()
    job = BC.Job([BC.stream(b""), BC.stream(good["cbcs_edge_parts"]), BC.stream(good["cenc_counts_0_1_2_3_17"], gather_first_row=2), BC.stream(b"", capacity=0, run_capacity=0, sub_capacity=0)])
    dst = np.full(job.dst_bytes, BC.FILL, dtype=np.uint8)
    results, run_rows, packets, samples = vctx.cbcs_process_host(job.descs, job.n_packets, job.n_runs, job.n_subsamples, job.src, dst)
    BC.assert_same(results, run_rows, packets, samples, dst, job)


def test_fixed_seed_damage(vctx):
    job = BJ.damage_job()
    BJ.assert_damage(job)
    run(vctx, job, runs=1)


def test_more_chunk_slots_than_the_launch_has_waves(vctx):
    """W = 8 x 4 x CUs waves and 5 W slots and more: every wave makes five trips, each into another stream's schedule, and over the
    slots behind a stream's last unit.  The plain route makes no trips: it is here because both routes must write the same bytes."""
    cus = compute_units()
    job, slots = BJ.many_trip_job(cus)
    BJ.assert_trips(cus, job, slots)
    run(vctx, job, runs=1, slots=slots)
