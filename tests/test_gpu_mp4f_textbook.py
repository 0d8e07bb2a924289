"""The fragmented MPEG-4 layer on the device (ohgpu_mp4f_*, csrc/mp4_frag_kernel.hip) against the independent model
(tests/mp4f_textbook.py), byte for byte and on both routes (the six phases, and the plain one a batch created under kernel variant 1
takes, each first asserted through ohgpu_mp4f_batch_paths): every result, the three whole tables -- pre-filled with 0xA5 by the batch,
with guard rows in front of, between and behind the streams' ranges -- and the whole destination arena, 0xA5 before the run and with
guard bytes round every stream's room.  Every named file, good and malformed, and the capacity cases in one batch; CUTS = 400 of the
cuts round box boundaries, every n-th of the whole set (the sanitised CPU build takes them all); the gather from source addresses 0..15
mod 16 to destination addresses 0..15 mod 16, from every kind of first row into every kind of room; 300 damaged files; a run table
longer than one trip of the two persistent launches (a wave a run slot, at most 8 workgroups a CU: restated below); an empty stream and
an empty batch; a second run, and a second batch of the same shape, that allocate nothing."""
import numpy as np
import pytest

import mp4f_cases as FC
import mp4f_textbook as FX
from device_shape import compute_units
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

TILE = 1024          # mp4frag::kTile (csrc/mp4_frag_core.h): the samples one workgroup of the expansion takes
CUTS = 400           # the cuts a route runs


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["phases", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.mp4f_route = capi.MP4F_ROUTE_PLAIN if request.param else capi.MP4F_ROUTE_PHASES
    yield ctx
    ctx.set_kernel_variant(0)


def run(ctx, job, runs=2):
    capi.mp4f_batch_check(job.descs, job.n_packets, job.n_runs, job.src.size, job.dst_bytes)
    d_src, d_dst = ctx.upload(job.src), ctx.malloc(max(job.dst_bytes, 4))
    b = ctx.mp4f_batch(job.descs, job.n_packets, job.n_runs, job.src.size, job.dst_bytes)
    try:
        paths = ctx.mp4f_paths(b)
        assert paths["route"] == ctx.mp4f_route
        allocs = []
        for _ in range(runs):
            ctx.memset(d_dst, FC.FILL, max(job.dst_bytes, 4))
            ctx.mp4f_run(b, d_src, d_dst)
            results, run_rows, packets, samples = ctx.mp4f_results(b, len(job.streams), job.n_packets, job.n_runs)
            dst = ctx.download(d_dst, max(job.dst_bytes, 4))[:job.dst_bytes]
            FC.assert_same(results, run_rows, packets, samples, dst, job)
            allocs.append(ctx.device_allocations())
        assert len(set(allocs)) == 1                                   # a second run allocates nothing on the device
        ms = ctx.mp4f_phase_ms(b)
        assert all(v >= 0 for v in ms) and (ctx.mp4f_route == capi.MP4F_ROUTE_PHASES or ms[1:] == (0.0,) * 5)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return results, paths


def test_every_named_file_and_every_capacity(vctx):
    good, bad, caps = FC.named_good(), FC.named_malformed(), FC.named_capacities()
    streams = [FC.stream(m, gather_first_row=k % 3) for k, m in enumerate(good.values())] + [FC.stream(data, codecs=codecs) for data, _, _, codecs in bad.values()]
    streams += [FC.stream(m, capacity=pc, run_capacity=rc) for m, rc, pc in caps.values()] + [FC.stream(m) for m, _ in FC.limit_edges().values()]
    job = FC.Job(streams)
    for m, model in zip(good.values(), job.models):
        FC.check_against_record(model, m)
    assert [(model["samples_available"], model["samples_refused"]) for model in job.models[-4:]] == [(2, 1)] * 4        # the limit's edge
    results, _ = run(vctx, job)
    assert {int(r["status"]) for r in results} == set(range(7))
    assert [(int(r["status"]), int(r["error_offset"])) for r in results[len(good):len(good) + len(bad)]] == [(status, at) for _, status, at, _ in bad.values()]


def test_four_hundred_cuts_round_box_boundaries(vctx):
    streams = []
    for m in FC.named_good().values():
        streams += [FC.stream(data, capacity=m.n, run_capacity=len(m.runs), dst_capacity=len(m.data)) for data in FC.cuts(m)]
    streams = streams[::len(streams) // CUTS][:CUTS]
    assert len(streams) == CUTS >= 300
    job = FC.Job(streams)
    assert {FX.OK, FX.TRUNCATED} <= {m["status"] for m in job.models} and any(m["samples_refused"] and m["bytes_gathered"] for m in job.models)
    run(vctx, job, runs=1)


def test_the_gather_between_every_pair_of_addresses(vctx):
    m = FC.mux(FC.init_segment(), [FC.fragment([FC.run(FC.pattern_samples(9, k), [10] * 9), FC.run(FC.pattern_samples(3, k + 5, 70), [10] * 3, data_offset=False)], sequence=k)
                                   for k in (1, 2)])
    job = FC.Job([FC.stream(m, gather_first_row=(i * 7) % 11) for i in range(256)], align=lambda i: i % 16, dst_align=lambda i: i // 16)
    pairs = {(int(d["src_offset"]) % 16, int(d["dst_offset"]) % 16) for d in job.descs}
    assert pairs == {(a, b) for a in range(16) for b in range(16)}           # (the device arenas are 256-byte aligned)
    assert all(model["bytes_gathered"] for model in job.models)
    run(vctx, job, runs=1)


def test_gathers_from_every_row_into_every_room(vctx):
    m = FC.named_good()["two_truns_without_data_offset"]
    total = sum(m.sizes)
    streams = [FC.stream(m, gather_first_row=row, dst_capacity=total) for row in (0, 1, 4, 5, 6, 70, 71, 73, 74, 75, 147, 148, 200)]
    streams += [FC.stream(m, dst_capacity=total - 1), FC.stream(m, dst_capacity=0), FC.stream(m, gather=False), FC.stream(m, capacity=72), FC.stream(m, run_capacity=2)]
    big = FC.named_good()["run_of_2049"]
    streams += [FC.stream(big, gather_first_row=row) for row in (0, TILE - 1, TILE, 2048)] + [FC.stream(big, capacity=TILE + 1)]
    job = FC.Job(streams)
    assert [model["bytes_gathered"] for model in job.models[12:16]] == [0, 0, 0, 0] and job.models[0]["bytes_gathered"] == total
    run(vctx, job)


def test_three_hundred_damaged_files_in_one_batch(vctx):
    job = FC.Job([FC.stream(data, capacity=2100, run_capacity=8) for data in FC.damaged(300)])
    statuses = [m["status"] for m in job.models]
    assert statuses.count(FX.OK) >= 75 and sum(1 for s in statuses if s != FX.OK) >= 75
    run(vctx, job, runs=1)


def test_a_run_table_longer_than_one_trip_of_the_persistent_launches(vctx):
    many = FC.mux(FC.init_segment(), [FC.fragment([FC.run(FC.pattern_samples(2, k), [3, 4]), FC.run(FC.pattern_samples(1, k + 1), [5], data_offset=False)], sequence=k)
                                      for k in range(1, 41)])
    small = FC.named_good()["size_only"]
    cus = compute_units()
    waves_a_trip = 8 * cus * 4                                               # kMp4fGroupsPerCu workgroups a CU, four waves each: a wave a run slot
    job = FC.Job([FC.stream(small, run_capacity=waves_a_trip + 5), FC.stream(many), FC.stream(small)])
    assert int(job.descs[1]["run_first"]) > waves_a_trip and len(many.runs) == 80
    results, paths = run(vctx, job, runs=1)
    assert vctx.mp4f_route == capi.MP4F_ROUTE_PLAIN or paths["wave_blocks"] * 4 < job.n_runs


def test_an_empty_stream_and_an_empty_batch(vctx):
    good = FC.named_good()["tfdt_absent"]
    run(vctx, FC.Job([FC.stream(b""), FC.stream(good), FC.stream(b"", capacity=0, run_capacity=0), FC.stream(FC.named_good()["init_segment_alone"], capacity=4, run_capacity=2)]))
    run(vctx, FC.Job([FC.stream(b"", gather=False)]))
    b = vctx.mp4f_batch(np.zeros(0, dtype=capi.MP4F_STREAM_DESC), 0, 0, 0, 0)
    try:
        vctx.mp4f_run(b, None, None)
        results, run_rows, packets, samples = vctx.mp4f_results(b, 0, 0, 0)
        assert results.size == 0 and run_rows.size == 0 and packets.size == 0 and samples.size == 0
    finally:
        vctx.batch_destroy(b)


def test_a_second_batch_of_the_same_shape_allocates_nothing(vctx):
    job = FC.Job([FC.stream(FC.named_good()["run_of_1025"]), FC.stream(FC.named_good()["alac_patterns"])])
    run(vctx, job)
    before = vctx.device_allocations()
    again = vctx.mp4f_batch(job.descs, job.n_packets, job.n_runs, job.src.size, job.dst_bytes)
    try:
        assert vctx.device_allocations() == before
    finally:
        vctx.batch_destroy(again)


def test_the_host_buffer_call(vctx):
    good = FC.named_good()
    job = FC.Job([FC.stream(good["negative_data_offset"]), FC.stream(FC.named_malformed()["no_dfla"][0]), FC.stream(good["two_truns_with_data_offset"], capacity=6, gather_first_row=2)])
    dst = np.full(job.dst_bytes, FC.FILL, dtype=np.uint8)
    results, run_rows, packets, samples = vctx.mp4f_process_host(job.descs, job.n_packets, job.n_runs, job.src, dst)
    FC.assert_same(results, run_rows, packets, samples, dst, job)
