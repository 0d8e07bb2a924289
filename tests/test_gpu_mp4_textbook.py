"""The MPEG-4 container layer on the device (ohgpu_mp4_*, csrc/mp4_table_kernel.hip) against the independent model
(tests/mp4_textbook.py), byte for byte and on both routes (the four phases, and the plain one a batch created under kernel variant 1
takes, each first asserted through ohgpu_batch_paths_info): every result, and both whole tables -- pre-filled with 0xA5 by the batch,
with guard rows in front of, between and behind the streams' ranges.  The shapes are the smallest at which a kernel can go wrong:
sample counts round a wave and round a tile; chunkings whose chunks are everything, one sample, seven samples with a short last one,
different at every chunk, and astride every tile edge; the file at every address mod 16 with its tables at every address mod 4; offsets
and sizes that wrap in 32 bits; both forms of a box size; every status between good neighbours; 300 damaged files; a table of no room
and of one row too few; an empty stream and an empty batch; a second run of one batch on other bytes.  No launch is persistent -- a
workgroup a tile, a wave or a lane a stream -- so there is no trip rule to restate."""
import numpy as np
import pytest

import mp4_cases as MC
import mp4_textbook as MX
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

TILE = 1024          # kMp4Tile (csrc/ohgpu_internal.h, = mp4box::kTile of csrc/mp4_box_core.h): the samples one workgroup of the sums and of the expansion takes


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["fused", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.mp4_route = capi.MP4_ROUTE_PLAIN if request.param else capi.MP4_ROUTE_FUSED
    yield ctx
    ctx.set_kernel_variant(0)


def run(ctx, job, runs=1):
    capi.mp4_batch_check(job.descs, job.n_packets, job.src.size)
    d_src = ctx.upload(job.src)
    b = ctx.mp4_batch(job.descs, job.n_packets, job.src.size)
    try:
        assert ctx.batch_paths(b)["mp4_route"] == ctx.mp4_route
        for _ in range(runs):
            ctx.mp4_run(b, d_src)
            results, packets, samples = ctx.mp4_results(b, len(job.streams), job.n_packets)
            MC.assert_same(results, packets, samples, job)
        ms = ctx.mp4_phase_ms(b)
        assert all(v >= 0 for v in ms) and (ctx.mp4_route == capi.MP4_ROUTE_FUSED or ms[1:] == (0.0, 0.0, 0.0))
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
    return results, packets, samples


def test_sample_counts_round_a_wave_and_a_tile_in_every_chunking(vctx):
    streams = []
    for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        packets = MC.pattern_packets(n, seed=n)
        assert all(1 <= len(p) <= 90 for p in packets)
        frames = [1 + (k * 5) % 7 for k in range(n)]
        # everything in one chunk; one sample a chunk; seven with a short last chunk; another count at every chunk (E = C); chunks
        # astride every tile edge, so that a sample's place in its chunk reaches back into the tile in front
        for per_chunk in ([1 << 20], [1], [7], [3, 5, 2, 9, 4], [TILE - 3, 700, TILE + 5]):
            m = MC.mux(packets, MC.PATTERN_COOKIE, per_chunk=per_chunk, frames=frames, entry_per_chunk=len(per_chunk) > 1, co64=n % 2 == 1, gap=n % 4)
            MC.check_against_record(MX.demux(m.data, n), m)
            if per_chunk[0] == TILE - 3 and n > TILE:
                assert m.chunk_of[TILE - 1] == m.chunk_of[TILE] and (n <= 2 * TILE or m.chunk_of[2 * TILE - 1] == m.chunk_of[2 * TILE])
            if per_chunk == [7] and n % 7:
                assert m.chunk_of.count(m.chunks - 1) == n % 7
            streams.append(MC.stream(m))
    job = MC.Job(streams)
    assert all(m["status"] == MX.OK and m["samples_refused"] == 0 for m in job.models)
    run(vctx, job)


def test_the_file_at_every_address_and_the_tables_at_every_address(vctx):
    packets = MC.pattern_packets(70, seed=3)
    files = [MC.mux(packets, MC.PATTERN_COOKIE, per_chunk=[5, 9], free_before_stbl=k, co64=k % 2 == 1) for k in range(4)]
    job = MC.Job([MC.stream(files[i // 16]) for i in range(64)], align=lambda i: i % 16)
    seen = set()
    for i, d in enumerate(job.descs):
        m = files[i // 16]
        for name in ("stsz", "stsc", "stts"):
            assert (m.find(name)[1] - files[0].find(name)[1]) % 4 == (i // 16) % 4
        seen.add((int(d["src_offset"]) % 16, (int(d["src_offset"]) + m.find("stsz")[1]) % 4))
    assert seen == {(a, b) for a in range(16) for b in range(4)}             # (the device arena is 256-byte aligned)
    assert all(m["status"] == MX.OK and len(m["rows"]) == 70 for m in job.models)
    run(vctx, job)


def test_sums_that_would_wrap_in_32_bits(vctx):
    m = MC.mux(MC.pattern_packets(2 * TILE + 9, seed=5), MC.PATTERN_COOKIE, per_chunk=[TILE + 3], co64=True)
    co, stsz = m.find("co64"), m.find("stsz")
    far = MC.patched(m, co[1] + 8 + 8, (1 << 32) + m.offsets[TILE + 3], 8)       # the second chunk at 2^32 + a valid offset: refused, not aliased
    huge = MC.patched(m, stsz[1] + 12 + 4 * 5, 0xffffffff)                       # the sixth sample: every later one of its chunk is refused
    good = MC.named_good()
    job = MC.Job([MC.stream(far, capacity=m.n), MC.stream(huge, capacity=m.n), MC.stream(good["box_size_64"]), MC.stream(good["size_0_last"]),
                  MC.stream(good["size_0_last_moov"])])
    a, b = job.models[0], job.models[1]
    assert a["status"] == MX.OK and [r is None for r in a["rows"]] == [TILE + 3 <= s < 2 * TILE + 6 for s in range(m.n)]
    assert b["status"] == MX.OK and [r is None for r in b["rows"]] == [5 <= s < TILE + 3 for s in range(m.n)] and b["samples_available"] == 5
    for model, name in zip(job.models[2:], ("box_size_64", "size_0_last", "size_0_last_moov")):
        MC.check_against_record(model, good[name])
    run(vctx, job)


def test_every_status_between_good_neighbours(vctx):
    good = MC.named_good()["changing"]
    bad = MC.named_malformed()
    streams = []
    for data, _, _ in bad.values():
        streams += [MC.stream(good), MC.stream(data), MC.stream(good)]
    job = MC.Job(streams)
    assert [m["status"] for m in job.models[1::3]] == [status for _, status, _ in bad.values()]
    assert {m["status"] for m in job.models} == set(range(6)) and all(m["status"] == MX.OK for m in job.models[0::3] + job.models[2::3])
    run(vctx, job)


def test_three_hundred_damaged_files_in_one_batch(vctx):
    job = MC.Job([MC.stream(data) for data in MC.damaged(300)])
    statuses = [m["status"] for m in job.models]
    assert statuses.count(MX.OK) > 50 and statuses.count(MX.INVALID) > 50
    run(vctx, job)


def test_tables_of_no_room_and_of_one_row_too_few(vctx):
    m = MC.mux(MC.pattern_packets(TILE + 7, seed=8), MC.PATTERN_COOKIE, per_chunk=[11])
    job = MC.Job([MC.stream(m, capacity=0), MC.stream(m, capacity=m.n - 1), MC.stream(m)])
    results, _, _ = run(vctx, job)
    assert [int(r["samples"]) for r in results] == [m.n] * 3 and [int(r["samples_available"]) for r in results] == [0, m.n - 1, m.n]


def test_an_empty_stream_and_an_empty_batch(vctx):
    good = MC.named_good()["co64"]
    run(vctx, MC.Job([MC.stream(b""), MC.stream(good), MC.stream(b"", capacity=0), MC.stream(MC.named_good()["no_samples"], capacity=4)]))
    run(vctx, MC.Job([MC.stream(b"")]))
    b = vctx.mp4_batch(np.zeros(0, dtype=capi.MP4_STREAM_DESC), 0, 0)
    try:
        vctx.mp4_run(b, None)
        results, packets, samples = vctx.mp4_results(b, 0, 0)
        assert results.size == 0 and packets.size == 0 and samples.size == 0
    finally:
        vctx.batch_destroy(b)


def test_a_second_run_on_other_bytes_allocates_nothing(vctx):
    first = MC.mux(MC.pattern_packets(TILE + 40, seed=11), MC.PATTERN_COOKIE, per_chunk=[9])
    data = bytearray(first.data)
    stsz = first.find("stsz")
    data[stsz[1] + 12 + 4 * 30:stsz[1] + 12 + 4 * 31] = (1 << 20).to_bytes(4, "big")      # other bytes of the same length: a sample above the packet limit
    jobs = [MC.Job([MC.stream(first)]), MC.Job([MC.stream(bytes(data), capacity=first.n)])]
    assert jobs[1].models[0]["samples_refused"] > 0 and jobs[1].models[0]["first_bad_sample"] == 30
    d_src = vctx.malloc(jobs[0].src.size)
    b = vctx.mp4_batch(jobs[0].descs, jobs[0].n_packets, jobs[0].src.size)
    try:
        allocs = []
        for job in (jobs[0], jobs[1], jobs[0]):
            vctx.copy_h2d(d_src, job.src)
            vctx.sync()
            vctx.mp4_run(b, d_src)
            results, packets, samples = vctx.mp4_results(b, 1, job.n_packets)
            MC.assert_same(results, packets, samples, job)
            allocs.append(vctx.device_allocations())
        assert allocs[0] == allocs[1] == allocs[2]
    finally:
        vctx.batch_destroy(b)
        vctx.free(d_src)
    again = vctx.mp4_batch(jobs[0].descs, jobs[0].n_packets, jobs[0].src.size)             # a second batch of the same shape
    try:
        assert vctx.device_allocations() == allocs[0]
    finally:
        vctx.batch_destroy(again)


def test_the_host_buffer_call(vctx):
    good = MC.named_good()
    job = MC.Job([MC.stream(good["moov_last"]), MC.stream(MC.named_malformed()["mp4a_only"][0]), MC.stream(good["entry_per_chunk"], capacity=6)])
    results, packets, samples = vctx.mp4_process_host(job.descs, job.n_packets, job.src)
    # (the call's batch is its own: rows that no run wrote come home as the batch made them, 0xA5)
    MC.assert_same(results, packets, samples, job)
