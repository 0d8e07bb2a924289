"""The protected MPEG-4 layer on the device (ohgpu_cenc_*, csrc/cenc_kernel.hip) against the independent model (tests/cenc_textbook.py),
byte for byte and on both routes (the phases, and the plain one a batch created under kernel variant 1 takes, each first asserted through
ohgpu_cenc_batch_paths): every result, the three whole tables -- pre-filled with 0xA5 by the batch, with guard rows round the streams'
ranges -- and the whole destination arena, 0xA5 before the run and with guard bytes round every stream's room.  Samples of 0, 1, 15, 16,
17 and 33 bytes; samples of 63, 64, 65, 128 and 129 keystream blocks; four source and four destination alignments; IVs of 8 and 16
bytes; the low half's wrap inside a three-block sample; senc in front of and behind the truns, two truns under one senc; a
gather_first_row in the middle of a traf; a prefix of a stream; capacities below the counts; five keys interleaved with a clear stream
and a NO_KEY stream between good ones; a 64-stream batch run twice and a second batch that allocates nothing; the host-buffer call.

Streams of more than one tile (tests/cenc_cases.py's multi_tile_jobs: 255, 256, 257, 1023, 1024, 1025, 2049 and 3077 samples): rows
with blocks in every wave of a tile behind the first, so that cenc_rows_kernel's prefix across the waves and a tile's s0 count;
three tiles and more with blocks, and a tile without any between two that hold some, for cenc_tiles_kernel's loop and the tile
search's tie; runs that end and begin inside tiles 1 and 2 and two truns under one senc across row 1024, for the IV's place; samples
of 63 and 65 blocks behind row 1024; nothing at rows 1023 and 1024; clear streams of three tiles; gather_first_row at 255, 256, 1023,
1024, 1025 and 2048; rows cut at TILE + 1; rooms that end inside tile 1, at its first byte, and of no bytes.  And a work list of five
times as many chunk slots as the capped decrypt-gather launch has waves (many_trip_job, for this device's CU count): every wave goes
round its loop again and again, into another stream's key schedule, from a protected stream into a clear one and back, and over the
slots behind a stream's last block.  Each such job asserts from its models that it reaches these places before it runs, and has
passed tests/test_cenc_core_cpu.py's sanitised driver first (the work list in its one-CU build).  So has the damage job
(tests/cenc_cases.damage_job): a cut at every byte of the protection boxes and 300 files of fixed-seed damage, 608 streams that end
in every status beside one another."""
import numpy as np
import pytest

import cenc_cases as CC
import cenc_textbook as CX
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
    ctx.cenc_route = capi.MP4F_ROUTE_PLAIN if request.param else capi.MP4F_ROUTE_PHASES
    yield ctx
    ctx.set_kernel_variant(0)


@pytest.fixture(scope="module")
def good():
    return CC.named_good()


def run(ctx, job, runs=2, slots=None):
    capi.cenc_batch_check(job.descs, job.n_packets, job.n_runs, job.src.size, job.dst_bytes)
    d_src, d_dst = ctx.upload(job.src), ctx.malloc(max(job.dst_bytes, 4))
    b = ctx.cenc_batch(job.descs, job.n_packets, job.n_runs, job.src.size, job.dst_bytes)
    try:
        paths = ctx.cenc_paths(b)
        assert paths["route"] == ctx.cenc_route
        # the persistent decrypt-gather launch, restated: a wave per chunk slot of 64 keystream blocks, a stream has room for
        # dst_capacity / 16 + packet_capacity blocks, four waves a workgroup, at most 8 workgroups a CU.  (The other constants, as
        # tests/cenc_cases.py restates them: TILE = 1024 samples a workgroup of the rows launch, 256 threads of four samples,
        # SLOT_BLOCKS = 64, CRYPT_WAVES = 4 and CRYPT_GROUPS_PER_CU = 8.)
        chunks = sum((int(d["dst_capacity"]) // 16 + int(d["packet_capacity"]) + 63) // 64 for d in job.descs if d["dst_capacity"] and d["packet_capacity"])
        assert paths["wave_blocks"] == (0 if ctx.cenc_route == capi.MP4F_ROUTE_PLAIN else min((chunks + 3) // 4, 8 * compute_units()))
        assert slots is None or (chunks == slots and (ctx.cenc_route == capi.MP4F_ROUTE_PLAIN or paths["wave_blocks"] * 4 < slots))    # the launch is capped: its waves go round
        allocs = []
        for _ in range(runs):
            ctx.memset(d_dst, CC.FILL, max(job.dst_bytes, 4))
            ctx.cenc_run(b, d_src, d_dst)
            results, run_rows, packets, samples = ctx.cenc_results(b, len(job.streams), job.n_packets, job.n_runs)
            dst = ctx.download(d_dst, max(job.dst_bytes, 4))[:job.dst_bytes]
            CC.assert_same(results, run_rows, packets, samples, dst, job)
            allocs.append(ctx.device_allocations())
        assert len(set(allocs)) == 1                                   # a second run allocates nothing on the device
        ms = ctx.cenc_phase_ms(b)
        assert all(v >= 0 for v in ms) and (ctx.cenc_route == capi.MP4F_ROUTE_PHASES or ms[1:] == (0.0,) * 5)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return results


def test_every_named_file(vctx, good):
    bad = CC.named_malformed()
    streams = [CC.stream(m, gather_first_row=k % 3) for k, m in enumerate(good.values())]
    streams += [CC.stream(data, codecs=codecs, have_key=have_key, kid=kid) for data, _, _, codecs, have_key, kid in bad.values()]
    job = CC.Job(streams)
    results = run(vctx, job)
    assert [(int(r["mp4f"]["status"]), int(r["mp4f"]["error_offset"])) for r in results[len(good):]] == [(status, at) for _, status, at, _, _, _ in bad.values()]
    assert {int(r["iv_size"]) for r in results} == {0, 8, 16} and sum(1 for r in results if int(r["blocks"])) >= 12


def test_sample_sizes_and_piece_edges_at_four_by_four_alignments(vctx, good):
    files = [good["sizes_0_1_15_16_17_33"], good["piece_edges"]]
    job = CC.Job([CC.stream(files[i % 2]) for i in range(32)], align=lambda i: (0, 1, 7, 14)[i // 2 % 4], dst_align=lambda i: (0, 3, 8, 15)[i // 8])
    assert {(int(d["src_offset"]) % 16, int(d["dst_offset"]) % 16) for d in job.descs} == {(a, b) for a in (0, 1, 7, 14) for b in (0, 3, 8, 15)}
    assert all(m["samples_available"] == len(f.sizes) for m, f in zip(job.models, files * 16))
    run(vctx, job, runs=1)


def test_the_wrap_both_iv_sizes_and_senc_on_either_side(vctx, good):
    wrap, two = good["wrap_inside_three_blocks"], good["two_truns_under_one_senc_behind"]
    streams = [CC.stream(wrap), CC.stream(good["flac_iv8"]), CC.stream(good["alac_iv16"]), CC.stream(good["senc_in_front_of_the_truns"]), CC.stream(good["senc_behind_the_truns"]),
               CC.stream(good["two_truns_under_one_senc_front"])]
    streams += [CC.stream(two, gather_first_row=row) for row in (3, 5, 40, 71, 100, 141, 142)]        # (a traf holds rows 0..70: 5 and 66 samples)
    streams += [CC.stream(two, capacity=40, run_capacity=2), CC.stream(two, capacity=100, run_capacity=3, gather_first_row=72), CC.stream(two, dst_capacity=sum(two.sizes) - 1),
                CC.stream(two, dst_capacity=0), CC.stream(two, capacity=0, run_capacity=0)]
    streams += [CC.stream(two.data[:cut], capacity=two.n, run_capacity=len(two.runs), key=two.key, kid=two.kid) for cut in (two.segment_ends[0] + 30, two.segment_ends[0] - 9)]
    job = CC.Job(streams)
    assert job.models[0]["gathered"][:48] == wrap.clear[0] and job.models[0]["blocks"] == 3 + 1 + 3
    assert job.models[-1]["samples_refused"] and job.models[-1]["bytes_gathered"] and job.models[8]["clear_rows"][40] == (0, two.sizes[40])
    run(vctx, job)


def test_five_keys_a_clear_stream_and_a_stream_without_its_key(vctx, good):
    files = [CC.simple([7, 5], seed=20 + k, key=CC.key_of(k), kid=CC.kid_of(k), iv_size=(8, 16)[k % 2]) for k in range(5)]
    streams = []
    for k, m in enumerate(files):
        streams += [CC.stream(m), CC.stream(good["clear_plain_flac"]) if k % 2 else CC.stream(files[(k + 1) % 5], have_key=False)]
    streams.append(CC.stream(files[0], key=CC.key_of(3)))                                             # a wrong key under the right kid: other bytes, no refusal
    job = CC.Job(streams)
    assert [m["status"] for m in job.models] == [CX.OK, CX.NO_KEY, CX.OK, CX.OK, CX.OK, CX.NO_KEY, CX.OK, CX.OK, CX.OK, CX.NO_KEY, CX.OK]
    assert job.models[-1]["gathered"] != job.models[0]["gathered"] and job.models[-1]["bytes_gathered"] == job.models[0]["bytes_gathered"]
    results = run(vctx, job)
    no_key = results[1]
    assert bytes(no_key["kid"]) == CC.kid_of(1) and int(no_key["iv_size"]) == 16 and int(no_key["mp4f"]["codec"]) == CX.code(b"fLaC") and int(no_key["mp4f"]["samples"]) == 0


def test_sixty_four_streams_twice_and_a_second_batch_that_allocates_nothing(vctx, good):
    names = ["flac_iv8", "alac_iv16", "clear_plain_alac", "senc_behind_the_truns", "sizes_0_1_15_16_17_33", "enca_not_protected", "second_senc_skipped", "saiz_and_saio_skipped"]
    job = CC.Job([CC.stream(good[names[i % 8]], gather_first_row=i // 8 % 3) for i in range(64)])
    run(vctx, job, runs=2)
    before = vctx.device_allocations()
    again = vctx.cenc_batch(job.descs, job.n_packets, job.n_runs, job.src.size, job.dst_bytes)
    try:
        assert vctx.device_allocations() == before
    finally:
        vctx.batch_destroy(again)


def test_an_empty_stream_an_empty_batch_and_the_host_buffer_call(vctx, good):
    run(vctx, CC.Job([CC.stream(b""), CC.stream(good["flac_iv16"]), CC.stream(b"", capacity=0, run_capacity=0), CC.stream(good["init_segment_alone"], capacity=4, run_capacity=2)]))
    b = vctx.cenc_batch(np.zeros(0, dtype=capi.CENC_STREAM_DESC), 0, 0, 0, 0)
    try:
        vctx.cenc_run(b, None, None)
        assert all(t.size == 0 for t in vctx.cenc_results(b, 0, 0, 0))
    finally:
        vctx.batch_destroy(b)
    job = CC.Job([CC.stream(good["alac_iv8"]), CC.stream(CC.named_malformed()["senc_subsamples"][0]), CC.stream(good["two_truns_under_one_senc_front"], capacity=60, gather_first_row=2)])
    dst = np.full(job.dst_bytes, CC.FILL, dtype=np.uint8)
    results, run_rows, packets, samples = vctx.cenc_process_host(job.descs, job.n_packets, job.n_runs, job.src, dst)
    CC.assert_same(results, run_rows, packets, samples, dst, job)


def test_the_damage_and_the_protection_cuts(vctx):
    """tests/cenc_cases.damage_job: 308 cuts in the protection boxes and 300 damaged files in one batch, so that the persistent
    decrypt-gather launch goes over the chunk slots of streams that ended INVALID, TRUNCATED, UNSUPPORTED or NO_KEY part-way through,
    beside streams that gather.  The job has passed tests/test_cenc_core_cpu.py's sanitised driver, in both builds, first."""
    job = CC.damage_job()
    assert len(job.streams) == 608
    statuses = [model["status"] for model in job.models]
    assert statuses.count(CX.OK) >= 100 and sum(1 for s in statuses if s not in (CX.OK, CX.TRUNCATED)) >= 50 and CX.TRUNCATED in statuses
    run(vctx, job, runs=1)


@pytest.mark.parametrize("name", ["every_count", "descriptors"])
def test_streams_of_more_than_one_tile(vctx, name):
    job = CC.multi_tile_jobs()[name]
    CC.assert_reaches(name, job)
    run(vctx, job, runs=1)


def test_more_chunk_slots_than_the_launch_has_waves(vctx):
    """W = max(8 x 4, 32 resident) x CUs waves; 5 W + 67 slots and more, so every wave makes five trips and some a sixth.  The plain
    route makes no trips: it is here because both routes must write the same bytes and tables for this job too."""
    cus = compute_units()
    job, slots, per_slot = CC.many_trip_job(cus)
    CC.assert_trips(cus, job, slots, per_slot)
    run(vctx, job, runs=2, slots=slots)
