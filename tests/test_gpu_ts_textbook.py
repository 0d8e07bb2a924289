"""The transport stream demultiplexer and the ADTS frame table on the device (ohgpu_ts_*, ohgpu_adts_*, csrc/ts_packet_kernel.hip) against
the independent model (tests/ts_textbook.py), byte for byte: every result, every record a stream has room for, and the whole destination
arena, which is pre-filled with 0xA5 and has guard bytes round every run.  Every test names the route that served it.  The shapes are
the smallest at which a kernel can go wrong -- tests/ts_cases.py's named streams hold them: streams of 0 to 3 packets and round one
and two waves and one workgroup's tile (63..65, 255..257) and of five tiles; 187 and 188 + 187 bytes; every payload length 0..184 and
the corrupt 184; runs of 0- and 1-byte payloads; every table and PES rule once; all 256 pairs of source and destination phase; tables
of no room and of too little; an empty stream and an empty batch; a second run of one batch on other bytes; more tiles than one trip of
the capped gather launch covers; ADTS frames round every boundary of the map (a word, a wave, a workgroup's tile, the chain's 2048-bit
step); recognition at its edges; and the fused call."""
import numpy as np
import pytest

import ts_cases as TC
import ts_textbook as TX
from device_shape import MAX_WAVES_PER_CU, compute_units
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

WAVES, GROUPS_PER_CU, TILE_PIECES = 4, 8, 64          # kTsWaves, kTsGroupsPerCu, kTsTilePieces: ts_wave_blocks(tiles, cus) = min(ceil(tiles / 4), 8 * cus)
ROUTES = [pytest.param(0, id="launches"), pytest.param(1, id="plain")]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def tiles_of(job):
    """The gather's work list by the documented rule: per stream ceil((packets * 184 // 16 + 2) / 64) tiles, none for no packet."""
    return sum(-(-(int(d["src_bytes"]) // 188 * 184 // 16 + 2) // TILE_PIECES) for d in job.descs if int(d["src_bytes"]) >= 188)


def ts_batch(ctx, job, variant):
    ctx.set_kernel_variant(variant)
    try:
        b = ctx.ts_batch(job.descs, job.n_pes, job.src.size, job.dst0.size)
    finally:
        ctx.set_kernel_variant(0)
    paths = ctx.ts_paths(b)
    assert paths["route"] == (2 if variant else 1) and paths["tiles"] == tiles_of(job), paths
    if not variant:
        assert paths["wave_blocks"] == min(-(-paths["tiles"] // WAVES), GROUPS_PER_CU * compute_units())
    return b


def run(ctx, job, variant=0, runs=1):
    capi.ts_batch_check(job.descs, job.n_pes, job.src.size, job.dst0.size)
    d_src, d_dst = ctx.upload(job.src), ctx.upload(job.dst0)
    b = ts_batch(ctx, job, variant)
    try:
        for _ in range(runs):
            ctx.copy_h2d(d_dst, job.dst0)
            ctx.ts_run(b, d_src, d_dst)
            results, pes = ctx.ts_results(b, len(job.streams), job.n_pes)
            TC.assert_same(results, pes, ctx.download(d_dst, job.dst0.size).tobytes(), job)
        assert all(ms >= 0 for ms in ctx.ts_phase_ms(b))
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return results, pes


def adts_batch(ctx, job, variant):
    ctx.set_kernel_variant(variant)
    try:
        b = ctx.adts_batch(job.descs, job.n_frames, job.src.size)
    finally:
        ctx.set_kernel_variant(0)
    paths = ctx.adts_paths(b)
    assert paths["route"] == (2 if variant else 1), paths
    if not variant:
        assert paths["tiles"] == sum(-(-int(d["src_bytes"]) // 1024) for d in job.descs), paths
    return b


def run_adts(ctx, job, variant=0, runs=1):
    capi.adts_batch_check(job.descs, job.n_frames, job.src.size)
    d_src = ctx.upload(job.src)
    b = adts_batch(ctx, job, variant)
    try:
        for _ in range(runs):
            ctx.adts_run(b, d_src)
            results, frames = ctx.adts_results(b, len(job.streams), job.n_frames)
            TC.assert_same_adts(results, frames, job)
        assert all(ms >= 0 for ms in ctx.adts_phase_ms(b))
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
    return results, frames


# ---------------------------------------------------------------- layer 1
@pytest.mark.parametrize("variant", ROUTES)
def test_every_named_stream(ctx, variant):
    named = TC.named()
    job = TC.Job(list(named.values()))
    names = list(named)
    assert {m["status"] for m in job.models} == set(range(5))
    assert [job.models[names.index(f"packets_{n}")]["packets"] for n in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)] == [0, 1, 2, 3, 63, 64, 65, 255, 256, 257]
    corrupt = job.models[names.index("corrupt")]
    assert corrupt["status"] == TX.CORRUPT and len(corrupt["pes"]) == 2 and corrupt["packets"] > corrupt["corrupt_packet"] + 4
    tiny = job.models[names.index("tiny_payloads")]
    assert tiny["audio_packets"] > 40 and tiny["pes_open_bytes"] == TX.UNBOUNDED
    results, _ = run(ctx, job, variant)
    assert [int(r["pes_packets"]) for r in results[[names.index("no_room_for_records"), names.index("little_room_for_records")]]] == [4, 4]


@pytest.mark.parametrize("variant", ROUTES)
def test_a_stream_of_five_tiles_of_the_sums(ctx, variant):
    rng = TC.Lcg(55)
    job = TC.Job([TC.stream(TC.long_stream(rng, 1100 + 7)), TC.stream(TC.long_stream(rng, 513)), TC.stream(TC.long_stream(rng, 512)[188 * 2:], audio_pid=TC.AUDIO_PID,
                                                                                                        flags=TX.PES_OPEN, pes_open_bytes=100)])
    m = job.models[0]
    assert m["packets"] == 1107 and m["cc_jumps"] > 2 and m["bad_pes_starts"] > 2 and len(m["pes"]) > 150
    assert any(r["packet"] // 256 != (r["packet"] + 9) // 256 for r in m["pes"])          # PES packets that straddle a tile's end
    run(ctx, job, variant)


def test_every_source_phase_to_every_destination_phase(ctx):
    job = TC.phases_job()                                                                     # (asserts that all 256 pairs occur)
    d_src, d_dst = ctx.upload(job.src), ctx.upload(job.dst0)
    try:
        assert d_src.value % 16 == 0 and d_dst.value % 16 == 0                                # the offsets' phases are the addresses'
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
    run(ctx, job, 0)


def test_an_empty_stream_and_an_empty_batch(ctx):
    named = TC.named()
    for variant in (0, 1):
        run(ctx, TC.Job([named["packets_0"], named["ten_pes"], named["packets_0"], named["bytes_187"]]), variant)
        run(ctx, TC.Job([named["packets_0"]]), variant)
        b = ctx.ts_batch(np.zeros(0, dtype=capi.TS_STREAM_DESC), 0, 0, 0)
        try:
            ctx.ts_run(b, None, None)
            results, pes = ctx.ts_results(b, 0, 0)
            assert results.size == 0 and pes.size == 0
        finally:
            ctx.batch_destroy(b)


@pytest.mark.parametrize("variant", ROUTES)
def test_a_second_run_on_other_bytes_allocates_nothing(ctx, variant):
    rng = TC.Lcg(77)
    first = TC.long_stream(rng, 300)
    other = b"".join(TC.head_packets() + TC.audio_run(rng, n_pes=3)[0] + [TC.packet(TC.OTHER_PID, b"", adaptation=190)])
    other += rng.bytes(len(first) - len(other))
    jobs = [TC.Job([TC.stream(first)]), TC.Job([TC.stream(other)])]
    assert jobs[0].models[0]["status"] == TX.OK and jobs[1].models[0]["status"] == TX.CORRUPT
    assert jobs[0].src.size == jobs[1].src.size and jobs[0].n_pes >= jobs[1].n_pes
    jobs[1].n_pes = jobs[0].n_pes
    d_src, d_dst = ctx.malloc(jobs[0].src.size), ctx.malloc(jobs[0].dst0.size)
    b = ts_batch(ctx, jobs[0], variant)
    try:
        allocs = []
        for job in (jobs[0], jobs[1], jobs[0]):
            ctx.copy_h2d(d_src, job.src)
            ctx.copy_h2d(d_dst, job.dst0)
            ctx.sync()
            ctx.ts_run(b, d_src, d_dst)
            results, pes = ctx.ts_results(b, 1, job.n_pes)
            TC.assert_same(results, pes, ctx.download(d_dst, job.dst0.size).tobytes(), job)
            allocs.append(ctx.device_allocations())
        assert allocs[0] == allocs[1] == allocs[2]
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)


def test_the_host_buffer_call(ctx):
    named = TC.named()
    job = TC.Job([named["ten_pes"], named["counter_jumps"], named["before_first_start_open_less"]])
    dst = job.dst0.copy()
    results, pes = ctx.ts_process_host(job.descs, job.n_pes, job.src, dst)
    TC.assert_same(results, pes, dst.tobytes(), job)


def trips_need(cus):
    return 2 * max(GROUPS_PER_CU * WAVES, MAX_WAVES_PER_CU) * cus + 67


def test_more_tiles_than_one_trip_of_the_gather_launch(ctx):
    """The gather is persistent: a wave per tile of 64 destination pieces, the launch capped at 8 workgroups of 4 waves a CU, every wave
    going round the list in strides of the launch's waves.  More than 2 x that + 67 streams of one to three packets (a tile each):
    every wave makes two trips and the lowest-numbered ones a third."""
    cus = compute_units()
    rng = TC.Lcg(1000 + cus)
    pool = [rng.bytes(184) for _ in range(16)]
    kinds = []
    for k in range(48):                                                  # 48 distinct small streams, drawn from in a seeded order
        n = 1 + k % 3
        es = b"".join(pool[rng.below(16)] for _ in range(n))[:n * 184 - 9 - rng.below(100)]
        kinds.append(TC.stream(b"".join(TC.carry(TC.AUDIO_PID, TC.pes(es), cc=k)), audio_pid=TC.AUDIO_PID, pes_capacity=1))
    need = trips_need(cus)
    streams = [kinds[rng.below(48)] for _ in range(need + 1)]
    job = TC.Job(streams)
    assert tiles_of(job) == len(streams) > need == 2 * max(8 * 4, 32) * cus + 67
    assert min(-(-tiles_of(job) // WAVES), cus * GROUPS_PER_CU) == cus * GROUPS_PER_CU      # the launch IS capped
    assert all(m["status"] == TX.OK and len(m["run"]) > 60 for m in job.models)
    run(ctx, job, 0, runs=2)


# ---------------------------------------------------------------- layer 2
@pytest.mark.parametrize("variant", ROUTES)
def test_every_named_adts_stream(ctx, variant):
    named = TC.adts_named()
    for lead in (0, 1, 2, 3):                                            # the streams at other addresses mod 4
        job = TC.AdtsJob(list(named.values()), lead=lead)
        names = list(named)
        assert {m["status"] for m in job.models} == {TX.ADTS_OK, TX.NOT_ADTS}
        assert job.models[names.index("largest")]["frames"][0]["bytes"] == 8191 and job.models[names.index("recognise_at_1001")]["first_frame_offset"] == 1001
        results, _ = run_adts(ctx, job, variant)
        assert [int(r["frames"]) for r in results[[names.index("little_room"), names.index("no_room")]]] == [7, 7]


@pytest.mark.parametrize("variant", ROUTES)
def test_adts_an_empty_batch_and_a_second_run_on_other_bytes(ctx, variant):
    b = ctx.adts_batch(np.zeros(0, dtype=capi.ADTS_STREAM_DESC), 0, 0)
    try:
        ctx.adts_run(b, None)
        results, frames = ctx.adts_results(b, 0, 0)
        assert results.size == 0 and frames.size == 0
    finally:
        ctx.batch_destroy(b)
    named = TC.adts_named()
    a = named["plain"]["data"]
    other = named["junk_between"]["data"]
    other = other + TC.clean(TC.Lcg(4).bytes(len(a) - len(other)))
    jobs = [TC.AdtsJob([TC.adts_stream(a)]), TC.AdtsJob([TC.adts_stream(other)])]
    n_frames = max(j.n_frames for j in jobs)
    for j in jobs:
        j.n_frames = n_frames
        j.descs["frame_capacity"][0] = n_frames
    d_src = ctx.malloc(jobs[0].src.size)
    b = adts_batch(ctx, jobs[0], variant)
    try:
        allocs = []
        for job in (jobs[0], jobs[1], jobs[0]):
            ctx.copy_h2d(d_src, job.src)
            ctx.sync()
            ctx.adts_run(b, d_src)
            results, frames = ctx.adts_results(b, 1, n_frames)
            TC.assert_same_adts(results, frames, job)
            allocs.append(ctx.device_allocations())
        assert allocs[0] == allocs[1] == allocs[2]
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)


def test_adts_the_host_buffer_call(ctx):
    named = TC.adts_named()
    job = TC.AdtsJob([named["plain"], named["recognise_four_then_five"], named["junk_between"]])
    results, frames = ctx.adts_process_host(job.descs, job.n_frames, job.src)
    TC.assert_same_adts(results, frames, job)


# ---------------------------------------------------------------- both
def test_the_fused_call_on_a_ten_pes_stream(ctx):
    """Transport bytes in; the run, the PES table and the frame table out.  The frame table must be layer 2 alone on the model's run."""
    rng = TC.Lcg(10)
    packets, es = TC.segment(rng, 40, frames_per_pes=4)
    cut, _ = TC.segment(rng, 30, frames_per_pes=3)
    job = TC.Job([TC.stream(b"".join(packets)), TC.stream(b"".join(cut)[:-188 * 2])])
    assert [len(m["pes"]) for m in job.models] == [10, 10] and job.models[0]["run"] == es
    want = [TX.adts_chain(m["run"], TX.RECOGNISE) for m in job.models]
    assert [len(w["frames"]) for w in want] == [40, 29] and want[1]["bytes_consumed"] < len(job.models[1]["run"])
    adescs = np.zeros(2, dtype=capi.ADTS_STREAM_DESC)
    adescs["src_offset"], adescs["flags"] = job.descs["dst_offset"], capi.ADTS_RECOGNISE
    adescs["frame_first"], adescs["frame_capacity"] = [0, 45], [45, 45]
    dst = job.dst0.copy()
    tres, pes, ares, frames = ctx.ts_adts_process_host(job.descs, adescs, job.n_pes, 90, job.src, dst)
    TC.assert_same(tres, pes, dst.tobytes(), job)
    alone = TC.AdtsJob.__new__(TC.AdtsJob)
    alone.descs, alone.models = adescs, want
    TC.assert_same_adts(ares, frames, alone)
