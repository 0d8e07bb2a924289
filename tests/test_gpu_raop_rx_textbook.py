"""The RAOP receiver on the device (ohgpu_raop_rx_batch_create / _run / _results / _packets, csrc/raop_rx_kernel.hip) against the model
(tests/raop_rx_textbook.py: struct.unpack, a first frame and a Python list, the reference's `if` chains; held to the hand-written golden
file by tests/test_raop_rx_textbook.py).

Every record, every stream result and every packet row is compared byte for byte, on both routes -- the wave route (a wave per stream,
the waiting frames in its lanes) and the plain one (ohgpu_set_kernel_variant(1): a lane per stream runs the serial text) -- and the two
routes' answers with each other.  The source arena is allocated to the byte.  The device sees only tables that
ohgpu_raop_rx_batch_check passed; odd tables are tests/test_raop_rx_core_cpu.py's.  Nothing here is random: the sessions come from
tests/golden/raop_rx_textbook.json and fixed-seed generators (tests/raop_rx_cases.py), whose coverage tests/test_raop_rx_textbook.py
asserts on the model alone.  A trip of the wave route's fast path is 64 datagrams."""
import numpy as np
import pytest

import raop_rx_cases as RC
import raop_rx_textbook as RX
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu
ROUTES = {"wave": 0, "plain": 1}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def run(ctx, job, variant, times=1):
    capi.raop_rx_batch_check(job.d_streams, job.d_grams, len(job.src))
    d_src = ctx.upload(np.frombuffer(job.src, dtype=np.uint8))
    ctx.set_kernel_variant(variant)
    allocs = [ctx.device_allocations()]                                   # [before the batch, after each run]
    try:
        b = ctx.raop_rx_batch(job.d_streams, job.d_grams, len(job.src))
    finally:
        ctx.set_kernel_variant(0)
    got = []
    try:
        assert ctx.batch_paths(b)["raop_rx_route"] == (2 if variant else 1)
        for _ in range(times):
            ctx.raop_rx_run(b, d_src)
            sres, recs = ctx.raop_rx_results(b, len(job.streams), len(job.table))
            got.append((sres, recs, ctx.raop_rx_packets(b, len(job.table))))
            allocs.append(ctx.device_allocations())
        ms = ctx.raop_rx_phase_ms(b)
        assert len(ms) == 3 and all(v >= 0 for v in ms)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
    return got, allocs


def check(ctx, job, times=1):
    """both routes against the model, and against each other"""
    answers = {}
    for route, variant in ROUTES.items():
        got, allocs = run(ctx, job, variant, times)
        for sres, recs, rows in got:
            RC.assert_same(sres, recs, rows, job)
        answers[route] = got[-1], allocs
    (a, _), (b, _) = answers["wave"], answers["plain"]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    return answers


def test_the_committed_sessions_and_datagrams(ctx):
    gold = RC.load_golden()
    sessions = [RC.stream(RC.golden_grams(s), s["state_in"], s["max_frames"]) for s in gold["sessions"]]
    grams = RC.stream([(bytes.fromhex(g["hex"]), g["port"]) for g in gold["datagrams"]])
    job = RC.Job(sessions + [grams])
    assert {int(r["status"]) for r in job.want_records} == {RX.OK, RX.TRUNCATED, RX.OVERSIZE, RX.OTHER_TYPE}
    assert {int(r["disposition"]) for r in job.want_records} >= {RX.OUTPUT, RX.DROPPED_BY_RESET, RX.FLUSHED, RX.WRONG_SESSION, RX.SYNC, RX.IGNORED, RX.NOT_REACHED}
    assert {int(r["events"]) for r in job.want_records} == {0, 1, 2, 3}
    check(ctx, job)
    assert max(o + s for o, s, _ in job.table) == len(job.src)           # (the source arena ends with its last datagram)


def test_the_reference_suite_batch_by_batch(ctx):
    """every batch of the nineteen cases as the caller hands it over: the pending datagrams in front, state_out as state_in"""
    streams, want_ranges = [], []
    for case in RC.load_golden()["resend_suite"]:
        state = RX.new_state()
        batches = RC.suite_batches(case)
        for (_, what), (todo, _, res) in zip(batches, RC.play(batches, case["max_frames"])):
            streams.append(RC.stream(todo, state, case["max_frames"]))
            want_ranges.append(what[1] if what[0] == "timer" else None)
            state = RX.drop_audio(res["state_out"]) if what[0] == "drop" else res["state_out"]
    job = RC.Job(streams)
    for want, res in zip(want_ranges, job.results):                       # what the reference's tests expect at each timer, once more
        assert want is None or [list(r) for r in res["ranges"]] == want
    check(ctx, job)


def test_the_seeded_lossy_sessions(ctx):
    job = RC.Job(RC.lossy_streams())
    assert {int(r["stop_reason"]) for r in job.want_results} == {0, 1, 2} and any(r["n_pending"] for r in job.want_results)
    check(ctx, job)


def test_the_shapes_at_which_a_wave_can_go_wrong(ctx):
    """in-order runs of 1, 63, 64, 65, 128, 129; the 65535 -> 0 wrap at lanes 0, 31, 63 and the first of the second trip; a sync packet, a
    foreign ssrc and a truncated datagram at lanes 0, 1, 63 of both trips; max_frames 1, 5, 50, 63 filled to full and to full + 1 at the
    first, a middle and the last place; drains of 1, 2 and max_frames + 1; a drain that ends at a trip boundary; duplicates of the first,
    the last and a middle waiting frame; a late non-resend in and outside a repair; start, resume, the flush window, the delay rule"""
    job = RC.Job(RC.shape_streams())
    by_frames = {}
    for s, res in zip(job.streams, job.results):
        by_frames.setdefault(s["max_frames"], set()).add((res["stop_reason"], res["n_pending"]))
    for m in (1, 5, 50, 63):
        assert (RX.STOP_BUFFER_FULL, 0) in by_frames[m] and (RX.STOP_NONE, m + 1) in by_frames[m], m
    assert any(res["n_output"] == 129 for res in job.results)
    check(ctx, job)


def test_every_length_at_every_alignment(ctx):
    job = RC.Job(RC.sweep_streams())
    assert {(size, off % 16) for off, size, _ in job.table} == {(n, a) for n in RC.SWEEP_LENGTHS for a in (0, 4, 8, 12)}
    check(ctx, job)


def test_64_streams_of_mixed_shapes_with_empty_ones_between(ctx):
    job = RC.Job(RC.mixed_streams(64))
    assert sum(1 for s in job.streams if not s["grams"]) >= 10 and len(job.table) > 3000
    check(ctx, job)


def test_a_second_run_and_a_second_batch_allocate_nothing(ctx):
    job = RC.Job(RC.mixed_streams(16))
    check(ctx, job)                                                        # (the context's block cache has seen the shape)
    for route, (_, allocs) in check(ctx, job, times=2).items():
        assert allocs[0] == allocs[1] == allocs[2], (route, allocs)        # neither the second batch of the shape nor either of its runs
