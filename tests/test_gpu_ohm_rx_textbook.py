"""The Songcast receiver on the device (ohgpu_ohm_rx_batch_create / _run / _results, csrc/ohm_rx_kernel.hip) against the model
(tests/ohm_rx_textbook.py: struct.unpack, a Python set, slicing; held to the oracle's parse and to invariants by
tests/test_ohm_rx_textbook.py).

Conventions, as the other textbook tests: the source arena allocated to the byte (the last datagram ends where it ends), the
destination pre-filled with 0xA5 with guard bytes around every run, the WHOLE destination arena compared with the model's, every
record and every stream result compared byte for byte.  The device sees only tables that ohgpu_ohm_rx_batch_check passed; odd tables
are tests/test_ohm_rx_core_cpu.py's, on the sanitised CPU build of the same core.  Everything is exact.  Nothing here is random:
payloads come from fixed-seed generators, the sessions from tests/golden/ohm_rx_textbook.json."""
import numpy as np
import pytest

import ohm_rx_cases as RC
import ohm_rx_textbook as RX
import ohm_textbook as OT
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def run(ctx, job, times=1):
    capi.ohm_rx_batch_check(job.d_streams, job.d_grams, len(job.src), len(job.dst0))
    src, dst0 = np.frombuffer(job.src, dtype=np.uint8), np.frombuffer(job.dst0, dtype=np.uint8)
    d_src, d_dst = ctx.upload(src), ctx.upload(dst0)
    b = ctx.ohm_rx_batch(job.d_streams, job.d_grams, src.size, dst0.size)
    allocs, arenas = [], []
    try:
        for _ in range(times):
            ctx.copy_h2d(d_dst, dst0)
            ctx.ohm_rx_run(b, d_src, d_dst)
            sres, recs = ctx.ohm_rx_results(b, len(job.streams), len(job.table))
            allocs.append(ctx.device_allocations())
            arenas.append(ctx.download(d_dst, dst0.size))
        ms = ctx.ohm_rx_phase_ms(b)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return sres, recs, arenas, allocs, ms


def check(ctx, job, times=1):
    sres, recs, arenas, allocs, ms = run(ctx, job, times)
    for arena in arenas:
        RC.assert_same(sres, recs, arena.tobytes(), job)
    return allocs, ms


@pytest.fixture(scope="module")
def sweep():
    return RC.sweep_job()


def test_every_audio_length_at_every_alignment(ctx, sweep):
    """audio lengths 0..5760 x codec lengths 0, 1, 2, 3, 29 x datagram offsets 0, 4, 8, 12 mod 16, five interleaved streams"""
    job = sweep
    codecs = [c for c in RC.SWEEP_CODEC for _ in range(80)]
    assert {(size - 58 - c, off % 16, c) for (off, size), c in zip(job.table, codecs)} == {(n, a, c) for n in RC.SWEEP_AUDIO for a in (0, 4, 8, 12) for c in RC.SWEEP_CODEC}
    assert {(off + 58 + c) % 4 for (off, _), c in zip(job.table, codecs)} == {0, 1, 2, 3}
    assert {int(r["dst_offset"]) % 16 for r in job.want_records if r["audio_bytes"]} == set(range(16))
    check(ctx, job)
    assert job.want != job.dst0 and max(o + s for o, s in job.table) == len(job.src)      # (the source arena ends with its last datagram)


def test_the_committed_sessions(ctx):
    sessions = RC.load_sessions()
    job = RC.Job([RC.session_stream(s) for s in sessions])
    for s, res in zip(sessions, job.results):                             # the model today is the model that was recorded
        assert (res["stop_reason"], res["resend"], res["n_pending"]) == (s["result"]["stop_reason"], s["result"]["resend"], s["result"]["n_pending"]), s["name"]
    assert {int(r["disposition"]) for r in job.want_records} == set(range(1, 8))
    assert {int(r["events"]) for r in job.want_records} >= {0, 1, 2, 3, 4}
    check(ctx, job)


def test_mixed_types_and_every_bad_status_in_one_stream(ctx):
    good = RC.audio_gram(3, bytes(range(40)), codec=b"abc")
    big = RC.audio_gram(4, bytes(range(256)) * 22 + bytes(128), codec=b"x" * 29)
    over = big[:6] + (len(big) + 1).to_bytes(2, "big") + big[8:] + b"\0"
    short = RC.audio_gram(5, b"", codec=b"abcdef")[:60]
    grams = [RC.audio_gram(2, b"\1\2"), good, b"", b"Ohm \1", over, good[:57] + bytes([30]) + good[58:], short[:6] + (60).to_bytes(2, "big") + short[8:],
             RC.other_gram(8), b"Ohm \2\3\0\10", good[:8] + b"\x31" + good[9:], good[:56] + b"\1" + good[57:], big] + \
            [RC.other_gram(k, bytes(k)) for k in (0, 1, 2, 4, 5, 6, 7, 255)] + [RC.audio_gram(7, b"\5"), RC.audio_gram(30, b"\6\7"), RC.audio_gram(204, b"\10")]
    job = RC.Job([RC.stream(grams), RC.stream([]), RC.stream([RC.other_gram(0)])])
    assert {int(r["status"]) for r in job.want_records} == {RX.OK, RX.NOT_OHM, RX.NOT_AUDIO, RX.TRUNCATED, RX.BAD_HEADER, RX.OVERSIZE}
    assert sorted(int(r["msg_type"]) for r in job.want_records if r["status"] == RX.NOT_AUDIO) == [0, 0, 1, 2, 4, 5, 6, 7, 255]
    assert job.results[0]["n_pending"] == 3 and len(job.results[0]["resend"]) == 20
    check(ctx, job)


def shuffled_stream(rng, first, n, depth=8, channels=1):
    frames = RC.window_shuffle([(first + k) & 0xffffffff for k in range(n)], rng)
    grams = []
    for f in frames:
        grams.append(RC.audio_gram(f, rng.bytes(channels * depth // 8 * (1 + rng.below(12))), depth=depth, channels=channels))
        if rng.below(10) == 0:
            grams.append(RC.audio_gram(f, rng.bytes(channels * depth // 8), flags=OT.FLAG_LOSSLESS | OT.FLAG_RESENT, depth=depth, channels=channels))
    return RC.stream(grams)


@pytest.mark.parametrize("n_streams", [1, 63, 64, 65, 257])
def test_many_streams_in_a_batch(ctx, n_streams):
    """the sequence phase's launch at 1, 63, 64, 65 and 257 lanes: shuffled streams at the wrap, a stream that stops, an empty one"""
    rng = RC.Lcg(70 + n_streams)
    streams = []
    for i in range(n_streams):
        if i % 9 == 7:
            streams.append(RC.stream([]))
        elif i % 9 == 8:
            streams.append(RC.stream([RC.audio_gram(f, bytes([i & 255, f]), flags=OT.FLAG_LOSSLESS | (OT.FLAG_HALT if f == 13 else 0)) for f in (10, 12, 13, 15, 11, 14)]))
        else:
            streams.append(shuffled_stream(rng, (0, 5, 0xffffff00, 0xfffffffe)[i % 4], 6 + rng.below(30)))
    check(ctx, RC.Job(streams))


def test_a_batch_run_twice_gives_the_same_arena_and_allocates_nothing(ctx, sweep):
    allocs, ms = check(ctx, sweep, times=2)
    assert allocs[1] == allocs[0], allocs
    again, _ = check(ctx, RC.Job([RC.session_stream(s) for s in RC.load_sessions()]), times=2)
    assert again[1] == again[0], again
    assert len(ms) == 3 and all(v >= 0.0 for v in ms), ms


def test_the_waiting_frames_replayed_in_front_of_the_next_batch(ctx):
    """a stream cut in two batches: the PENDING datagrams of the first, in `order`, in front of the second's arrivals, from
    state_out -- the two runs' output is the uncut batch's"""
    rng = RC.Lcg(81)
    whole = shuffled_stream(rng, 0xffffff80, 200)["grams"]
    whole.insert(1, RC.audio_gram((0xffffff80 + 700) & 0xffffffff, b"far!", depth=8, channels=1))   # begins a repair far ahead, and waits to the end
    _, res_whole, out_whole = RX.receive(RX.new_state(), whole)
    assert res_whole["n_pending"] == 1 and res_whole["stop_reason"] == 0 and res_whole["n_output"] == 200
    for cut in (1, 19, 23, 60, 151):
        first = RC.Job([RC.stream(whole[:cut])])
        sres, recs, arenas, _, _ = run(ctx, first)
        RC.assert_same(sres, recs, arenas[0].tobytes(), first)
        waiting = sorted((k for k in range(cut) if recs[k]["disposition"] == capi.OHM_RX_PENDING), key=lambda k: int(recs[k]["order"]))
        assert len(waiting) == int(sres[0]["n_pending"])
        state = {k: int(sres[0][k]) for k in capi.OHM_RX_STATE_FIELDS}
        second = RC.Job([RC.stream([whole[k] for k in waiting] + whole[cut:], state=state)])
        sres2, recs2, arenas2, _, _ = run(ctx, second)
        RC.assert_same(sres2, recs2, arenas2[0].tobytes(), second)
        got = bytes(arenas[0][RC.GUARD:RC.GUARD + int(sres[0]["out_bytes"])]) + bytes(arenas2[0][RC.GUARD:RC.GUARD + int(sres2[0]["out_bytes"])])
        assert got == out_whole, cut
        assert {k: int(sres2[0][k]) for k in capi.OHM_RX_STATE_FIELDS} == res_whole["state_out"]
        assert all(int(e) == 0 for e in recs2["events"][:len(waiting)])


def test_the_empty_batch(ctx):
    b = ctx.ohm_rx_batch(np.zeros(0, dtype=capi.OHM_RX_STREAM), np.zeros(0, dtype=capi.OHM_RX_DATAGRAM), 0, 0)
    try:
        ctx.ohm_rx_run(b, None, None)
        sres, recs = ctx.ohm_rx_results(b, 0, 0)
        assert sres.size == 0 and recs.size == 0
    finally:
        ctx.batch_destroy(b)


def test_a_misaligned_source_base_is_refused_before_anything_is_queued(ctx):
    import ctypes
    job = RC.Job([RC.session_stream(RC.load_sessions()[1])])
    src, dst0 = np.frombuffer(job.src, dtype=np.uint8), np.frombuffer(job.dst0, dtype=np.uint8)
    d_src, d_dst = ctx.upload(np.concatenate([np.zeros(4, dtype=np.uint8), src])), ctx.upload(np.concatenate([dst0, dst0[:3]]))
    b = ctx.ohm_rx_batch(job.d_streams, job.d_grams, src.size, dst0.size)
    at = lambda p, skew: ctypes.c_void_p(p.value + skew)
    try:
        for skew in (1, 2, 3):
            with pytest.raises(capi.OhGpuError) as e:
                ctx.ohm_rx_run(b, at(d_src, skew), d_dst)
            assert e.value.code == capi.ERR_INVALID
        assert np.array_equal(ctx.download(d_dst, dst0.size), dst0)                      # nothing ran
        ctx.ohm_rx_run(b, at(d_src, 4), at(d_dst, 3))                                    # the destination may lie at any address
        sres, recs = ctx.ohm_rx_results(b, 1, len(job.table))
        got = ctx.download(d_dst, dst0.size + 3)
        assert np.array_equal(got[3:], np.frombuffer(job.want, dtype=np.uint8)) and np.array_equal(got[:3], dst0[:3])
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)


def test_process_host_brings_back_what_was_gathered(ctx):
    job = RC.Job([RC.session_stream(s) for s in RC.load_sessions()[:6]])
    dst = np.frombuffer(job.dst0, dtype=np.uint8).copy()
    sres, recs = ctx.ohm_rx_process_host(job.d_streams, job.d_grams, np.frombuffer(job.src, dtype=np.uint8), dst)
    RC.assert_same(sres, recs, dst.tobytes(), job)
