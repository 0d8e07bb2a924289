"""Apple Lossless packets decoded on the device (ohgpu_alac_batch_create / _run / _results, csrc/alac_packet_kernel.hip) against the
plain-Python model (tests/alac_textbook.py), on both routes: the three fused phases over the transposed scratch and, for a batch
created under kernel variant 1, the plain one (a thread per packet, straight from the bytes) -- each first asserted through
ohgpu_batch_paths_info.

Conventions, as the other textbook tests: arenas allocated to the byte (the last packet ends where the source arena ends), the
destination pre-filled with a pattern and guard bytes around every plane, the WHOLE destination arena compared with the model's,
every packet's status and sample count and every stream's result compared too.  Malformed input here is the named handful of
tests/alac_cases.malformed; a fixed selection of the fixed-seed damage goes to the device in tests/test_gpu_alac_damage.py, and the
full set runs only on the CPU.  Every packet of either tests/test_alac_core_cpu.py has already taken through the sanitised CPU
build of the same core; nothing here is random."""
import numpy as np
import pytest

import alac_cases as AC
import alac_textbook as T
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["fused", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.alac_route = capi.ALAC_ROUTE_PLAIN if request.param else capi.ALAC_ROUTE_FUSED
    yield ctx
    ctx.set_kernel_variant(0)


def run(ctx, job, times=1):
    descs, packets = AC.capi_tables(job)
    src, dst0 = np.frombuffer(job.src, dtype=np.uint8), np.frombuffer(job.dst0, dtype=np.uint8)
    d_src, d_dst = ctx.upload(src), ctx.upload(dst0)
    b = ctx.alac_batch(descs, packets, src.size, dst0.size)
    allocs = []
    try:
        assert ctx.batch_paths(b)["alac_route"] == ctx.alac_route
        for _ in range(times):
            ctx.alac_run(b, d_src, d_dst)
            sres, pres = ctx.alac_results(b, len(descs), len(packets))
            allocs.append(ctx.device_allocations())
        got = ctx.download(d_dst, dst0.size)
        assert all(ms >= 0.0 for ms in ctx.alac_phase_ms(b))
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return sres, pres, got, allocs


def check(ctx, job, times=1):
    sres, pres, got, allocs = run(ctx, job, times)
    assert [(int(p["status"]), int(p["samples"])) for p in pres] == [tuple(w) for w in job.want_packets]
    assert [(int(s["packets_ok"]), int(s["samples"]), int(s["first_bad_status"])) for s in sres] == job.want_streams()
    bad = np.flatnonzero(got != np.frombuffer(job.want, dtype=np.uint8))
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[0]}"
    return allocs


@pytest.mark.parametrize("form", AC.FORMS, ids=["planes", "packed_le", "packed_be"])
def test_every_fixture_and_handmade_packet_in_one_batch(vctx, form):
    """frame lengths 64 / 256 / 1024 / 4096 and depths 16 / 24 / 32 mixed, mono beside stereo beside six channels, every stream's
    last packet a partial one"""
    job = AC.Job(AC.fixture_streams(form) + AC.handmade_streams(form))
    assert {s["cfg"]["frame_length"] for s in job.streams} >= {256, 1024, 4096} and {s["cfg"]["bit_depth"] for s in job.streams} == {16, 24, 32}
    assert all(st == T.OK for st, _ in job.want_packets)
    check(vctx, job)


def mono_packets(n):
    pool = [p for name in ("orders", "factors", "den_shifts", "zero_runs", "coef_wrap") for p in AC.handmade()[name][1]]
    return [pool[k % len(pool)] for k in range(n)]


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 129])
def test_group_edges_of_the_transposed_scratch(vctx, rows):
    cfg = T.parse_config(AC.handmade()["orders"][0])
    check(vctx, AC.Job([(cfg, mono_packets(rows), AC.FORMS[rows % 3])]))


def test_a_groups_rows_come_from_different_packets_and_streams(vctx):
    """a mono stream of three packets beside a stereo one: the pair's rows start at an odd row; 31 pairs later the next would straddle
    the group's edge and moves to the next group"""
    hand = AC.handmade()
    mono = T.parse_config(hand["orders"][0])
    stereo_cookie, stereo_packets = hand["mode_nonzero"]
    stereo = T.parse_config(stereo_cookie)
    pairs = [stereo_packets[0], hand["hand_stereo8"][1][0], hand["partial"][1][0]] * 11
    check(vctx, AC.Job([(mono, mono_packets(3), T.PLANAR), (stereo, pairs, T.PLANAR), (mono, mono_packets(2), T.PACKED_BE)]))


@pytest.mark.parametrize("form", [T.PLANAR, T.PACKED_LE], ids=["planes", "packed_le"])
def test_malformed_packets_between_good_neighbours(vctx, form):
    job = AC.Job(AC.sandwiches(form))
    want = [st for _, _, st in AC.malformed().values()]
    assert [job.want_packets[3 * i + 1][0] for i in range(len(want))] == want and {T.CORRUPT, T.UNSUPPORTED} <= set(want)
    check(vctx, job)                     # (the whole arena: the neighbours intact, the bad packet's share untouched)


def test_a_batch_of_64_streams_twice_without_allocating(vctx):
    pool = AC.fixture_streams(T.PLANAR) + AC.handmade_streams(T.PLANAR)
    streams = [(pool[k % len(pool)][0], pool[k % len(pool)][1], AC.FORMS[k % 3]) for k in range(64)]
    allocs = check(vctx, AC.Job(streams), times=2)
    assert allocs[1] == allocs[0], allocs


def test_process_host_writes_only_what_was_decoded(ctx):
    job = AC.Job(AC.sandwiches(T.PLANAR) + AC.fixture_streams(T.PACKED_LE)[:2])
    descs, packets = AC.capi_tables(job)
    dst = np.frombuffer(job.dst0, dtype=np.uint8).copy()
    sres, pres = ctx.alac_process_host(descs, packets, np.frombuffer(job.src, dtype=np.uint8), dst)
    assert np.array_equal(dst, np.frombuffer(job.want, dtype=np.uint8))
    assert [(int(p["status"]), int(p["samples"])) for p in pres] == [tuple(w) for w in job.want_packets]
    assert [(int(s["packets_ok"]), int(s["samples"]), int(s["first_bad_status"])) for s in sres] == job.want_streams()
