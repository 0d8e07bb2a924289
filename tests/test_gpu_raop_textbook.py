"""RAOP audio on the device (ohgpu_raop_batch_create / _run / _results, csrc/raop_decrypt_kernel.hip in front of
csrc/alac_packet_kernel.hip) against the model chain: tests/raop_textbook.py (a plain FIPS-197 InvCipher, held to libcrypto by
tests/test_raop_textbook.py), then tests/alac_textbook.py.

Conventions, as the other textbook tests: the source arena allocated to the byte (the last packet ends where it ends), the destination
pre-filled with 0xA5 and guard bytes around every block, the WHOLE destination arena compared with the model's, every packet's status
and sample count and every stream's result compared too.  The device sees only tables that ohgpu_raop_batch_check passed; odd tables
are tests/test_raop_core_cpu.py's, on the sanitised CPU build of the same core.  Nothing here is random: keys, IVs and payloads come
from a fixed-seed generator, the sessions from tests/golden/raop_textbook.json."""
import ctypes

import numpy as np
import pytest

import alac_cases as AC
import alac_textbook as T
import raop_cases as RC
import raop_textbook as R
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

# piece edges at 1, 2, 63, 64, 65, 128 and 129 blocks; tail-only packets; exact multiples; nothing at all
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 1008, 1023, 1024, 1025, 1028, 1040, 1460, 2048, 2064)
FORMS = (T.PLANAR, T.PACKED_LE, T.PACKED_BE)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["fused", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.variant_now = request.param
    ctx.alac_route = capi.ALAC_ROUTE_PLAIN if request.param else capi.ALAC_ROUTE_FUSED
    yield ctx
    ctx.set_kernel_variant(0)
    ctx.variant_now = 0


@pytest.fixture
def fctx(ctx):
    """the context with the fused route selected for this test, whatever vctx has selected for its module-scoped turn"""
    before = getattr(ctx, "variant_now", 0)
    ctx.set_kernel_variant(0)
    yield ctx
    ctx.set_kernel_variant(before)


def run(ctx, job, times=1, route=capi.ALAC_ROUTE_FUSED):
    descs, packets = RC.capi_tables(job)
    src, dst0 = np.frombuffer(job.src, dtype=np.uint8), np.frombuffer(job.dst0, dtype=np.uint8)
    d_src, d_dst = ctx.upload(src), ctx.upload(dst0)
    b = ctx.raop_batch(descs, packets, src.size, dst0.size)
    allocs = []
    try:
        assert ctx.batch_paths(b)["alac_route"] == route
        for _ in range(times):
            ctx.raop_run(b, d_src, d_dst)
            sres, pres = ctx.raop_results(b, len(descs), len(packets))
            allocs.append(ctx.device_allocations())
        got = ctx.download(d_dst, dst0.size)
        ms = ctx.raop_phase_ms(b)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return sres, pres, got, allocs, ms


def check(ctx, job, times=1, route=capi.ALAC_ROUTE_FUSED):
    sres, pres, got, allocs, ms = run(ctx, job, times, route)
    assert [(int(p["status"]), int(p["samples"])) for p in pres] == [tuple(w) for w in job.want_packets]
    assert [(int(s["packets_ok"]), int(s["samples"]), int(s["first_bad_status"])) for s in sres] == job.want_streams()
    bad = np.flatnonzero(got != np.frombuffer(job.want, dtype=np.uint8))
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[0]}"
    return allocs, ms


@pytest.fixture(scope="module")
def plaintext_job():
    """five streams under five keys, every length in each of them, interleaved in the arena; packet k of stream i lies at source offset
    4 * ((k + i) % 4) mod 16, so every length meets every source alignment"""
    rng = AC.Lcg(51)
    return RC.Job([RC.stream(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), [RC.rand_bytes(rng, n) for n in LENGTHS],
                             align=[4 * ((k + i) % 4) for k in range(len(LENGTHS))]) for i in range(5)])


def test_the_decryptor_alone_at_every_piece_edge_and_alignment(fctx, plaintext_job):
    ctx = fctx
    job = plaintext_job
    assert {(size, off % 16) for off, size in job.table} == {(n, a) for n in LENGTHS for a in (0, 4, 8, 12)}
    assert len({s["key"] for s in job.streams}) == 5
    check(ctx, job)
    assert job.want != job.dst0


def decode_job(form, key_of=lambda i, s: None):
    return RC.Job([RC.session_stream(s, form, key_of(i, s)) for i, s in enumerate(RC.sessions())])


@pytest.fixture(scope="module")
def decode_jobs():
    return {form: decode_job(form) for form in FORMS}


@pytest.mark.parametrize("form", FORMS, ids=["planes", "packed_le", "packed_be"])
def test_every_session_decodes_to_the_pcm_it_was_encoded_from(vctx, decode_jobs, form):
    job = decode_jobs[form]
    assert all(st == T.OK for st, _ in job.want_packets)
    check(vctx, job, route=vctx.alac_route)
    if form != T.PLANAR:                                   # losslessness through the cipher: the model's arena holds the fixtures' PCM
        for s in job.streams:
            fx = next(x["fx"] for x in RC.sessions() if x["payloads"] == s["payloads"])
            size = fx["meta"]["bits"] // 8
            pcm = fx["pcm"] if form == T.PACKED_LE else b"".join(fx["pcm"][i:i + size][::-1] for i in range(0, len(fx["pcm"]), size))
            assert job.want[s["dst_offset"]:s["dst_offset"] + len(pcm)] == pcm


def test_a_wrong_key_between_two_good_streams(vctx):
    """the middle stream's key has one bit flipped: its packets end in whatever the model chain makes of those bytes, the neighbours'
    share of the arena is exact (the whole arena is compared)"""
    a, b, c = RC.sessions()[0], RC.sessions()[1], RC.sessions()[2]
    wrong = bytes([b["key"][0] ^ 0x10]) + b["key"][1:]
    job = RC.Job([RC.session_stream(a, T.PACKED_LE), RC.session_stream(b, T.PACKED_LE, wrong), RC.session_stream(c, T.PLANAR)])
    mid = job.streams[1]
    theirs = job.want_packets[mid["first_packet"]:mid["first_packet"] + mid["n_packets"]]
    assert R.decrypt_packet(wrong, b["iv"], b["payloads"][0])[:16] != b["fx"]["packets"][0][:16]
    assert [w for k, w in enumerate(job.want_packets) if not mid["first_packet"] <= k < mid["first_packet"] + mid["n_packets"]] == \
        [w for s in (a, c) for w in RC.Job([RC.session_stream(s, T.PACKED_LE)]).want_packets]
    assert theirs != RC.Job([RC.session_stream(b, T.PACKED_LE)]).want_packets
    check(vctx, job, route=vctx.alac_route)


def test_every_wrong_key_stream(vctx):
    """the nine streams of tests/raop_cases.wrong_key_streams -- which tests/test_raop_core_cpu.py has taken through the sanitised
    Apple Lossless core as decrypted bytes -- each between two good sessions, in every output form: the wrong streams' packets end
    as the model chain says, some of them CORRUPT, and the good sessions' share of the arena is exact"""
    good = RC.sessions()
    wrong = RC.wrong_key_streams(lambda k: FORMS[k % 3])
    assert len(wrong) == 9
    streams = [RC.session_stream(good[0], T.PLANAR)]
    for k, w in enumerate(wrong):
        streams += [w, RC.session_stream(good[(k + 1) % 4], FORMS[(k + 1) % 3])]
    job = RC.Job(streams)
    theirs = [st for s in job.streams[1::2] for st, _ in job.want_packets[s["first_packet"]:s["first_packet"] + s["n_packets"]]]
    ours = [st for s in job.streams[0::2] for st, _ in job.want_packets[s["first_packet"]:s["first_packet"] + s["n_packets"]]]
    assert T.CORRUPT in theirs and all(st == T.OK for st in ours)
    check(vctx, job, route=vctx.alac_route)


def test_plaintext_and_decoding_streams_in_one_batch(vctx):
    rng = AC.Lcg(52)
    s = RC.sessions()
    streams = [RC.session_stream(s[0], T.PLANAR), RC.stream(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), [RC.rand_bytes(rng, n) for n in (1028, 0, 7, 48)]),
               RC.session_stream(s[3], T.PACKED_BE), RC.session_stream(s[1], RC.PLAINTEXT), RC.session_stream(s[2], T.PACKED_LE)]
    job = RC.Job(streams)
    check(vctx, job, route=vctx.alac_route)
    clear = job.streams[3]                                  # a caller with its own decoder: the fixture's packets, in the clear, where the layout says
    for (off, size), p in zip(job.table[clear["first_packet"]:], s[1]["fx"]["packets"]):
        at = clear["dst_offset"] + off - job.table[clear["first_packet"]][0]
        assert job.want[at:at + size] == p


def test_64_streams_twice_and_a_second_batch_without_allocating(fctx):
    ctx = fctx
    s = RC.sessions()
    streams = lambda: [RC.session_stream(s[k % 4], (T.PLANAR, T.PACKED_LE, T.PACKED_BE, RC.PLAINTEXT)[(k // 4) % 4]) for k in range(64)]
    first = RC.Job(streams())
    allocs, _ = check(ctx, first, times=2)
    assert allocs[1] == allocs[0], allocs
    again, _ = check(ctx, RC.Job(streams()), times=1)
    assert again[0] == allocs[1], (allocs, again)


def test_phase_times(fctx, decode_jobs):
    ctx = fctx
    _, ms = check(ctx, decode_jobs[T.PACKED_BE])
    assert len(ms) == 4 and all(v >= 0.0 for v in ms), ms


def test_misaligned_bases_are_refused_before_anything_is_queued(fctx, plaintext_job):
    ctx = fctx
    job = plaintext_job
    descs, packets = RC.capi_tables(job)
    dst0 = np.frombuffer(job.dst0, dtype=np.uint8)
    d_src, d_dst = ctx.upload(np.concatenate([np.zeros(4, dtype=np.uint8), np.frombuffer(job.src, dtype=np.uint8)])), ctx.upload(np.concatenate([dst0, dst0[:4]]))
    b = ctx.raop_batch(descs, packets, len(job.src), dst0.size)
    at = lambda p, skew: ctypes.c_void_p(p.value + skew)
    try:
        for src_skew, dst_skew in ((1, 0), (2, 0), (0, 2), (3, 3)):
            with pytest.raises(capi.OhGpuError) as e:
                ctx.raop_run(b, at(d_src, src_skew), at(d_dst, dst_skew))
            assert e.value.code == capi.ERR_INVALID
        assert np.array_equal(ctx.download(d_dst, dst0.size), dst0)                      # nothing ran
        ctx.raop_run(b, at(d_src, 4), at(d_dst, 4))                                            # a multiple of 4 is enough
        ctx.raop_results(b, len(descs), len(packets))
        assert np.array_equal(ctx.download(d_dst, dst0.size + 4)[4:], np.frombuffer(job.want, dtype=np.uint8))
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)


def test_process_host_brings_back_what_was_written(fctx):
    ctx = fctx
    rng = AC.Lcg(53)
    s = RC.sessions()
    job = RC.Job([RC.session_stream(s[0], T.PACKED_LE), RC.stream(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), [RC.rand_bytes(rng, n) for n in (100, 16, 0, 3)]),
                  RC.session_stream(s[3], T.PLANAR)])
    descs, packets = RC.capi_tables(job)
    dst = np.frombuffer(job.dst0, dtype=np.uint8).copy()
    sres, pres = ctx.raop_process_host(descs, packets, np.frombuffer(job.src, dtype=np.uint8), dst)
    assert np.array_equal(dst, np.frombuffer(job.want, dtype=np.uint8))
    assert [(int(p["status"]), int(p["samples"])) for p in pres] == [tuple(w) for w in job.want_packets]
    assert [(int(x["packets_ok"]), int(x["samples"]), int(x["first_bad_status"])) for x in sres] == job.want_streams()
