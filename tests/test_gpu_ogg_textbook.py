"""The Ogg page layer on the device (ohgpu_ogg_*, csrc/ogg_page_kernel.hip) against the independent model (tests/ogg_textbook.py),
byte for byte: every result, every packet record a stream has room for, and the whole destination arena, which is pre-filled with
0xA5 and has guard bytes round every run.  The shapes are the smallest at which a kernel can go wrong: pages of 27, 28 and 29 bytes,
pages round one lane's slice (16 bytes) and round a wave's worth of slices (1024), the largest page; a piece at every source address
mod 16 going to every destination address mod 16; every named and every recorded session; a body that holds a whole valid page; the
mapping header and its two errors; a packet table of no room and of too little; an empty stream and an empty batch; a second run of
one batch on other bytes; more candidates than the list holds; and more pages than one trip of the verify and gather launches covers."""
import numpy as np
import pytest

import ogg_cases as GC
import ogg_textbook as OX
from device_shape import MAX_WAVES_PER_CU, compute_units
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

WAVES, GROUPS_PER_CU = 4, 8          # kOggWaves, kGroupsPerCu: ogg_wave_blocks(items, cus) = min(ceil(items / 4), 8 * cus) workgroups


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def run(ctx, job, runs=1):
    capi.ogg_batch_check(job.descs, job.n_packets, job.src.size, job.dst0.size)
    d_src, d_dst = ctx.upload(job.src), ctx.upload(job.dst0)
    b = ctx.ogg_batch(job.descs, job.n_packets, job.src.size, job.dst0.size)
    try:
        for _ in range(runs):
            ctx.copy_h2d(d_dst, job.dst0)
            ctx.ogg_run(b, d_src, d_dst)
            results, packets = ctx.ogg_results(b, len(job.streams), job.n_packets)
            GC.assert_same(results, packets, ctx.download(d_dst, job.dst0.size).tobytes(), job)
        assert all(ms >= 0 for ms in ctx.ogg_phase_ms(b))
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return results, packets


def test_every_named_and_every_recorded_session(ctx):
    named = GC.sessions()
    golden = [GC.stream(data, serial=rec["serial"], flags=OX.ANY_SEQ if rec["any_seq"] else 0) for data, rec in GC.load_golden().values()]
    job = GC.Job(list(named.values()) + golden)
    names = list(named)
    assert {m["status"] for m in job.models} == set(range(6))
    inner = job.models[names.index("page_in_body")]                  # the whole valid page inside a body stayed payload
    assert inner["pages"] == 2 and b"OggS" in inner["packets"][0]["data"]
    mapping = job.models[names.index("mapping")]
    assert mapping["packets"][0]["flags"] & OX.PACKET_MAPPING_HEADER and mapping["run"][:4] == b"fLaC"
    assert [job.models[names.index(n)]["status"] for n in ("mapping_short", "mapping_magic", "mapping_version")] == [OX.NOT_FLAC, OX.NOT_FLAC, OX.UNSUPPORTED_MAPPING]
    run(ctx, job)


def test_pages_of_every_size_where_the_slices_change(ctx):
    rng = GC.Lcg(9)
    sizes = [27, 28, 29] + list(range(30, 70)) + [1023, 1024, 1025, 1039, 1040, 1041, 1087, 1088, 1089, 4095, 4096, 4097, 65306, 65307]
    pages = [GC.page_of_size(n, 3, k, rng) for k, n in enumerate(sizes)]
    assert [len(p) for p in pages] == sizes
    pages.append(GC.page(3, len(sizes), [0, 3], b"end", OX.CONTINUED, 1))       # (the largest page's packet ends here)
    flipped = bytearray(b"".join(pages))
    flipped[-40000] ^= 1                                                         # one bit of the largest page's body
    job = GC.Job([GC.stream(b"".join(pages), serial=3), GC.stream(b"".join(pages[5:]), serial=3, expect_seq=5), GC.stream(flipped, serial=3)])
    assert [m["status"] for m in job.models] == [OX.OK, OX.OK, OX.LOST_SYNC] and job.models[2]["pages"] == len(sizes) - 1
    run(ctx, job)


def test_every_source_alignment_to_every_destination_alignment(ctx):
    rng = GC.Lcg(16)
    streams = []
    for i in range(16):
        pages = [GC.page(i, k, [n], rng.bytes(n), 0, k) for k, n in enumerate(1 + rng.below(90) for _ in range(200))]
        streams.append(GC.stream(b"".join(pages), serial=i))
    job = GC.Job(streams)
    seen = set()
    for d, m in zip(job.descs, job.models):
        assert m["status"] == OX.OK and len(m["packets"]) == 200
        for k in m["packets"]:
            seen.add(((int(d["src_offset"]) + k["page_offset"] + 28) % 16, (int(d["dst_offset"]) + k["run_pos"]) % 16))
    assert seen == {(a, b) for a in range(16) for b in range(16)}                # (d_src and d_dst are 256-byte aligned)
    run(ctx, job)


def test_packet_tables_of_no_room_and_too_little(ctx):
    named = GC.sessions()
    job = GC.Job([dict(named["sizes"], packet_capacity=0), dict(named["three_pages"], packet_capacity=2), named["mapping"]])
    results, _ = run(ctx, job)
    assert [int(r["packets"]) for r in results] == [7, 3, 3]


def test_an_empty_stream_and_an_empty_batch(ctx):
    named = GC.sessions()
    run(ctx, GC.Job([named["empty"], named["sizes"], named["empty"], named["short"]]))
    run(ctx, GC.Job([named["empty"]]))
    b = ctx.ogg_batch(np.zeros(0, dtype=capi.OGG_STREAM_DESC), 0, 0, 0)
    try:
        ctx.ogg_run(b, None, None)
        results, packets = ctx.ogg_results(b, 0, 0)
        assert results.size == 0 and packets.size == 0
    finally:
        ctx.batch_destroy(b)


def test_a_second_run_on_other_bytes_allocates_nothing(ctx):
    rng = GC.Lcg(77)
    def bytes_of(seed_packets):
        return b"".join(GC.mux(seed_packets, 4, max_segments=3))
    first = bytes_of([rng.bytes(n) for n in (5, 900, 0, 300, 41)])
    other = bytearray(bytes_of([rng.bytes(n) for n in (300, 41, 500, 99)]))
    assert len(first) > len(other)
    other += bytes(len(first) - len(other) - 30) + b"OggS" + bytes(26)            # same length: zeros where a page should follow
    jobs = [GC.Job([GC.stream(first, serial=4)]), GC.Job([GC.stream(bytes(other), serial=4)])]
    assert jobs[0].models[0]["status"] == OX.OK and jobs[1].models[0]["status"] == OX.LOST_SYNC
    assert jobs[0].src.size == jobs[1].src.size and jobs[0].n_packets >= jobs[1].n_packets
    jobs[1].n_packets = jobs[0].n_packets
    d_src, d_dst = ctx.malloc(jobs[0].src.size), ctx.malloc(jobs[0].dst0.size)
    b = ctx.ogg_batch(jobs[0].descs, jobs[0].n_packets, jobs[0].src.size, jobs[0].dst0.size)
    try:
        allocs = []
        for job in (jobs[0], jobs[1], jobs[0]):
            ctx.copy_h2d(d_src, job.src)
            ctx.copy_h2d(d_dst, job.dst0)
            ctx.sync()
            ctx.ogg_run(b, d_src, d_dst)
            results, packets = ctx.ogg_results(b, 1, job.n_packets)
            GC.assert_same(results, packets, ctx.download(d_dst, job.dst0.size).tobytes(), job)
            allocs.append(ctx.device_allocations())
        assert allocs[0] == allocs[1] == allocs[2]
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)


def test_more_candidates_than_the_list_holds(ctx):
    """"OggS" every four bytes is a page image every four bytes (103 segments of about a hundred bytes, all inside the stream): three
    times what the list holds.  The real pages round it may or may not be among those listed; the walk checks what it was not given."""
    rng = GC.Lcg(31)
    body = b"OggS" * 6000 + b"".join(GC.mux([rng.bytes(50)], 5))
    pages = GC.mux([body, rng.bytes(700), b"OggS" * 4000], 5, max_segments=40)
    data = b"".join(pages)
    images = sum(1 for p in range(0, len(data) - 4, 1) if data[p:p + 4] == b"OggS" and data[p + 26:p + 27] == b"g" and p + 27 + 103 + 103 * 115 < len(data))
    assert images > 2 * (len(data) // 27 + 1)
    job = GC.Job([GC.stream(data, serial=5), GC.stream(b"OggS" * 5000, serial=5)])
    assert [m["status"] for m in job.models] == [OX.OK, OX.LOST_SYNC] and len(job.models[0]["packets"]) == 3
    run(ctx, job)


def test_the_host_buffer_call(ctx):
    named = GC.sessions()
    job = GC.Job([named["mapping"], named["gap"], named["three_pages"]])
    dst = job.dst0.copy()
    results, packets = ctx.ogg_process_host(job.descs, job.n_packets, job.src, dst)
    GC.assert_same(results, packets, dst.tobytes(), job)


def trips_need(cus):
    return 2 * max(GROUPS_PER_CU * WAVES, MAX_WAVES_PER_CU) * cus + 67


def test_more_pages_than_one_trip_of_the_verify_and_gather_launches(ctx):
    """Both are persistent: a wave per candidate / per piece, the launch capped at 8 workgroups of 4 waves a CU, every wave going
    round its list in strides of the launch's waves.  More than 2 x that + 67 pages of 29 bytes: every wave makes two trips and the
    lowest-numbered ones a third.  Every page has one packet of one byte, so every page is a candidate and a piece."""
    cus = compute_units()
    n_streams = 6
    per_stream = trips_need(cus) // n_streams + 3
    rng = GC.Lcg(1000 + cus)
    streams = []
    for i in range(n_streams):
        first = (0, 0xFFFFFF00, 7)[i % 3]
        pages = [GC.page(i, first + k, [1], bytes([rng.below(256)]), 0, k) for k in range(per_stream)]
        assert all(len(p) == 29 for p in pages)
        streams.append(GC.stream(b"".join(pages), serial=i, expect_seq=first, packet_capacity=5))
    job = GC.Job(streams)
    total = sum(m["pages"] for m in job.models)
    assert total == n_streams * per_stream > trips_need(cus) == 2 * max(8 * 4, 32) * cus + 67
    cand_cap = sum(len(s["data"]) // 27 + 1 for s in streams)
    assert min(-(-cand_cap // WAVES), cus * GROUPS_PER_CU) == cus * GROUPS_PER_CU                  # the launches ARE capped
    assert all(m["status"] == OX.OK and len(m["run"]) == per_stream for m in job.models)
    run(ctx, job, runs=2)
