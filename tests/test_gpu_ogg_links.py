"""Chained streams through the Ogg page layer on the device (OHGPU_OGG_FOLLOW_LINKS; the walk of csrc/ogg_page_core.h in
csrc/ogg_page_kernel.hip's chain phase) against the independent model (tests/ogg_links_textbook.py), byte for byte: every result with
its `links`, every packet record a stream has room for, and the whole destination arena with its guard bytes.  Every named chained
session in one batch; 1, 64 and 65 two-link streams, the chain phase being a lane a stream in workgroups of 64; rule 7's cut at the
offsets where a link can go wrong; one stream laid across byte 2^32 of the source arena; and the same bytes without the flag, which
must give what the plain model gives."""
import numpy as np
import pytest

import far_cases as FAR
import ogg_cases as GC
import ogg_links_cases as LC
import ogg_links_textbook as LX
import ogg_textbook as OX
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def run(ctx, job):
    capi.ogg_batch_check(job.descs, job.n_packets, job.src.size, job.dst0.size)
    d_src, d_dst = ctx.upload(job.src), ctx.upload(job.dst0)
    b = ctx.ogg_batch(job.descs, job.n_packets, job.src.size, job.dst0.size)
    try:
        ctx.ogg_run(b, d_src, d_dst)
        results, packets = ctx.ogg_results(b, len(job.streams), job.n_packets)
        LC.assert_same(results, packets, ctx.download(d_dst, job.dst0.size).tobytes(), job)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return results, packets


def test_every_named_chained_session_in_one_batch(ctx):
    named = LC.sessions()
    job = LC.Job(list(named.values()))
    assert {m["links"] for m in job.models} == {0, 1, 2} and {m["status"] for m in job.models} == {OX.OK, OX.LOST_SYNC, OX.HOLE, OX.UNSUPPORTED_MAPPING}
    results, packets = run(ctx, job)
    i = list(named).index("three_links")
    first = int(job.descs["packet_first"][i])
    assert [int(packets[first + k]["flags"]) & LX.PACKET_LINK for k in range(9)] == [0, 0, 0, 0, 8, 0, 0, 8, 0] and int(results[i]["serial"]) == 33


@pytest.mark.parametrize("n", [1, 64, 65])
def test_two_link_streams_a_lane_each(ctx, n):
    rng = GC.Lcg(400 + n)
    streams = []
    for i in range(n):
        a = LC.link(rng, 2 * i + 1, [1 + rng.below(300), 1 + rng.below(40)], seq0=rng.below(4), eos=bool(i % 2))
        b = LC.link(rng, 2 * i + 2, [1 + rng.below(90), 255, 1 + rng.below(600)], seq0=rng.below(9), max_segments=2, granule0=1000 * i)
        streams.append(LC.stream(b"".join(a + b), serial=2 * i + 1, flags=OX.ANY_SEQ))
    job = LC.Job(streams)
    assert all((m["links"], m["serial"], m["status"], len(m["packets"])) == (1, 2 * i + 2, OX.OK, 7) for i, m in enumerate(job.models))
    run(ctx, job)


def test_the_two_call_cut_where_a_link_can_go_wrong(ctx):
    """[0, cut) and the rest from where the first call stops, as two streams of one batch: a cut inside the link's first page, between
    its header pages, inside a packet that is open over the link's first page, inside an open packet of the link before, at the end."""
    named = LC.sessions()
    streams, expected_links = [], 0
    for name, cuts in (("two_links", lambda a, n: [a + 10, a + 58, a + 80, n - 5, n]), ("open_at_boundary", lambda a, n: [a - 20, a + 3, a + 200]),
                       ("link_packet_open_then_closed", lambda a, n: [a + 100, a + 283, a + 290, n])):
        s = named[name]
        whole = LC.model(s)
        at = whole["packets"][[k for k, pk in enumerate(whole["packets"]) if pk["flags"] & LX.PACKET_LINK][0]]["page_offset"]
        for cut in cuts(at, len(s["data"])):
            one = LC.stream(s["data"][:cut], magic=s["magic"], serial=s["serial"])
            m = LC.model(one)
            two = LC.stream(s["data"][m["bytes_consumed"]:], magic=s["magic"], serial=m["serial"], expect_seq=m["next_seq"], first_page_segment=m["resume_segment"])
            m2 = LC.model(two)
            assert m["status"] == OX.OK and m["run"] + m2["run"] == whole["run"] and m["links"] + m2["links"] == whole["links"] and m2["serial"] == whole["serial"]
            streams += [one, two]
            expected_links += whole["links"]
    job = LC.Job(streams)
    results, _ = run(ctx, job)
    assert sum(LC.links_of(results)) == expected_links
    assert any(m["links"] == 0 and m["bytes_consumed"] < len(s["data"]) - 200 for s, m in zip(job.streams[::2], job.models[::2]))       # rule L4 was taken


def test_without_the_flag_the_same_batch_is_the_plain_one(ctx):
    named = LC.sessions()
    follow = [s for s in named.values() if s["flags"] & LX.FOLLOW_LINKS]
    plain = [GC.stream(s["data"], serial=s["serial"], expect_seq=s["expect_seq"], first_page_segment=s["first_page_segment"], flags=s["flags"] & ~LX.FOLLOW_LINKS,
                       packet_capacity=s["packet_capacity"]) for s in follow]
    job = GC.Job(plain)
    assert not job.descs["reserved"].any() and not (job.descs["flags"] & LX.FOLLOW_LINKS).any()
    d_src, d_dst = ctx.upload(job.src), ctx.upload(job.dst0)
    b = ctx.ogg_batch(job.descs, job.n_packets, job.src.size, job.dst0.size)
    try:
        ctx.ogg_run(b, d_src, d_dst)
        results, packets = ctx.ogg_results(b, len(job.streams), job.n_packets)
        GC.assert_same(results, packets, ctx.download(d_dst, job.dst0.size).tobytes(), job)
        assert not results["reserved2"].any() and not (packets["flags"] & LX.PACKET_LINK).any()
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)


def test_a_chained_stream_across_2_to_the_32_of_the_source_arena(ctx):
    """As tests/test_gpu_far_offsets.py's test_ogg: the stream's bytes straddle byte 2^32 of the source arena, the link's first page
    among them; results and records are relative to the stream's own offsets and equal for both copies."""
    named = LC.sessions()
    job = LC.Job([named["open_at_boundary"], named["three_links"]])
    arenas = FAR.FarArenas(ctx)
    try:
        twin = FAR.Twin(arenas, job.src, job.dst0, "s32_s31", *FAR.ALIGN["ogg"], GC.FILL)
        twin.prepare()
        lo, hi = twin.src_at[1] + int(job.descs["src_offset"][0]), twin.src_at[1] + int(job.descs["src_offset"][0]) + len(job.streams[0]["data"])
        assert lo < (1 << 32) < hi
        copies = [FAR.relocate("ogg", {"descs": job.descs}, twin.src_at[k], twin.dst_at[k])["descs"] for k in (0, 1)]
        copies[1]["packet_first"] += job.n_packets
        descs = np.concatenate(copies)
        capi.ogg_batch_check(descs, 2 * job.n_packets, FAR.SPAN, FAR.SPAN)
        batch = ctx.ogg_batch(descs, 2 * job.n_packets, FAR.SPAN, FAR.SPAN)
        try:
            ctx.ogg_run(batch, arenas.src, arenas.dst)
            results, packets = ctx.ogg_results(batch, len(descs), 2 * job.n_packets)
        finally:
            ctx.batch_destroy(batch)
        n = len(job.streams)
        for k in (0, 1):
            LC.assert_same(results[k * n:(k + 1) * n], packets[k * job.n_packets:(k + 1) * job.n_packets], job.want.tobytes(), job)
        twin.check(job.want, "ogg links s32_s31")
    finally:
        arenas.close()
