"""What the chained-stream tests share: the named chained sessions, built with tests/ogg_cases.py's page writer and muxer, and a Job
as ogg_cases.Job whose descriptors carry OHGPU_OGG_FOLLOW_LINKS and the link magic and whose expectations come from
tests/ogg_links_textbook.py."""
import numpy as np

import ogg_cases as GC
import ogg_links_textbook as LX
import ogg_textbook as OX

V, F = LX.VORBIS_MAGIC, LX.FLAC_MAGIC


def stream(data, magic=V, follow=True, **kw):
    """ogg_cases.stream's arguments and the magic; follow=False leaves the flag and the magic out of the descriptor."""
    s = GC.stream(data, **kw)
    s["magic"] = magic if follow else None
    if follow:
        s["flags"] |= LX.FOLLOW_LINKS
    return s


def link(rng, serial, sizes, seq0=0, magic=V, eos=True, max_segments=255, granule0=0, head_bytes=23):
    """The pages of one link: a first packet that begins with the magic alone on the first page, then packets of `sizes` bytes."""
    first = GC.mux([magic + rng.bytes(head_bytes)], serial, seq0, granules=[0], eos=False)
    rest = [rng.bytes(n) for n in sizes]
    pages = GC.mux(rest, serial, seq0 + 1, max_segments=max_segments, granules=[granule0 + 10 * (k + 1) for k in range(len(rest))], bos=False, eos=eos)
    return first + pages


def sessions():
    rng = GC.Lcg(1066)
    out = {}
    a, b, c = link(rng, 11, [40, 300, 7]), link(rng, 22, [5, 600], granule0=1000000), link(rng, 33, [90], seq0=9)
    out["two_links"] = stream(b"".join(a + b), serial=11)
    out["three_links"] = stream(b"".join(a + b + c), serial=11)
    out["three_links_any_serial"] = stream(b"".join(a + b + c), flags=OX.ANY_SERIAL | OX.ANY_SEQ)
    out["no_eos_before"] = stream(b"".join(link(rng, 11, [40, 41], eos=False) + b), serial=11)
    cut = link(rng, 11, [30, 255 * 3 + 9], max_segments=2, eos=False)[:-1]            # the last page is missing: a packet stays open
    out["open_at_boundary"] = stream(b"".join(cut + b + c), serial=11)
    foreign = GC.mux([b"\x80theora" + rng.bytes(20)], 77, granules=[0], eos=False)
    out["foreign_first_page"] = stream(b"".join(a[:2] + foreign + a[2:]), serial=11)
    out["foreign_then_link"] = stream(b"".join(a + foreign + b), serial=11)
    g1, g2 = link(rng, 5, [50, 60, 70], max_segments=1), link(rng, 6, [51, 61, 71], max_segments=1)
    group = [g1[0], g2[0]] + [x for pair in zip(g1[1:], g2[1:]) for x in pair]
    out["opening_group"] = stream(b"".join(group), serial=5)
    out["opening_group_any_serial"] = stream(b"".join(group), flags=OX.ANY_SERIAL)
    five = link(rng, 44, [20, 30, 40, 50], seq0=5, max_segments=1)
    out["first_page_number_5"] = stream(b"".join(a + five), serial=11)
    out["hole_in_link"] = stream(b"".join(a + five[:3] + five[4:]), serial=11)
    out["reused_serial"] = stream(b"".join(a + link(rng, 11, [12, 13])), serial=11)
    out["magic_length_0"] = stream(b"".join(a + foreign + b), magic=b"", serial=11)
    out["magic_longer_than_body"] = stream(b"".join(a + GC.mux([V[:5]], 22, granules=[0], eos=False) + b[1:]), serial=11)
    head = b"\x7fFLAC\x01\x00\x00\x02fLaC" + rng.bytes(38)
    fa = GC.mux([head, rng.bytes(40), rng.bytes(300)], 7, max_segments=2)
    head2 = b"\x7fFLAC\x01\x00\x00\x01fLaC" + rng.bytes(38)
    fb = GC.mux([head2], 8, eos=False) + GC.mux([rng.bytes(64), rng.bytes(500)], 8, 1, bos=False)
    out["flac_mapping"] = stream(b"".join(fa + fb), magic=F, serial=7, flags=OX.FLAC_MAPPING)
    out["flac_mapping_bad_version"] = stream(b"".join(fa + GC.mux([b"\x7fFLAC\x02\x00\x00\x01fLaC" + rng.bytes(38), rng.bytes(9)], 8)), magic=F, serial=7, flags=OX.FLAC_MAPPING)
    out["small_capacity"] = stream(b"".join(a + b + c), serial=11, packet_capacity=3)
    out["no_capacity"] = stream(b"".join(a + b), serial=11, packet_capacity=0)
    # rule L4: the range ends before a packet of the link has completed (a whole first page whose packet goes on; a first page alone)
    long_first = GC.page(22, 0, [255], V + rng.bytes(248), OX.BOS, -1)
    out["link_packet_open_at_end"] = stream(b"".join(a) + long_first, serial=11)
    out["link_packet_open_then_closed"] = stream(b"".join(a) + long_first + GC.page(22, 1, [3, 8], rng.bytes(11), OX.CONTINUED, 5), serial=11)
    out["link_page_without_segments"] = stream(b"".join(a) + GC.page(22, 0, [], b"", OX.BOS, -1), magic=b"", serial=11)
    out["ends_in_links_first_page"] = stream(b"".join(a + b)[:len(b"".join(a)) + 40], serial=11)
    out["lost_sync_in_link"] = stream(b"".join(a + b[:2]) + b"\x00" * 30, serial=11)
    for name in ("two_links", "three_links", "open_at_boundary", "opening_group", "flac_mapping", "magic_length_0"):
        s = out[name]
        out[name + "_unfollowed"] = stream(s["data"], follow=False, serial=s["serial"], flags=s["flags"] & ~LX.FOLLOW_LINKS)
    return out


def model(s):
    return LX.demux(s["data"], s["serial"], s["expect_seq"], s["first_page_segment"], s["flags"], s["magic"] or b"")


class Job(GC.Job):
    """ogg_cases.Job for streams of stream() above: the same arenas, the magic in the descriptors, the expectations of the links
    model."""

    def __init__(self, streams, seed=5):
        plain = [dict(s, flags=s["flags"] & ~LX.FOLLOW_LINKS) for s in streams]
        GC.Job.__init__(self, plain, seed)                 # the layout does not depend on the model but for the packet capacities
        self.streams = streams
        self.models = [model(s) for s in streams]
        from ohpipeline_amd import capi
        links_view = self.descs.view(capi.OGG_STREAM_DESC_LINKS)
        pk_at = 0
        for i, (s, m) in enumerate(zip(streams, self.models)):
            cap = len(m["packets"]) if s["packet_capacity"] is None else s["packet_capacity"]
            self.descs["flags"][i], self.descs["packet_first"][i], self.descs["packet_capacity"][i] = s["flags"], pk_at, cap
            if s["magic"] is not None:
                links_view["link_magic_bytes"][i] = len(s["magic"])
                links_view["link_magic"][i, :len(s["magic"])] = np.frombuffer(s["magic"], dtype=np.uint8)
            pk_at += cap + (i % 2)
        self.n_packets = pk_at
        self.want = self.dst0.copy()
        for d, m in zip(self.descs, self.models):
            a = int(d["dst_offset"])
            self.want[a:a + len(m["run"])] = np.frombuffer(m["run"], dtype=np.uint8)


def assert_same(results, packets, arena, job):
    from ohpipeline_amd import capi
    GC.assert_same(results, packets, arena, job)
    assert links_of(results) == [m["links"] for m in job.models]
    assert not np.ascontiguousarray(results).view(capi.OGG_STREAM_RESULT_LINKS)["reserved2_high"].any()


def links_of(results):
    from ohpipeline_amd import capi
    return [int(x) for x in np.ascontiguousarray(results).view(capi.OGG_STREAM_RESULT_LINKS)["links"]]
