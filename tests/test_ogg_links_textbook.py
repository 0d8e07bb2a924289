"""The chained-stream model (tests/ogg_links_textbook.py) and its committed cases (tests/ogg_links_cases.py) held to the text of
rules L1-L5 in include/ohgpu.h, without a device and without the library: what every named case must give, a census -- every rule is
hit by a committed case -- the same inputs without the flag, and rule 7's two-call cut at every byte offset of a two-link stream."""
import pytest

import ogg_cases as GC
import ogg_links_cases as LC
import ogg_links_textbook as LX
import ogg_textbook as OX

NAMED = LC.sessions()
MODELS = {name: LC.model(s) for name, s in NAMED.items()}
LINK, BOS = LX.PACKET_LINK, OX.PACKET_BOS


def link_flags(m):
    return [k for k, pk in enumerate(m["packets"]) if pk["flags"] & LINK]


def test_what_the_named_cases_give():
    m = MODELS
    assert (m["two_links"]["links"], m["two_links"]["serial"], link_flags(m["two_links"])) == (1, 22, [4])
    assert (m["three_links"]["links"], m["three_links"]["serial"], link_flags(m["three_links"])) == (2, 33, [4, 7])
    assert all(m["three_links"]["packets"][k]["flags"] & BOS for k in (0, 4, 7))
    assert m["three_links"]["packets"][4]["data"][:7] == LX.VORBIS_MAGIC and m["three_links"]["last_granule"] == 10     # the granules restart
    assert m["two_links"]["last_granule"] == 1000020
    assert {k: m["three_links_any_serial"][k] for k in ("links", "serial", "run")} == {k: m["three_links"][k] for k in ("links", "serial", "run")}
    assert m["no_eos_before"]["links"] == 1 and not any(pk["flags"] & OX.PACKET_EOS for pk in m["no_eos_before"]["packets"][:3])
    plain = MODELS["open_at_boundary_unfollowed"]
    assert plain["bytes_consumed"] < len(NAMED["open_at_boundary"]["data"]) and plain["resume_segment"]               # a packet is open there
    assert m["open_at_boundary"]["links"] == 2 and m["open_at_boundary"]["packets"][:2] == plain["packets"]            # ... and is dropped
    assert (m["foreign_first_page"]["links"], m["foreign_first_page"]["pages_ignored"]) == (0, 1)
    assert (m["foreign_then_link"]["links"], m["foreign_then_link"]["pages_ignored"], m["foreign_then_link"]["serial"]) == (1, 1, 22)
    for name in ("opening_group", "opening_group_any_serial"):
        assert (m[name]["links"], m[name]["serial"], m[name]["pages_ignored"], m[name]["status"]) == (0, 5, 4, OX.OK)
    five = m["first_page_number_5"]
    assert five["links"] == 1 and five["packets"][4]["page_seq"] == 5 and five["next_seq"] == 10 and five["status"] == OX.OK
    assert (m["hole_in_link"]["status"], m["hole_in_link"]["links"], m["hole_in_link"]["next_seq"]) == (OX.HOLE, 1, 8)
    assert (m["reused_serial"]["status"], m["reused_serial"]["links"]) == (OX.HOLE, 0)
    assert (m["magic_length_0"]["links"], m["magic_length_0"]["serial"]) == (1, 77)        # the foreign page is taken, the one behind it is its group
    assert m["magic_longer_than_body"]["links"] == 0
    fl = m["flac_mapping"]
    assert fl["links"] == 1 and [pk["flags"] for pk in fl["packets"]][3] == LINK | BOS | OX.PACKET_MAPPING_HEADER and fl["packets"][3]["data"][:4] == b"fLaC"
    assert (m["flac_mapping_bad_version"]["status"], m["flac_mapping_bad_version"]["links"]) == (OX.UNSUPPORTED_MAPPING, 1)
    assert m["small_capacity"]["links"] == 2 and NAMED["small_capacity"]["packet_capacity"] < link_flags(m["small_capacity"])[0]
    a_bytes = m["ends_in_links_first_page"]["bytes_consumed"]
    for name in ("link_packet_open_at_end", "link_page_without_segments", "ends_in_links_first_page"):                # rule L4
        assert {k: m[name][k] for k in ("status", "links", "serial", "bytes_consumed", "resume_segment", "next_seq", "pages")} == \
            dict(status=OX.OK, links=0, serial=11, bytes_consumed=a_bytes, resume_segment=0, next_seq=2, pages=2), name
    assert (m["link_packet_open_then_closed"]["links"], link_flags(m["link_packet_open_then_closed"])) == (1, [4])
    assert (m["lost_sync_in_link"]["status"], m["lost_sync_in_link"]["links"]) == (OX.LOST_SYNC, 1)


def test_every_rule_is_hit_by_a_committed_case():
    hit = set()
    for name, (s, m) in ((n, (NAMED[n], MODELS[n])) for n in NAMED):
        if not s["flags"] & LX.FOLLOW_LINKS:
            hit.add("unfollowed")
            continue
        plain = OX.demux(s["data"], s["serial"], s["expect_seq"], s["first_page_segment"], s["flags"] & ~LX.FOLLOW_LINKS)
        if m["links"]:
            hit.add("L1 taken")
            first = m["packets"][link_flags(m)[0]] if link_flags(m) else None
            if first and first["page_seq"] != 0:
                hit.add("L2 any page number")
            if first and first["flags"] & OX.PACKET_MAPPING_HEADER:
                hit.add("L2 mapping header")
            if plain["status"] == OX.OK and plain["bytes_consumed"] < len(s["data"]) and m["bytes_consumed"] == len(s["data"]):
                hit.add("L2 open packet dropped")
            if m["links"] > 1:
                hit.add("L3 more than one")
            if s["packet_capacity"] is not None and s["packet_capacity"] < len(m["packets"]):
                hit.add("L3 unrecorded")
            if m["status"] == OX.HOLE:
                hit.add("L2 hole inside a link")
            if m["pages_ignored"] and len(s["magic"]):
                hit.add("L1 magic refused, then taken")
            if not len(s["magic"]):
                hit.add("L1 magic of no bytes")
        else:
            if m["status"] == OX.HOLE:
                hit.add("L5 reused serial")
            elif m["pages_ignored"] > 1 and m["serial"] in (5,):
                hit.add("L1 opening group")
            elif m["pages_ignored"]:
                hit.add("L1 magic refused")
            if m["bytes_consumed"] < len(s["data"]) and LX.whole_page(s["data"], m["bytes_consumed"]) is not None:
                hit.add("L4 left for the later call")
    assert hit == {"unfollowed", "L1 taken", "L2 any page number", "L2 mapping header", "L2 open packet dropped", "L3 more than one", "L3 unrecorded",
                   "L2 hole inside a link", "L1 magic refused, then taken", "L1 magic of no bytes", "L5 reused serial", "L1 opening group", "L1 magic refused",
                   "L4 left for the later call"}, sorted(hit)


@pytest.mark.parametrize("name", sorted(NAMED))
def test_without_the_flag_it_is_the_plain_model(name):
    s = NAMED[name]
    flags = s["flags"] & ~LX.FOLLOW_LINKS
    got = LX.demux(s["data"], s["serial"], s["expect_seq"], s["first_page_segment"], flags, s["magic"] or b"")
    assert got == dict(OX.demux(s["data"], s["serial"], s["expect_seq"], s["first_page_segment"], flags), links=0)


def two_calls(data, cut, **kw):
    """Rule 7 and L4: the range [0, cut), then the rest from where the first call says, with its serial."""
    one = LX.demux(data[:cut], **kw)
    if one["status"] != OX.OK:
        return None
    flags = kw["flags"] & ~(OX.ANY_SERIAL | OX.ANY_SEQ) if one["pages"] else kw["flags"]
    two = LX.demux(data[one["bytes_consumed"]:], serial=one["serial"], expect_seq=one["next_seq"], first_page_segment=one["resume_segment"], flags=flags, magic=kw["magic"])
    return one, two


KEEP = ("data", "bytes", "flags", "granule", "page_seq", "segment")


@pytest.mark.parametrize("name", ["two_links", "open_at_boundary", "link_packet_open_then_closed", "flac_mapping"])
def test_the_two_call_cut_at_every_byte_offset(name):
    s = NAMED[name]
    kw = dict(serial=s["serial"], expect_seq=s["expect_seq"], first_page_segment=0, flags=s["flags"], magic=s["magic"])
    data, whole = s["data"], MODELS[name]
    assert whole["links"] >= 1 and whole["status"] == OX.OK
    for cut in range(len(data) + 1):
        one, two = two_calls(data, cut, **kw)
        joined = [dict({f: pk[f] for f in KEEP}, page_offset=pk["page_offset"]) for pk in one["packets"]] + \
                 [dict({f: pk[f] for f in KEEP}, page_offset=pk["page_offset"] + one["bytes_consumed"]) for pk in two["packets"]]
        assert joined == [dict({f: pk[f] for f in KEEP}, page_offset=pk["page_offset"]) for pk in whole["packets"]], cut
        assert one["run"] + two["run"] == whole["run"], cut
        assert one["links"] + two["links"] == whole["links"] and two["serial"] == whole["serial"], cut
        assert (two["status"], one["bytes_consumed"] + two["bytes_consumed"], two["next_seq"]) == (whole["status"], whole["bytes_consumed"], whole["next_seq"]), cut


def test_the_known_exception_of_rule_l4():
    """A range that ends exactly between two first pages of one opening group that both match the magic: the later call has not
    seen the first of them, and takes the second for a link.  Written down, not wanted."""
    s = NAMED["opening_group"]
    first_page = LX.whole_page(s["data"], 0)["size"]
    one, two = two_calls(s["data"], first_page, serial=5, expect_seq=0, first_page_segment=0, flags=s["flags"], magic=s["magic"])
    assert (one["pages"], one["bytes_consumed"]) == (1, first_page) and (two["links"], two["serial"]) == (1, 6)
    one, two = two_calls(s["data"], first_page + LX.whole_page(s["data"], first_page)["size"], serial=5, expect_seq=0, first_page_segment=0, flags=s["flags"], magic=s["magic"])
    assert (two["links"], two["serial"]) == (0, 5)                    # one page later the group is behind the cut
