"""tests/ogg_textbook.py, the independent model of the Ogg page layer, held to what does not depend on this project's code: two
checksum values, the sessions recorded from the reference's own page library (tests/golden/ogg), and the resume property of the
walk at every page boundary and at every segment of one session.  The library's own host-side checksum is held to the same values."""
import ogg_cases as GC
import ogg_textbook as OX

# The second anchor: serial 0x1234, first page, granule 0, page 0, one packet of 510 bytes b[i] = (7 i) & 255, as the reference's
# page library writes it.
ANCHOR_HEADER = bytes.fromhex("4f67675300020000000000000000341200000000000014 43d55a03ffff00".replace(" ", ""))
ANCHOR_BODY = bytes((7 * i) & 255 for i in range(510))


def test_the_checksum_of_123456789():
    assert OX.crc_bitwise(b"123456789") == 0x89A1897F == (0x765E7680 ^ 0xFFFFFFFF)
    assert OX.crc(b"123456789") == 0x89A1897F


def test_the_checksum_of_a_page_the_reference_wrote():
    page = ANCHOR_HEADER + ANCHOR_BODY
    assert len(ANCHOR_HEADER) == 30 and int.from_bytes(page[22:26], "little") == 0x5AD54314
    blank = page[:22] + bytes(4) + page[26:]
    assert OX.crc_bitwise(blank) == 0x5AD54314 and OX.page_crc(page) == 0x5AD54314
    assert GC.page(0x1234, 0, [255, 255, 0], ANCHOR_BODY, OX.BOS, 0) == page          # the tests' page writer makes the same bytes
    out = OX.demux(page, serial=0x1234)
    assert out["status"] == OX.OK and [k["data"] for k in out["packets"]] == [ANCHOR_BODY]


def test_the_table_is_the_bitwise_definition():
    rng = GC.Lcg(3)
    for n in (0, 1, 2, 3, 4, 5, 31, 255, 1000):
        data = rng.bytes(n)
        assert OX.crc(data) == OX.crc_bitwise(data)
    a, b = rng.bytes(77), rng.bytes(130)                   # linear: crc(A | B) = crc(A | zeros) ^ crc(B)
    assert OX.crc(a + b) == OX.crc(a + bytes(len(b))) ^ OX.crc(b)


def test_the_librarys_host_checksum():
    from ohpipeline_amd import capi
    assert capi.ogg_crc(b"123456789") == 0x89A1897F and capi.ogg_crc(b"") == 0
    page = ANCHOR_HEADER + ANCHOR_BODY
    assert capi.ogg_crc(page[:22] + bytes(4) + page[26:]) == 0x5AD54314


def test_the_recorded_sessions():
    golden = GC.load_golden()
    assert len(golden) == 13
    seen = set()
    for name, (data, rec) in golden.items():
        status, delivered = GC.golden_expectation(rec["events"])
        out = OX.demux(data, serial=rec["serial"], flags=OX.ANY_SEQ if rec["any_seq"] else 0)
        got = [(k["bytes"], k["granule"], 1 if k["flags"] & OX.PACKET_BOS else 0, 1 if k["flags"] & OX.PACKET_EOS else 0, GC.fnv1a32(k["data"]))
               for k in out["packets"]]
        assert (out["status"], got) == (status, delivered), name
        stop = next((i for i, e in enumerate(rec["events"]) if e[0] in ("sync", "hole")), len(rec["events"]))
        assert out["pages_ignored"] == sum(1 for e in rec["events"][:stop] if e[0] == "refused"), name
        seen.add(status)
    assert seen == {OX.OK, OX.LOST_SYNC, OX.HOLE}
    sizes = [k["bytes"] for k in OX.demux(golden["sizes"][0], serial=0x1234)["packets"]]
    assert sizes == [0, 1, 254, 255, 256, 510, 65030]
    middle = OX.demux(golden["three_pages"][0], serial=0x1234)
    assert middle["pages"] == 4 and [k["granule"] for k in middle["packets"]] == [0, -1, 3000]


def resumed(data, cut, **kw):
    """Two calls, the first over data[:cut], the second from where the first says to go on: the packets of both."""
    one = OX.demux(data[:cut], **kw)
    assert one["status"] == OX.OK
    two = OX.demux(data[one["bytes_consumed"]:], serial=one["serial"], expect_seq=one["next_seq"], first_page_segment=one["resume_segment"],
                   flags=kw.get("flags", 0) & OX.FLAC_MAPPING if one["pages"] else kw.get("flags", 0))
    return one, two


def test_resuming_gives_what_one_call_gives():
    named = GC.sessions()
    for name in ("three_pages", "sizes", "mapping", "two_serials", "ends_on_255k"):
        s = named[name]
        kw = dict(serial=s["serial"], expect_seq=s["expect_seq"], flags=s["flags"])
        whole = OX.demux(s["data"], **kw)
        assert whole["status"] == OX.OK
        data = s["data"]
        # every page boundary; for one session also every byte of every header and lacing table and a byte inside every segment
        cuts, p = {0, len(data)}, 0
        while p < len(data):
            n = data[p + 26]
            cuts.update((p, p + 13, p + 27 + n // 2))
            at = p + 27 + n
            if name == "three_pages":
                cuts.update(range(p, at + 1))
            for v in data[p + 27:p + 27 + n]:
                if name == "three_pages":
                    cuts.update((at, at + v // 2))
                at += v
            p = at
        assert p == len(data)
        for cut in sorted(cuts):
            one, two = resumed(data, cut, **kw)
            assert one["run"] + two["run"] == whole["run"], (name, cut)
            got = [(k["bytes"], k["granule"], k["flags"]) for k in one["packets"] + two["packets"]]
            assert got == [(k["bytes"], k["granule"], k["flags"]) for k in whole["packets"]], (name, cut)
            assert two["status"] == OX.OK and one["bytes_consumed"] + two["bytes_consumed"] == whole["bytes_consumed"], (name, cut)


def test_a_resume_point_past_the_page_is_refused():
    named = GC.sessions()
    assert OX.demux(**{k: v for k, v in named["bad_resume"].items() if k != "packet_capacity"})["status"] == OX.BAD_RESUME
