"""The model of the MPEG-4 container layer (tests/mp4_textbook.py) against the muxer's own record (tests/mp4_cases.py): where the muxer
put every packet and which frame each begins at is the truth, made by no parser.  All eleven Apple Lossless fixtures in every chunking,
every named way of writing a good file, the named malformed files with the status each must get, prefixes, and a census that fails
when a named feature goes missing from the cases."""
import pytest

import alac_cases as AC
import mp4_cases as MC
import mp4_textbook as MX


@pytest.mark.parametrize("name", list(AC.FIXTURES))
def test_every_fixture_in_every_chunking(name):
    fx = AC.load_fixture(name)
    for per_chunk in MC.CHUNKINGS.values():
        for co64 in (False, True):
            for moov_last in (False, True):
                m = MC.fixture_file(fx, per_chunk=per_chunk, co64=co64, moov_last=moov_last)
                model = MX.demux(m.data, m.n)
                MC.check_against_record(model, m)
                assert model["samples_available"] == m.n and model["samples_refused"] == 0 and model["first_bad_sample"] == MX.NO_SAMPLE
                assert b"".join(m.data[a:a + n] for a, n in model["rows"]) == b"".join(fx["packets"])
                assert model["frames"] == fx["meta"]["frames"]


def test_every_named_good_file():
    for name, m in MC.named_good().items():
        model = MX.demux(m.data, m.n)
        MC.check_against_record(model, m)
        assert model["samples_refused"] == 0, name
        mdat = m.find("mdat")
        assert (model["moov_offset"], model["mdat_offset"]) == (m.find("moov")[0], mdat[0]) and model["mdat_bytes"] == mdat[2] - mdat[1], name


def test_every_named_malformed_file():
    for name, (data, status, codec) in MC.named_malformed().items():
        model = MX.demux(data, 8)
        assert model["status"] == status, name
        assert model["codec"] == (int.from_bytes(codec, "big") if codec else 0), name
        assert model["rows"] == [] and model["samples"] == 0 and model["first_bad_sample"] == MX.NO_SAMPLE, name


def test_a_capacity_below_the_sample_count_and_of_none():
    m = MC.named_good()["entry_per_chunk"]
    for capacity in (0, 1, m.n - 1):
        model = MX.demux(m.data, capacity)
        MC.check_against_record(model, m)
        assert len(model["rows"]) == capacity == model["samples_available"] and model["samples"] == m.n


def test_a_prefix_plays_what_lies_inside_it():
    fx = AC.load_fixture("stereo16_fl1024")
    m = MC.fixture_file(fx, per_chunk=[2])
    cut = m.offsets[2] + 5                                   # inside the third packet
    model = MX.demux(m.data[:cut], m.n)
    assert model["status"] == MX.OK and model["samples"] == 4
    assert (model["samples_available"], model["samples_refused"], model["first_bad_sample"]) == (2, 2, 2)
    assert model["rows"] == [(m.offsets[0], m.sizes[0]), (m.offsets[1], m.sizes[1]), None, None]
    last = MC.fixture_file(fx, moov_last=True)
    assert MX.demux(last.data[:last.find("moov")[0] + 9], 4)["status"] == MX.TRUNCATED


def test_sizes_and_offsets_that_would_wrap_32_bits_are_refused():
    m = MC.mux(MC.pattern_packets(6), MC.PATTERN_COOKIE, per_chunk=[3], co64=True)
    co, stsz = m.find("co64"), m.find("stsz")
    far = MC.patched(m, co[1] + 8 + 8, (1 << 32) + m.offsets[3], 8)          # the second chunk: 2^32 + a valid offset
    model = MX.demux(far, 6)
    assert model["rows"][:3] == list(zip(m.offsets, m.sizes))[:3] and model["rows"][3:] == [None] * 3 and model["samples_refused"] == 3
    huge = MC.patched(m, stsz[1] + 12 + 4, 0xffffffff)                       # the second sample of the first chunk
    model = MX.demux(huge, 6)
    assert model["rows"] == [(m.offsets[0], m.sizes[0]), None, None] + list(zip(m.offsets, m.sizes))[3:]
    assert (model["samples_available"], model["first_bad_sample"], model["samples_refused"]) == (1, 1, 2)


def test_the_seek_lands_on_the_packet_that_holds_the_frame():
    m = MC.fixture_file(AC.load_fixture("stereo16_fl1024"), per_chunk=[3])
    rows = MX.demux(m.data, 4)["samples_rows"]
    assert MX.seek(rows, 0) == (0, 0) and MX.seek(rows, 1023) == (0, 0) and MX.seek(rows, 1024) == (1, 1024)
    assert MX.seek(rows, 2 * 1024 + 17) == (2, 2048) and MX.seek(rows, m.total_frames - 1) == (3, 3072) and MX.seek(rows, m.total_frames) is None


def test_census_of_what_the_cases_cover():
    good, bad = MC.named_good(), MC.named_malformed()
    assert {status for _, status, _ in bad.values()} | {MX.OK} == set(range(6))
    marks = {name: {x[0].split("/")[-1] for x in m.marks} for name, m in good.items()}
    assert any("co64" in k for k in marks.values()) and any("stco" in k for k in marks.values())
    assert good["box_size_64"].data[good["box_size_64"].find("moov")[0]:][:4] == b"\0\0\0\1"                       # a 64-bit box size
    assert good["size_0_last"].data[good["size_0_last"].find("mdat")[0]:][:4] == b"\0\0\0\0"                       # size 0: to the end
    assert good["size_0_last_moov"].data[good["size_0_last_moov"].find("moov")[0]:][:4] == b"\0\0\0\0"
    stsz = good["uniform_stsz"].find("stsz")
    assert good["uniform_stsz"].data[stsz[1] + 4:stsz[1] + 8] == (40).to_bytes(4, "big") and stsz[2] - stsz[1] == 12     # no array
    for name in ("two_tracks_alac_first", "two_tracks_alac_second"):
        assert sum(1 for x in good[name].marks if x[0] == "moov/trak") == 2
    assert good["two_tracks_alac_second"].data.index(b"mp4a") < good["two_tracks_alac_second"].data.index(b"alac")
    for name in ("moov_last", "moov_last_co64", "size_0_last_moov"):
        assert good[name].find("moov")[0] > good[name].find("mdat")[0]
    assert set(MC.CHUNKINGS) == {"one_chunk", "one_a_chunk", "three_short_last", "changing"}
    assert len(AC.FIXTURES) == 11
