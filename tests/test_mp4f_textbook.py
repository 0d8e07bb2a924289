"""(These tests use the tests' own muxer and model alone: they tie the model to the muxer's record and run without the product.  What
exercises the product is tests/test_mp4f_core_cpu.py, test_mp4f_abi_host.py and the two test_gpu_mp4f_* files.)
The independent model of the fragmented MPEG-4 layer (tests/mp4f_textbook.py) held to the muxer's own record (tests/mp4f_cases.py)
on every named file: every sample's place, size, first frame and run, every run row, the gathered bytes -- the join of the samples
the muxer wrote -- and, for the malformed files, the status and the box that gave it.  No device and no library: two texts that share
nothing, one writing and one reading."""
import pytest

import mp4f_cases as FC
import mp4f_textbook as FX

GOOD, BAD, CAPS = FC.named_good(), FC.named_malformed(), FC.named_capacities()


@pytest.mark.parametrize("name", sorted(GOOD))
def test_a_good_file_reads_as_it_was_written(name):
    m = GOOD[name]
    model = FX.demux(m.data, gather=True, dst_capacity=len(m.data))
    FC.check_against_record(model, m)
    assert model["samples_refused"] == 0 and model["samples_available"] == m.n
    assert model["gathered"] == b"".join(m.data[at:at + size] for at, size in zip(m.offsets, m.sizes))
    codec_only = FX.demux(m.data, FX.CODEC_ALAC if m.codec == FC.ALAC else FX.CODEC_FLAC)
    assert codec_only["status"] == FX.OK and codec_only["run_rows"] == model["run_rows"]


def test_the_named_files_cover_what_the_format_allows():
    assert {GOOD[f"run_of_{n}"].n for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049)} == {1, 63, 64, 65, 1023, 1024, 1025, 2049}
    neg = GOOD["negative_data_offset"]
    assert all(FX.u(neg.data, t[1] + 8, 4) >= 1 << 31 for t in (neg.find("trun", k) for k in range(4)))       # every data_offset is negative
    gap = GOOD["tfdt_v1_with_a_gap"]
    assert gap.first_frames[4] == (1 << 33) + 1000 and gap.first_frames[3] + gap.frames[3] < gap.first_frames[4] and gap.first_frames[12] == gap.first_frames[11] + 10
    assert GOOD["init_segment_alone"].n == 0 and GOOD["mdhd_duration_beats_mehd"].track_id == 0x01020304
    assert FX.demux(GOOD["mehd_sidx_styp"].data)["duration"] == 123456789012 and FX.demux(GOOD["mdhd_duration_beats_mehd"].data)["duration"] == 1234
    assert {(f["channels"], f["bits"]) for f in (FX.demux(GOOD[f"flac_{c}ch_{b}bit"].data)["flac"] for c in range(1, 9) for b in (8, 16, 24))} == \
        {(c, b) for c in range(1, 9) for b in (8, 16, 24)}


@pytest.mark.parametrize("name", sorted(FC.limit_edges()))
def test_a_sample_of_the_limit_is_served_and_one_byte_more_is_refused(name):
    m, limit = FC.limit_edges()[name]
    model = FX.demux(m.data)
    assert m.sizes == [5, limit, limit + 1, 7]
    assert model["rows"] == [(m.offsets[0], 5), (m.offsets[1], limit), None, (m.offsets[3], 7)]
    assert (model["samples_available"], model["samples_refused"], model["first_bad_sample"]) == (2, 1, 2)


@pytest.mark.parametrize("name", sorted(CAPS))
def test_capacities_count_what_they_do_not_expand(name):
    m, run_capacity, packet_capacity = CAPS[name]
    model = FX.demux(m.data, 3, packet_capacity, run_capacity)
    FC.check_against_record(model, m, packet_capacity, run_capacity)
    in_runs = sum(r[3] for r in m.runs[:run_capacity])
    assert len(model["run_rows"]) == min(run_capacity, len(m.runs)) and len(model["rows"]) == min(packet_capacity, in_runs)


@pytest.mark.parametrize("name", sorted(BAD))
def test_a_malformed_file_is_refused_where_it_is_wrong(name):
    data, status, at, codecs = BAD[name]
    model = FX.demux(data, codecs)
    assert (model["status"], model["error_offset"]) == (status, at)
    assert all(model[k] == 0 for k in FX.RESULT_FIELDS if k not in ("status", "error_offset", "codec", "first_bad_sample")) and model["rows"] == []


def test_every_status_is_named():
    assert {status for _, status, _, _ in BAD.values()} == set(range(1, 7))


def test_a_prefix_serves_its_whole_fragments():
    m = GOOD["two_truns_with_data_offset"]
    whole_first = FX.demux(m.data[:m.segment_ends[0]])
    assert whole_first["status"] == FX.OK and whole_first["samples"] == m.n // 2 and whole_first["samples_refused"] == 0
    into_second_mdat = FX.demux(m.data[:m.segment_ends[1] - 10])         # the moof is whole, its data is not: the tail is refused
    assert into_second_mdat["samples"] == m.n and 0 < into_second_mdat["samples_refused"] and into_second_mdat["samples_available"] >= m.n // 2
    into_second_moof = FX.demux(m.data[:m.find("moof", 1)[2] - 1])
    assert into_second_moof["samples"] == m.n // 2


def test_the_damage_set_keeps_a_quarter_and_refuses_a_quarter():
    statuses = [FX.demux(data)["status"] for data in FC.damaged(400)]
    assert statuses.count(FX.OK) >= 100 and sum(1 for s in statuses if s != FX.OK) >= 100
