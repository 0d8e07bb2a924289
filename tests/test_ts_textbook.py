"""The model of the transport stream demultiplexer and the ADTS frame table (tests/ts_textbook.py) held to fixed facts, and the tests'
own muxer (tests/ts_cases.py) held to the model: known checksums, the fixtures under tests/golden/ts, streams that demux to exactly the
elementary bytes they were muxed from, ADTS chains that return the offsets the frames were written at.  No GPU."""
import gzip
import json
import os

import ts_cases as TC
import ts_textbook as TX

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ts")
PAT_SECTION = bytes.fromhex("00b00d0001c100000001f000")       # one program, number 1, on PID 0x1000: the PAT every common muxer writes


def test_the_checksum_of_the_check_string():
    assert TX.crc(b"123456789") == 0x0376E6E7


def test_the_checksum_of_the_common_pat():
    assert TX.crc(PAT_SECTION) == 0x2AB104B2
    assert TX.crc(PAT_SECTION + bytes.fromhex("2ab104b2")) == 0
    assert TC.pat() == PAT_SECTION + bytes.fromhex("2ab104b2")
    assert TX.pat_pid(b"\x00" + TC.pat() + b"\xff" * 50) == 0x1000


def test_the_muxed_streams_demux_to_what_they_were_muxed_from():
    rng = TC.Lcg(1)
    for sizes in (None, [20, 0, 1, 184, 3], [14], [15, 1]):
        audio, es = TC.audio_run(rng, n_pes=5, sizes=sizes)
        other = TC.carry(TC.OTHER_PID, TC.pes(rng.bytes(400), stream_id=0xE0))
        mixed = TC.head_packets() + [p for pair in zip(audio, other * len(audio)) for p in pair]
        m = TX.demux(b"".join(mixed))
        assert m["status"] == TX.OK and m["run"] == es and len(m["pes"]) == 5 and m["dropped_bytes"] == 0 and m["cc_jumps"] == 0
        assert [r["pts"] for r in m["pes"]] == [90000 * k + 7 for k in range(5)] and m["pes_open_bytes"] == 0
        assert sum(r["bytes"] for r in m["pes"]) == len(es) and [r["flags"] for r in m["pes"]] == [0] * 5


def test_a_stream_cut_in_two_ticks_gives_the_same_run():
    rng = TC.Lcg(2)
    audio, es = TC.audio_run(rng, n_pes=4, es_bytes=(900, 333))
    packets = TC.head_packets() + audio
    for cut in range(3, len(packets)):
        a = TX.demux(b"".join(packets[:cut]))
        b = TX.demux(b"".join(packets[cut:]), flags=TX.PES_OPEN if a["pes_open_bytes"] else 0, pmt_pid=a["pmt_pid"], audio_pid=a["audio_pid"], pes_open_bytes=a["pes_open_bytes"])
        assert a["run"] + b["run"] == es, cut


def test_the_named_streams_say_what_their_names_say():
    named = TC.named()
    m = {name: TX.demux(s["data"], s["flags"], s["pmt_pid"], s["audio_pid"], s["pes_open_bytes"]) for name, s in named.items()}
    assert {x["status"] for x in m.values()} == set(range(5))
    assert [m[f"packets_{n}"]["packets"] for n in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)] == [0, 1, 2, 3, 63, 64, 65, 255, 256, 257]
    assert (m["bytes_187"]["packets"], m["bytes_187"]["trailing_bytes"], m["bytes_188_187"]["packets"], m["bytes_188_187"]["trailing_bytes"]) == (0, 187, 1, 187)
    data = named["every_payload_length"]["data"]
    lengths = {(188 - 5 - data[k + 4] if data[k + 3] & 0x20 else 184) for k in range(0, len(data), 188)}
    assert lengths == set(range(185))
    assert m["corrupt"]["status"] == TX.CORRUPT and m["corrupt"]["corrupt_packet"] == 2 + len(TC.audio_run(TC.Lcg(0), n_pes=2)[0]) and len(m["corrupt"]["pes"]) == 2
    assert m["corrupt_before_pat"]["pat_packet"] == TX.NONE and m["corrupt_skipped"]["status"] == TX.OK and m["corrupt_skipped"]["tei_packets"] == 1
    assert m["program_zero_first"]["pmt_pid"] == TC.PMT_PID and m["bad_crc_then_good"]["pat_packet"] == 2 and m["bad_crc_then_good"]["pmt_packet"] == 3
    assert m["rich_pmt"]["audio_pid"] == TC.AUDIO_PID and m["pmt_without_audio"]["status"] == TX.NO_AUDIO and m["pmt_without_audio"]["run"] == b""
    assert m["pmt_before_pat"]["audio_pid"] == TC.AUDIO_PID and m["pmt_before_pat"]["pmt_packet"] == 2
    assert m["audio_before_pmt"]["dropped_bytes"] == 0 and len(m["audio_before_pmt"]["pes"]) == 2
    assert m["section_ends_with_packet"]["pmt_packet"] == 1 and m["section_one_byte_over"]["pmt_packet"] == 2
    for name, x in m.items():
        if name.startswith("break_pat"):
            assert (x["pat_packet"], x["pmt_packet"], x["status"]) == (1, 2, TX.OK), name
        if name.startswith("break_pmt"):
            assert (x["pat_packet"], x["pmt_packet"], x["status"]) == (0, 2, TX.OK), name
    assert m["audio_pid_given"]["pat_packet"] == TX.NONE and len(m["audio_pid_given"]["pes"]) == 3
    assert m["pmt_pid_given"]["pat_packet"] == TX.NONE and m["pmt_pid_given"]["pmt_packet"] == 1
    assert (m["no_pat"]["status"], m["no_pmt"]["status"]) == (TX.NO_PAT, TX.NO_PMT)
    assert [r["pts"] for r in m["header_lengths"]["pes"]] == [TX.NO_PTS, 12345678, 0x1FFFFFFFF, TX.NO_PTS]
    assert m["header_fills_packet"]["pes"][0]["bytes"] == 204 and m["header_fills_packet"]["pes"][0]["es_offset"] == 0
    assert m["header_one_byte_too_long"]["bad_pes_starts"] == 1 and m["header_one_byte_too_long"]["dropped_bytes"] == 368
    assert [r["stream_id"] for r in m["stream_ids"]["pes"]] == [0xC0, 0xDF] and m["stream_ids"]["bad_pes_starts"] == 2
    assert m["bad_marker_and_prefix"]["bad_pes_starts"] == 4 and len(m["bad_marker_and_prefix"]["pes"]) == 1
    assert m["length_zero"]["pes_open_bytes"] == TX.UNBOUNDED
    assert m["length_short_before_start"]["pes"][0]["flags"] == TX.EXCESS and m["length_short_at_end"]["pes"][0]["bytes"] == 250
    assert m["length_beyond_before_start"]["pes"][0]["flags"] == TX.TRUNCATED and m["length_beyond_at_end"]["pes_open_bytes"] == 500
    assert m["before_first_start_dropped"]["dropped_bytes"] == 284 and len(m["before_first_start_dropped"]["pes"]) == 1
    assert [(r["flags"], r["bytes"]) for r in m["before_first_start_open"]["pes"]] == [(TX.CONTINUATION, 284), (0, 300)]
    assert m["before_first_start_open_more"]["pes"][0]["flags"] == TX.CONTINUATION | TX.TRUNCATED
    assert [(r["flags"], r["bytes"]) for r in m["before_first_start_open_less"]["pes"]] == [(TX.CONTINUATION | TX.EXCESS, 200), (0, 300)]
    assert m["open_and_no_start"]["pes_open_bytes"] == 5000 - 284 and m["open_and_no_audio"]["pes_open_bytes"] == 77 and len(m["open_and_a_start_first"]["pes"]) == 1
    assert m["counter_jumps"]["cc_jumps"] == 3 and [r["flags"] for r in m["counter_jumps"]["pes"]] == [TX.CC_JUMP, TX.CC_JUMP, 0]
    assert (m["skipped_kinds"]["bad_sync"], m["skipped_kinds"]["tei_packets"], m["skipped_kinds"]["scrambled_packets"]) == (1, 1, 1)
    assert m["skipped_kinds"]["run"] == named["skipped_kinds"]["es"] and m["skipped_kinds"]["cc_jumps"] == 0
    assert m["start_without_payload"]["bad_pes_starts"] == 1


def test_the_adts_chain_returns_the_offsets_the_frames_were_written_at():
    rng = TC.Lcg(3)
    sizes = [0, 5, 200, 1, 8182, 0, 33]
    frames = [TC.adts_frame(TC.clean(rng.bytes(n)), protection_absent=bool(k % 2)) for k, n in enumerate(sizes)]
    junk = TC.clean(rng.bytes(25))
    data = frames[0] + frames[1] + junk + b"".join(frames[2:5]) + junk[:3] + frames[5] + frames[6] + frames[0][:6]
    m = TX.adts_chain(data)
    want, at = [], 0
    for k, f in enumerate(frames):
        at += len(junk) if k == 2 else (3 if k == 5 else 0)
        want.append((at, len(f), 7 if k % 2 else 9))
        at += len(f)
    assert [(f["offset"], f["bytes"], f["header_bytes"]) for f in m["frames"]] == want
    assert [f["flags"] for f in m["frames"]] == [0, 0, 1, 0, 0, 1, 0] and m["interruptions"] == 2 and m["skipped_bytes"] == 28 and m["bytes_consumed"] == at


def test_the_named_adts_streams_say_what_their_names_say():
    named = TC.adts_named()
    m = {name: TX.adts_chain(s["data"], s["flags"]) for name, s in named.items()}
    assert [(f["bytes"], f["header_bytes"]) for f in m["seven_and_nine"]["frames"]] == [(7, 7), (9, 9), (8, 7)]
    assert m["largest"]["frames"][0]["bytes"] == 8191
    assert len(m["ends_with_last_byte"]["frames"]) == 3 and len(m["one_byte_short"]["frames"]) == 2
    assert m["one_byte_short"]["bytes_consumed"] == m["ends_with_last_byte"]["frames"][2]["offset"]
    assert m["six_left_over"]["bytes_consumed"] == len(named["six_left_over"]["data"]) - 6 and m["six_left_over"]["skipped_bytes"] == 0
    assert len(m["junk_between"]["frames"]) == 4 and m["junk_between"]["interruptions"] == 2
    assert m["nothing_valid"]["frames"] == [] and m["nothing_valid"]["bytes_consumed"] == 3000 - 6
    for name, x in m.items():
        if name.startswith("start_at_"):
            assert x["frames"][0]["offset"] == int(name[9:]) and x["frames"][0]["flags"] == TX.INTERRUPTED and len(x["frames"]) == 2, name
        if name.startswith("chained_to_"):
            assert x["frames"][1]["offset"] == int(name[11:]) and x["skipped_bytes"] == 0, name
    assert m["recognise_four_then_five"]["first_frame_offset"] > 500 and m["recognise_four_then_five"]["mean_payload_bytes"] == 52
    assert m["recognise_at_1001"]["first_frame_offset"] == 1001 and m["recognise_at_1002"]["status"] == TX.NOT_ADTS
    assert m["recognise_nothing"]["status"] == TX.NOT_ADTS and m["recognise_fifth_lacks_ten"]["status"] == TX.NOT_ADTS
    assert m["recognise_fifth_has_ten"]["status"] == TX.ADTS_OK and len(m["recognise_fifth_has_ten"]["frames"]) == 4
    assert (m["recognise_at_0"]["profile"], m["recognise_at_0"]["sf_index"], m["recognise_at_0"]["channel_config"]) == (2, 3, 1)


def test_the_id3v2_tags_at_the_head():
    tag = b"ID3\x04\x00\x00" + bytes([0, 0, 1, 5]) + bytes(133)
    footed = b"ID3\x04\x00\x10" + bytes([0, 0, 0, 20]) + bytes(20) + b"3DI\x04\x00\x10" + bytes([0, 0, 0, 20])
    assert TX.id3v2_skip(tag + b"\xff\xf1") == 143 and TX.id3v2_skip(footed + b"\xff\xf1") == 40 and TX.id3v2_skip(tag + footed + tag[:9]) == 183
    assert TX.id3v2_skip(b"ID3\xff\x00\x00" + bytes(30)) == 0 and TX.id3v2_skip(b"ID3\x04\x00\x00\x00\x00\x80\x00" + bytes(30)) == 0 and TX.id3v2_skip(b"ID3") == 0


def test_the_fixtures():
    """tests/golden/ts: the streams tools/make_ts_fixtures.py wrote, and what the model said of them then."""
    with open(os.path.join(GOLDEN, "streams.json")) as f:
        index = json.load(f)
    assert index["crc_123456789"] == 0x0376E6E7 and bytes.fromhex(index["pat_section"]) == PAT_SECTION
    for name, rec in index["streams"].items():
        with gzip.open(os.path.join(GOLDEN, name + ".ts.gz"), "rb") as f:
            data = f.read()
        m = TX.demux(data)
        assert (m["status"], m["packets"], m["audio_pid"], len(m["pes"]), len(m["run"]), TC.fnv1a32(m["run"])) == \
            (rec["status"], rec["packets"], rec["audio_pid"], rec["pes_packets"], rec["bytes_delivered"], rec["run_fnv1a32"]), name
        a = TX.adts_chain(m["run"], TX.RECOGNISE)
        assert (a["status"], len(a["frames"]), a["bytes_consumed"]) == (rec["adts_status"], rec["adts_frames"], rec["adts_bytes_consumed"]), name
