"""Holds the Songcast receiver's model (tests/ohm_rx_textbook.py) against what there is to hold it against.

The parse has a checker: the oracle's ohp_ohm_audio_parse (oracle/ohp_songcast.h), field by field, over datagrams made by
tests/ohm_textbook.audio_frame -- codec lengths 0..29, every flag, audio lengths 0 and 5760 -- and the oracle's OHP_ERR_ASSERT cases
map to statuses other than OK.

The sequencer has none (PARITY UNPINNED: the reference has no test of ProtocolOhBase, and does not compile here).  It is held to
invariants that follow from the reference's text: a loss-free reordering within the repair window, with resent duplicates, comes out
once and in order with no event and nothing waiting; a gap beyond the window resets; a past frame that is no resend resets inside a
repair and stops the stream outside one; the resend request on three cases worked by hand; the replay of the waiting frames at the
head of the next batch changes nothing.  The committed sessions' dispositions are compared with a table written by hand."""
import pytest

import ohm_rx_cases as RC
import ohm_rx_textbook as RX
import ohm_textbook as OT
import oracle_lib as O

LETTER = {RX.OUTPUT: "O", RX.DUPLICATE: "D", RX.PENDING: "P", RX.DROPPED_BY_RESET: "R", RX.STALE: "S", RX.NOT_REACHED: "N", RX.IGNORED: "I"}
RUNNING = dict(RX.new_state(), running=1, frame=9, stream_msg_due=0, last_sample_start=(9 + 0x200) * 220, bit_depth=16, sample_rate=44100, channels=2, latency=4410)


def letters(recs):
    return "".join(LETTER[r["disposition"]] for r in recs)


def grams_of(frames, resent=(), **more):
    return [RC.audio_gram(f & 0xffffffff, bytes([k & 0xff, 1, 2, 3]), flags=OT.FLAG_LOSSLESS | (OT.FLAG_RESENT if k in resent else 0), **more) for k, f in enumerate(frames)]


# ---------------------------------------------------------------- the parse against the oracle
def same_as_oracle(gram):
    err, ref = O.ohm_audio_parse(gram)
    got = RX.parse(gram)
    if err != 0:
        assert got["status"] != RX.OK, gram[:64].hex()
        return got["status"]
    if len(gram) > 8 + ref.msg_bytes:
        # the one place where the model is stricter than the oracle: bytes behind the header's total.  The oracle reads the message out
        # of the front of the buffer; the receiver's table says how long the datagram WAS, and a total that disagrees is TRUNCATED.
        assert got["status"] == RX.TRUNCATED and same_as_oracle(gram[:8 + ref.msg_bytes]) == RX.OK
        return RX.TRUNCATED
    assert got["status"] == RX.OK
    flags = got["flags"]
    assert (ref.halt, ref.lossless, ref.timestamped, ref.resent, ref.timestamped2) == tuple(int(bool(flags & b)) for b in (1, 2, 4, 8, 16))
    for k in ("samples", "frame", "network_timestamp", "media_latency", "media_timestamp", "sample_start", "samples_total", "sample_rate", "bit_rate",
              "volume_offset", "bit_depth", "channels", "codec_bytes", "audio_offset", "audio_bytes", "msg_type"):
        assert getattr(ref, k) == got[k], k
    assert bytes(ref.codec[:ref.codec_bytes]) == got["codec"] and ref.msg_bytes == len(gram) - 8
    return RX.OK


def test_the_parse_equals_the_oracles_field_by_field():
    rng = RC.Lcg(5)
    for codec in range(30):
        for flags in range(16):
            for n in (0, 5760) if flags in (0, 15) or codec in (0, 29) else (0,):
                sh = OT.stream_header(rng.next() << 20 | rng.next(), 44100 + codec, rng.next(), rng.below(600) - 300, 8 * (1 + codec % 3), 1 + flags % 2, b"C" * codec)
                gram = OT.audio_frame(flags, rng.below(1 << 16), rng.next() << 8 | flags, rng.next(), rng.next(), rng.next() << 24 | rng.next(), sh, rng.bytes(8) * (n // 8),
                                      media_timestamp=rng.next())
                assert len(gram) == 58 + codec + n and same_as_oracle(gram) == RX.OK
                assert RX.parse(gram)["flags"] == flags | (16 if flags & 4 else 0)


def test_where_the_oracle_asserts_the_model_reports_a_status():
    good = RC.audio_gram(3, bytes(range(40)), codec=b"abc")
    big = RC.audio_gram(4, bytes(5760), codec=b"x" * 29)
    retotal = lambda g, n: g[:6] + n.to_bytes(2, "big") + g[8:]
    cases = [(b"", RX.TRUNCATED), (good[:7], RX.TRUNCATED), (b"Ohx " + good[4:], RX.NOT_OHM), (good[:4] + b"\2" + good[5:], RX.NOT_OHM),
             (good[:5] + b"\10" + good[6:], RX.NOT_OHM), (good[:5] + b"\xfe" + good[6:], RX.NOT_OHM), (good[:-1], RX.TRUNCATED), (good + b"\0", RX.TRUNCATED),
             (retotal(good, 7)[:7], RX.TRUNCATED), (RC.other_gram(4, b"track"), RX.NOT_AUDIO), (RC.other_gram(255, b"blob"), RX.NOT_AUDIO), (RC.other_gram(0), RX.NOT_AUDIO),
             (retotal(good[:40], 40), RX.TRUNCATED), (good[:8] + b"\x31" + good[9:], RX.BAD_HEADER), (good[:56] + b"\1" + good[57:], RX.BAD_HEADER),
             (good[:57] + b"\x1e" + good[58:], RX.BAD_HEADER), (retotal(good[:60], 60), RX.TRUNCATED), (retotal(big + b"\0", len(big) + 1), RX.OVERSIZE)]
    for gram, status in cases:
        assert RX.parse(gram)["status"] == status, gram[:60].hex()
        assert same_as_oracle(gram) == status
    assert same_as_oracle(good) == RX.OK and same_as_oracle(big) == RX.OK
    assert RX.parse(RC.other_gram(4, b"track"))["msg_type"] == 4 and RX.parse(b"Ohx " + good[4:])["msg_type"] == 0


# ---------------------------------------------------------------- the sequencer's invariants
@pytest.mark.parametrize("first", [0, 5, 0xffffff00, 0xfffffffe])
@pytest.mark.parametrize("seed", range(6))
def test_a_loss_free_reordering_within_the_window_comes_out_once_in_order(first, seed):
    rng = RC.Lcg(1000 * seed + first % 977)
    n = 2 + rng.below(399)
    frames = [(first + k) & 0xffffffff for k in range(n)]
    arrival = RC.window_shuffle(frames, rng, reach=(1, 2, 5, 50, 199, 199)[seed])
    assert arrival[0] == frames[0] and sorted(arrival, key=frames.index) == frames
    assert max(abs(arrival.index(f) - k) for k, f in enumerate(frames)) <= 199
    grams, tags = [], []
    for f in arrival:
        grams.append(RC.audio_gram(f, f.to_bytes(4, "big")))
        tags.append(f)
        if rng.below(10) == 0:                                            # a resent copy, at once or a little later
            grams.append(RC.audio_gram(f, b"copy", flags=OT.FLAG_LOSSLESS | OT.FLAG_RESENT))
            tags.append(None)
    recs, res, out = RX.receive(RX.new_state(), grams)
    assert out == b"".join(f.to_bytes(4, "big") for f in frames)          # every frame once, in order
    assert [r["events"] for r in recs if r["disposition"] == RX.OUTPUT][1:] == [0] * (n - 1) and recs[0]["events"] == RX.NEW_STREAM | RX.DELAY
    assert res["n_pending"] == 0 and res["resend"] == [] and res["stop_reason"] == RX.STOP_NONE and res["n_output"] == n
    assert res["state_out"]["frame"] == frames[-1] and res["state_out"]["running"] == 1
    assert all(r["disposition"] == (RX.OUTPUT if t is not None else RX.DUPLICATE) for r, t in zip(recs, tags))
    assert sorted(r["order"] for r in recs if r["disposition"] == RX.OUTPUT) == list(range(n))


@pytest.mark.parametrize("gap", [201, 202, 1000, 0x7fffffff])
def test_a_gap_beyond_the_window_resets_and_the_next_frame_starts_a_stream(gap):
    """inside a repair the frame beyond the window is the one that resets; outside one it BEGINS a repair (RepairBegin has no distance
    test) and the next frame beyond the window resets: either way the resetting frame and the waiting ones are dropped"""
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 12, 10 + gap, 11 + gap, 12 + gap]))
    assert letters(recs) == "ORROO" and recs[3]["events"] == RX.NEW_STREAM and recs[4]["events"] == 0
    assert res["state_out"]["frame"] == (12 + gap) & 0xffffffff and res["n_pending"] == 0
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 10 + gap, 11, 11 + gap, 12 + gap]))
    assert letters(recs) == "ORORO" and recs[4]["events"] == RX.NEW_STREAM
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 12, 210]))              # 200 ahead is still inside
    assert letters(recs) == "OPP" and res["n_pending"] == 2


def test_a_frame_begun_far_ahead_is_reached_or_waits():
    recs, res, out = RX.receive(RUNNING, grams_of([10 + 300] + list(range(10, 10 + 300))))
    assert letters(recs) == "O" * 301 and recs[0]["order"] == 300 and res["state_out"]["frame"] == 310
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 500, 11, 13]))
    assert letters(recs) == "OPOP" and [recs[1]["order"], recs[3]["order"]] == [0, 1]      # the far frame is replayed first
    assert res["resend"] == list(range(12, 13)) + list(range(14, 33))


def test_a_past_frame_that_is_no_resend_resets_in_a_repair_and_stops_outside_one():
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 12, 7, 13, 14]))
    assert letters(recs) == "ORROO" and res["stop_reason"] == RX.STOP_NONE and recs[3]["events"] == RX.NEW_STREAM
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 12, 7, 13, 14], resent={2}))
    assert letters(recs) == "OPDPP"
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 11, 7, 12, 13]))
    assert letters(recs) == "OOSNN" and res["stop_reason"] == RX.STOP_STALE
    assert res["state_out"] == dict(RUNNING, running=0, stream_msg_due=1, frame=11, last_sample_start=(11 + 0x200) * 220)
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 11, 11, 10, 12], resent={2, 3}))
    assert letters(recs) == "OODDO" and res["stop_reason"] == RX.STOP_NONE
    recs, res, _ = RX.receive(RUNNING, grams_of([10, 12, 9, 11], resent={2}) + [RC.audio_gram(13, b"halt", flags=OT.FLAG_HALT)] + grams_of([14]))
    assert letters(recs) == "OODOON" and res["stop_reason"] == RX.STOP_HALT


def test_a_halt_frame_stops_the_stream_once_it_is_output_and_drops_what_waits():
    grams = grams_of([10, 12]) + [RC.audio_gram(13, b"halt", flags=OT.FLAG_HALT)] + grams_of([15, 11, 14])
    recs, res, out = RX.receive(RUNNING, grams)
    assert letters(recs) == "OOORON" and recs[2]["events"] == RX.HALT and res["stop_reason"] == RX.STOP_HALT
    assert [r["order"] for r in recs] == [0, 2, 3, 0, 1, 0] and res["state_out"]["running"] == 0 and res["state_out"]["stream_msg_due"] == 1
    assert res["state_out"]["frame"] == 13 and res["resend"] == [] and res["n_pending"] == 0


def test_the_resend_request_by_hand():
    _, res, _ = RX.receive(RUNNING, grams_of([10, 13, 17, 15]))
    assert res["resend"] == [11, 12, 14, 16]
    _, res, _ = RX.receive(RUNNING, grams_of([10, 40, 12]))
    assert res["resend"] == [11] + list(range(13, 32))                    # twenty, the first of them
    # across the wrap: iFrame = 0xfffffffd, frames 0xffffffff and 2 wait.  Gap one is [0xfffffffe, 0xffffffff): one number.  Gap two is
    # `for (i = 0; i < 2; i++)` -- start = 0xffffffff + 1 wraps to 0 --: 0 and 1.
    _, res, _ = RX.receive(RX.new_state(), grams_of([0xfffffffd, 0xffffffff, 2]))
    assert res["resend"] == [0xfffffffe, 0, 1]
    # ... and iFrame = 0xfffffffe, frame 1 waits: `for (i = 0xffffffff; i < 1; i++)` runs not at all (kept from the reference)
    _, res, _ = RX.receive(RX.new_state(), grams_of([0xfffffffe, 1]))
    assert res["resend"] == [] and res["n_pending"] == 1
    assert RX.resend_datagram([11, 12]) == b"Ohm \x01\x07\x00\x14" + b"\0\0\0\2" + b"\0\0\0\x0b\0\0\0\x0c"


def replayed(state, grams, cut):
    """the batch cut at `cut`: the first part, then its PENDING datagrams in replay order in front of the rest"""
    recs1, res1, out1 = RX.receive(state, grams[:cut])
    waiting = sorted((k for k, r in enumerate(recs1) if r["disposition"] == RX.PENDING), key=lambda k: recs1[k]["order"])
    assert len(waiting) == res1["n_pending"]
    if res1["stop_reason"]:
        return None                             # (a stopped receiver drops what is queued and waits for a restart: nothing to replay)
    recs2, res2, out2 = RX.receive(res1["state_out"], [grams[k] for k in waiting] + grams[cut:])
    final = [(r["disposition"], r["events"]) for r in recs1] + [(r["disposition"], r["events"]) for r in recs2[len(waiting):]]
    for k, r in zip(waiting, recs2):
        final[k] = (r["disposition"], r["events"])
    return final, out1 + out2, res2


@pytest.mark.parametrize("seed", range(8))
def test_replaying_the_waiting_frames_in_front_of_the_next_batch_changes_nothing(seed):
    rng = RC.Lcg(300 + seed)
    first = (0, 5, 0xffffff00, 0xfffffffe)[seed % 4]
    frames = RC.window_shuffle([(first + k) & 0xffffffff for k in range(60 + rng.below(60))], rng, reach=(3, 20, 199)[seed % 3])
    if seed >= 4:
        frames.insert(10, (first + 700) & 0xffffffff)                     # a repair that begins far ahead, and the reset that follows it
        frames.insert(30, (first + 701) & 0xffffffff)
    grams = []
    for f in frames:
        grams.append(RC.audio_gram(f, f.to_bytes(4, "big"), latency=4410 if f % 16 else 8820))
        if rng.below(8) == 0:
            grams.append(RC.audio_gram(f, b"copy", flags=OT.FLAG_LOSSLESS | OT.FLAG_RESENT))
    recs, res, out = RX.receive(RX.new_state(), grams)
    whole = [(r["disposition"], r["events"]) for r in recs]
    for cut in range(len(grams) + 1):
        again = replayed(RX.new_state(), grams, cut)
        if again is None:
            assert res["stop_reason"] != RX.STOP_NONE
            continue
        final, out_cut, res_cut = again
        assert final == whole and out_cut == out, cut
        assert (res_cut["state_out"], res_cut["resend"], res_cut["n_pending"]) == (res["state_out"], res["resend"], res["n_pending"]), cut


# ---------------------------------------------------------------- the committed sessions
BY_HAND = {
    "in_order": "OOOOOO", "reorder": "OOOOOO", "duplicate": "OODODODD", "resend_pending": "OPPP", "gap_reset": "ORROO", "far_begin": "OROORO",
    "stale_stop": "OOSNN", "stale_in_repair": "ORROO", "halt_stop": "OOOON", "halt_in_a_run": "ORRON", "format_change": "OOOO", "latency_change": "OOO", "wrap": "OOOOOP",
    "mixed_types": "OIIIIIIIIIIOIO",
}
EVENTS_BY_HAND = {"in_order": [3, 0, 0, 0, 0, 0], "gap_reset": [0, 0, 0, 1, 0], "far_begin": [0, 0, 0, 0, 0, 1], "halt_stop": [0, 0, 4, 0, 0], "halt_in_a_run": [0, 0, 0, 4, 0],
                  "format_change": [0, 1, 0, 1], "latency_change": [0, 2, 3], "wrap": [3, 0, 0, 0, 0, 0]}


def test_the_committed_sessions_are_the_models_and_their_dispositions_the_hand_tables():
    sessions = RC.load_sessions()
    assert sorted(s["name"] for s in sessions) == sorted(BY_HAND) and len(sessions) >= 12
    for s in sessions:
        grams = [bytes.fromhex(g) for g in s["datagrams"]]
        recs, res, out = RX.receive(s["state_in"], grams)
        assert [[r["status"], r["disposition"], r["events"], r["order"]] for r in recs] == s["records"], s["name"]
        want = s["result"]
        assert (res["state_out"], res["n_output"], res["n_pending"], res["stop_reason"], res["resend"], out.hex()) == \
            (want["state_out"], want["n_output"], want["n_pending"], want["stop_reason"], want["resend"], want["out"]), s["name"]
        assert letters(recs) == BY_HAND[s["name"]], s["name"]
        if s["name"] in EVENTS_BY_HAND:
            assert [r["events"] for r in recs] == EVENTS_BY_HAND[s["name"]], s["name"]
    by = {s["name"]: s["result"] for s in sessions}
    assert by["resend_pending"]["resend"] == [11, 12, 14, 16] and by["wrap"]["resend"] == [3, 4]
    assert by["stale_stop"]["stop_reason"] == RX.STOP_STALE and by["halt_stop"]["stop_reason"] == RX.STOP_HALT
