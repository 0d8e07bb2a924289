"""tests/raop_rx_textbook.py -- the independent model of the RAOP receiver -- held to tests/golden/raop_rx_textbook.json,
whose expectations are written by hand from the reference's text (tests/golden/make_raop_rx_fixtures.py): the nineteen cases of the
reference's SuiteRaopResend cut into batches at every timer, drop and throw (so they pin the state hand-over and the replay too), the
hand-assembled datagrams, the short sessions.  Then fixed-seed lossy sessions cut at random places into several batches against the same
session in one batch, and the generator's own coverage."""
import pytest

import raop_rx_cases as RC
import raop_rx_textbook as RX

GOLD = RC.load_golden()
REASON = {"full": RX.STOP_BUFFER_FULL, "restarted": RX.STOP_RESTARTED}


def test_the_fixture_is_what_its_generator_writes(tmp_path, monkeypatch):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("make_raop_rx_fixtures", RC.GOLDEN.replace("raop_rx_textbook.json", "make_raop_rx_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(RC, "GOLDEN", str(tmp_path / "again.json"))
    mod.main()
    with open(tmp_path / "again.json") as f:
        assert json.load(f) == GOLD
    assert len(GOLD["resend_suite"]) == 19


@pytest.mark.parametrize("case", GOLD["resend_suite"], ids=lambda c: c["name"])
def test_the_reference_suite(case):
    batches = RC.suite_batches(case)
    played = RC.play(batches, case["max_frames"])
    outputs = []
    for (grams, what), (todo, recs, res) in zip(batches, played):
        outputs += [RX.parse(*todo[index])["seq"] for index, _, _ in res["rows"]]
        if what[0] == "timer":
            assert [list(r) for r in res["ranges"]] == what[1], case["name"]
            assert res["stop_reason"] == RX.STOP_NONE
        elif what[0] == "throws":
            assert res["stop_reason"] == REASON[what[1]] and res["n_pending"] == 0 and recs[-1]["disposition"] == RX.DROPPED_BY_RESET
            assert res["state_out"]["running"] == 0 and res["state_out"]["resume_pending"] == 1
        else:
            assert res["stop_reason"] == RX.STOP_NONE
    assert outputs == case["outputs"]
    assert played[-1][2]["n_pending"] == 0                   # (TestDropAudio's waiting frame: the drop is the caller's, RC.play forgets it)


@pytest.mark.parametrize("gram", GOLD["datagrams"], ids=lambda g: g["name"])
def test_the_hand_assembled_datagrams(gram):
    r = RX.parse(bytes.fromhex(gram["hex"]), gram["port"])
    want = {**dict.fromkeys(RX.RECORD_FIELDS, 0), "sync": [0, 0, 0, 0], "port": gram["port"], **gram["want"]}
    assert {k: r[k] for k in RX.RECORD_FIELDS} == want


@pytest.mark.parametrize("session", GOLD["sessions"], ids=lambda s: s["name"][:40])
def test_the_sessions(session):
    recs, res = RX.run_stream(session["state_in"], session["max_frames"], RC.golden_grams(session))
    assert [r["disposition"] for r in recs] == session["dispositions"]
    assert [r["events"] for r in recs] == session["events"]
    assert {k: res["state_out"][k] for k in session["state_out"]} == session["state_out"]


def test_the_quirks_of_the_ranges_at_the_wrap():
    def ranges(frame, waiting, max_frames=50):
        _, res = RX.run_stream(RC.running_state(frame), max_frames, [RC.A(s) for s in waiting])
        assert res["n_pending"] == len(waiting)
        return res["ranges"]

    assert ranges(65533, [65535]) == [(65534, 65534)]                    # the one the reference's suite pins
    assert ranges(65534, [0]) == [(65535, 0xffffffff)]                   # first - 1 of a first waiting frame 0, stored in a TUint
    assert ranges(65534, [1]) == [(65535, 0)]                            # a first gap across the wrap: end < start
    assert ranges(65530, [65532, 65534, 2]) == [(65531, 65531), (65533, 65533)]      # the gap 65535, 0, 1 straddles the wrap: never asked for
    assert ranges(65530, [65532, 65535, 1]) == [(65531, 65531), (65533, 65534), (0, 0)]
    assert ranges(65530, [65532, 0]) == [(65531, 65531)]                              # 0 - 65533 > 0 fails: 65533 .. 65535 are never asked for
    assert ranges(10, [12, 14, 16, 18], max_frames=5) == [(11, 11), (13, 13)]         # kMaxMissedRanges = 5 / 2
    assert ranges(10, [12, 14], max_frames=1 + 1) == [(11, 11)]
    assert ranges(10, [12], max_frames=1) == [(11, 11)]                               # (the deviation: the reference has no slot)


def outcome(batches_played):
    """what a listener sees of a session: the output datagrams in order with their events, and where the stream stands"""
    heard = []
    for todo, recs, res in batches_played:
        heard += [(todo[index][0], recs[index]["events"]) for index, _, _ in res["rows"]]
    last = batches_played[-1][2]
    return heard, last["state_out"], last["stop_reason"], [batches_played[-1][0][i][0] for i in last["pending"]]


@pytest.mark.parametrize("seed", RC.LOSSY_SEEDS[:12])
def test_a_session_cut_into_batches_is_the_session_in_one_batch(seed):
    grams = RC.lossy_session(seed)
    max_frames = 5 if seed % 4 else 50
    whole = RC.play([(grams, ("end",))], max_frames)
    rng = RC.Lcg(1000 + seed)
    for _ in range(4):
        cuts = sorted({rng.below(len(grams) + 1) for _ in range(1 + rng.below(6))})
        parts = [grams[a:b] for a, b in zip([0] + cuts, cuts + [len(grams)])]
        played, state, carried, stopped = [], RX.new_state(), [], False
        for part in parts:                                   # (RC.play, but a stream that stopped runs no further batch, as in one batch)
            if stopped:
                break
            todo = carried + part
            recs, res = RX.run_stream(state, max_frames, todo)
            played.append((todo, recs, res))
            state, carried, stopped = res["state_out"], [todo[i] for i in res["pending"]], res["stop_reason"] != RX.STOP_NONE
        assert outcome(played) == outcome(whole), cuts


def test_the_generators_cover_what_they_are_there_for():
    seen = set()
    for s in RC.lossy_streams():
        _, res = RX.run_stream(s["state"], s["max_frames"], s["grams"])
        seen.update(res["trace"])
    assert seen >= set(RC.COVERAGE), sorted(set(RC.COVERAGE) - seen)
    shapes = set()
    for s in RC.shape_streams():
        _, res = RX.run_stream(s["state"], s["max_frames"], s["grams"])
        shapes.update(res["trace"])
        shapes.add(("stop", res["stop_reason"], s["max_frames"]))
    assert shapes >= set(RC.COVERAGE) - {"wrap inside a repair"}, sorted(set(RC.COVERAGE) - shapes)
    assert shapes >= {("stop", RX.STOP_BUFFER_FULL, m) for m in (1, 5, 50, 63)}
