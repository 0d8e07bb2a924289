"""Writes tests/golden/ohm_rx_textbook.json: a dozen small scripted Songcast sessions -- the datagrams in arrival order, the state the
receiver starts from -- and what tests/ohm_rx_textbook.py makes of them: per datagram (status, disposition, events, order), per
session the stop reason, the resend request, the state to carry on and the gathered bytes.  tests/test_ohm_rx_textbook.py checks the
dispositions of every session against a table written by hand, so the file records the model's reading, it does not define it.

    python tests/golden/make_ohm_rx_fixtures.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ohm_rx_cases as RC          # noqa: E402
import ohm_rx_textbook as RX       # noqa: E402
import ohm_textbook as OT          # noqa: E402

RESENT, HALT, LOSSLESS = OT.FLAG_RESENT, OT.FLAG_HALT, OT.FLAG_LOSSLESS


def script(name, steps, state=None, note=""):
    """steps: (frame, flags) or (frame, flags, dict of audio_gram's other arguments) or raw bytes"""
    rng = RC.Lcg(sum(name.encode()))
    grams = []
    for k, step in enumerate(steps):
        if isinstance(step, bytes):
            grams.append(step)
            continue
        frame, flags, more = (step + ({},))[:3]
        grams.append(RC.audio_gram(frame & 0xffffffff, rng.bytes(more.pop("bytes", 8 + 4 * (k % 3))), flags=LOSSLESS | flags, **more))
    state = dict(state or RX.new_state())
    recs, res, out = RX.receive(state, grams)
    return dict(name=name, note=note, state_in=state, datagrams=[g.hex() for g in grams],
                records=[[r["status"], r["disposition"], r["events"], r["order"]] for r in recs],
                result=dict(state_out=res["state_out"], n_output=res["n_output"], n_pending=res["n_pending"], stop_reason=res["stop_reason"],
                            resend=res["resend"], out=out.hex()))


def sessions():
    running = dict(RX.new_state(), running=1, frame=9, stream_msg_due=0, last_sample_start=(9 + 0x200) * 220, bit_depth=16, sample_rate=44100, channels=2, latency=4410)
    bad = RC.audio_gram(3, b"\1\2\3\4")
    return [
        script("in_order", [(f, 0) for f in range(5, 11)], note="a new receiver: the first frame starts the stream"),
        script("reorder", [(10, 0), (12, 0), (14, 0), (11, 0), (13, 0), (15, 0)], state=running, note="two waiting frames drained by the missing ones"),
        script("duplicate", [(10, 0), (12, 0), (12, 0), (13, 0), (13, RESENT), (11, 0), (11, RESENT), (12, RESENT)], state=running,
               note="a second copy of a waiting frame, and resent copies of frames already output"),
        script("resend_pending", [(10, 0), (13, 0), (17, 0), (15, RESENT)], state=running, note="ends in a repair: 11, 12, 14, 16 are asked for"),
        script("gap_reset", [(10, 0), (12, 0), (213, 0), (214, 0), (215, 0)], state=running, note="213 is 203 ahead of 10: reset; 214 starts a stream"),
        script("far_begin", [(10, 0), (400, 0), (11, 0), (12, 0), (401, 0), (402, 0)], state=running,
               note="a repair may BEGIN any distance ahead (RepairBegin has no test): 400 waits, 401 resets, 402 starts a stream"),
        script("stale_stop", [(10, 0), (11, 0), (7, 0), (12, 0), (13, 0)], state=running, note="a past frame that is no resend, outside a repair: ReaderError"),
        script("stale_in_repair", [(10, 0), (12, 0), (7, 0), (13, 0), (14, 0)], state=running, note="the same inside a repair: RepairReset, the stream goes on"),
        script("halt_stop", [(10, 0), (12, 0), (13, HALT), (11, 0), (14, 0)], state=running, note="the halt frame stops the stream once it has been output"),
        script("halt_in_a_run", [(10, 0), (12, 0), (13, 0), (11, HALT), (14, 0)], state=running,
               note="the halt frame is the missing one: the frames that waited right behind it are dropped with the rest"),
        script("format_change", [(10, 0), (11, 0, dict(depth=24, bytes=12)), (12, 0, dict(depth=24, bytes=12)), (13, 0, dict(depth=24, bytes=12, sample_start=5))],
               state=running, note="a depth change, then a sample start that runs backwards"),
        script("latency_change", [(10, 0), (11, 0, dict(latency=8820)), (12, 0, dict(latency=8820, rate=48000))], state=running,
               note="a latency change is a delay; a rate change a new stream and a delay"),
        script("wrap", [(0xfffffffe, 0), (0, 0), (2, 0), (0xffffffff, 0), (1, 0), (5, 0)], note="frame numbers through 2^32; the request across the wrap"),
        script("mixed_types", [(10, 0), RC.other_gram(4, b"track"), b"Ohm", b"Ohx " + bad[4:], RC.other_gram(9), RC.other_gram(255, b"blob"),
                               bad[:8] + b"\x31" + bad[9:], bad[:56] + b"\1" + bad[57:], bad[:-1], bad + b"\0", bad[:40], (11, 0),
                               RC.other_gram(7, b"\0\0\0\0"), (12, 0)], state=running, note="every other type and every bad status between three frames"),
    ]


if __name__ == "__main__":
    with open(os.path.join(HERE, "ohm_rx_textbook.json"), "w") as f:
        json.dump(dict(sessions=sessions()), f, indent=1)
        f.write("\n")
