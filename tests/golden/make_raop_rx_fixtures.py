"""Writes tests/golden/raop_rx_textbook.json: what tests/test_raop_rx_textbook.py holds tests/raop_rx_textbook.py to, and through it
the library.  Every expectation below is written by hand from the reference's text, none is taken from the model or the library:

  resend_suite   the nineteen cases of SuiteRaopResend (OpenHome/Av/Tests/TestRaop.cpp:375-1108, Repairer<5>), restated as data: the
                 (seq, resend) inputs in order, ["timer", ranges] where the test fires the timer and the `a->b` ranges it expects there
                 ([] where it expects nothing), ["drop"] where it calls DropAudio, ["throws", seq, resend, which] where it expects
                 RepairerBufferFull ("full") or RepairerStreamRestarted ("restarted"), and the frames it expects at the audio supply,
                 in order.  A case is cut into a new batch at every timer, drop and throw.
  datagrams      hand-assembled datagrams of each kind and every refusal, with the fields a parse must give.
  sessions       short sessions for the flush window, a foreign ssrc, start and resume, sync packets on both sides of the 441-sample
                 threshold and a resend response whose RTP version and type are 0: dispositions, events and the state they leave.

Run from the repository root: python tests/golden/make_raop_rx_fixtures.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import raop_rx_cases as RC  # noqa: E402
import raop_rx_textbook as RX  # noqa: E402


def i(seq, resend=False):
    return ["in", seq, int(resend)]


def t(*ranges):
    return ["timer", [list(r) for r in ranges]]


SUITE = [
    ("TestNoDropouts", [i(0), i(1), i(2)], [0, 1, 2]),
    ("TestResendOnePacket", [i(0), i(2), t((1, 1)), i(1, True), i(3), t()], [0, 1, 2, 3]),
    ("TestResendMultiplePackets", [i(0), i(3), t((1, 2)), i(1, True), i(2, True), i(4)], [0, 1, 2, 3, 4]),
    ("TestResendMulitpleRanges", [i(0), i(3), i(4), i(6), t((1, 2), (5, 5)), i(1, True), i(2, True), i(5)], [0, 1, 2, 3, 4, 5, 6]),
    ("TestResendBeyondMultipleRangeLimit", [i(0), i(2), i(4), i(6), t((1, 1), (3, 3)), i(1, True), i(3, True), t((5, 5)), i(5, True)], [0, 1, 2, 3, 4, 5, 6]),
    ("TestMultipleResendRecover", [i(0), i(3), i(5), t((1, 2), (4, 4)), i(1, True), i(6), t((2, 2), (4, 4)), i(2, True), i(7), i(4, True), t(), i(8), i(9), i(11), i(12),
                                   t((10, 10)), i(13), i(14), i(10, True)], list(range(15))),
    ("TestResendRequest", [i(0), i(2), t((1, 1)), i(3), t((1, 1)), i(1, True)], [0, 1, 2, 3]),
    ("TestResendPacketBufferOverflowFirst", [i(0), i(3), t((1, 2)), i(4), i(5), i(6), i(7), i(8), ["throws", 2, 1, "full"]], [0]),
    ("TestResendPacketBufferOverflowMiddle", [i(0), i(2), t((1, 1)), i(4), t((1, 1), (3, 3)), i(5), i(6), i(7), i(8), ["throws", 3, 1, "full"]], [0]),
    ("TestResendPacketBufferOverflowLast", [i(0), i(2), t((1, 1)), i(3), i(4), i(5), i(6), i(7), ["throws", 8, 0, "full"]], [0]),
    ("TestResendBufferOverflowRecover", [i(0), i(2), t((1, 1)), i(3), i(4), i(5), i(6), i(7), ["throws", 8, 0, "full"], i(9), i(10)], [0, 9, 10]),
    ("TestResendPacketsOutOfOrder", [i(0), i(2), t((1, 1)), i(4), t((1, 1), (3, 3)), i(3, True), i(1, True)], [0, 1, 2, 3, 4]),
    ("TestDropPacketWhileAwaitingResend", [i(0), i(2), t((1, 1)), i(3), i(4), i(6), i(1, True), i(7), t((5, 5)), i(5, True)], [0, 1, 2, 3, 4, 5, 6, 7]),
    ("TestResendPacketsAlreadySeen", [i(0), i(2), t((1, 1)), i(4), t((1, 1), (3, 3)), t((1, 1), (3, 3)), i(3, True), i(1, True), i(3, True), i(5)], [0, 1, 2, 3, 4, 5]),
    ("TestStreamReset", [i(0), i(1), ["throws", 0, 0, "restarted"], i(1), i(2)], [0, 1, 1, 2]),
    ("TestStreamResetResendPending", [i(0), i(2), t((1, 1)), ["throws", 0, 0, "restarted"], i(1), i(2)], [0, 1, 2]),
    ("TestDropAudio", [i(0), i(2), t((1, 1)), ["drop"]], [0]),
    ("TestSequenceNumberWrapping", [i(65535), i(0)], [65535, 0]),
    ("TestSequenceNumberWrappingDuringRepair", [i(65533), i(65535), t((65534, 65534)), i(0), i(65534)], [65533, 65534, 65535, 0]),
]
assert len(SUITE) == 19

OK, TRUNCATED, OVERSIZE, OTHER_TYPE = range(4)
# (name, port, hex, the fields a parse gives -- what is not named is 0)
DATAGRAMS = [
    ("audio", 0, "80e0 1234 00000160 cafef00d a1a2a3", dict(status=OK, marker=1, type=0x60, seq=0x1234, timestamp=0x160, ssrc=0xcafef00d, payload_offset=12, payload_bytes=3)),
    ("audio, extension, no payload", 0, "9060 ffff ffffffff 00000001", dict(status=OK, extension=1, type=0x60, seq=0xffff, timestamp=0xffffffff, ssrc=1, payload_offset=12)),
    ("audio, version 0 and type 0 are not judged", 0, "0000 0002 00000003 00000004 aa", dict(status=OK, seq=2, timestamp=3, ssrc=4, payload_offset=12, payload_bytes=1)),
    ("audio of 11 bytes", 0, "8060 0001 00000160 cafef0", dict(status=TRUNCATED)),
    ("audio of 3 bytes", 0, "8060 00", dict(status=TRUNCATED)),
    ("nothing", 0, "", dict(status=TRUNCATED)),
    ("nothing on the control port", 1, "", dict(status=TRUNCATED)),
    ("sync", 1, "90d4 0007 0000d000 83aa7e80 00001000 0000fb11", dict(status=OK, marker=1, extension=1, type=0x54, seq=7, sync=[0xd000, 0x83aa7e80, 0x1000, 0xfb11])),
    ("sync of 19 bytes", 1, "80d4 0007 0000d000 83aa7e80 00001000 0000fb", dict(status=TRUNCATED)),
    ("resend response", 1, "80d6 0001 80e0 0101 00000200 cafef00d b1b2", dict(status=OK, resend=1, marker=1, type=0x60, seq=0x101, timestamp=0x200, ssrc=0xcafef00d, payload_offset=16,
                                                                              payload_bytes=2)),
    ("resend response, inner version and type 0", 1, "80d6 0001 0000 0101 00000200 cafef00d b1", dict(status=OK, resend=1, seq=0x101, timestamp=0x200, ssrc=0xcafef00d, payload_offset=16,
                                                                                                      payload_bytes=1)),
    ("resend response, inner header cut", 1, "80d6 0001 80e0 01", dict(status=TRUNCATED)),
    ("resend response, inner audio header cut", 1, "80d6 0001 80e0 0101 00000200 cafef0", dict(status=TRUNCATED)),
    ("resend response with nothing inside", 1, "80d6 0001", dict(status=TRUNCATED)),
    ("a resend request on the control port", 1, "80d5 0001 0005 0002", dict(status=OTHER_TYPE, type=0x55)),
    ("type 0 on the control port", 1, "8000 0001 00000000 00000000", dict(status=OTHER_TYPE)),
    ("a sync packet on the audio port is audio", 0, "80d4 0007 0000d000 83aa7e80 00001000 0000fb11", dict(status=OK, marker=1, type=0x54, seq=7, timestamp=0xd000, ssrc=0x83aa7e80,
                                                                                                           payload_offset=12, payload_bytes=8)),
    ("1472 bytes", 0, "8060 0001 00000160 cafef00d" + "00" * 1460, dict(status=OK, type=0x60, seq=1, timestamp=0x160, ssrc=0xcafef00d, payload_offset=12, payload_bytes=1460)),
    ("1473 bytes", 0, "8060 0001 00000160 cafef00d" + "00" * 1461, dict(status=OVERSIZE)),
    ("1473 bytes on the control port", 1, "80d4 0001 00000160 cafef00d" + "00" * 1461, dict(status=OVERSIZE)),
]

OUTPUT, DUPLICATE, PENDING, DROPPED, FLUSHED, WRONG_SESSION, SYNC, IGNORED, NOT_REACHED = range(1, 10)
NEW, DELAY = 1, 2
A, R, S = RC.A, RC.R, RC.S
# (name, max_frames, state_in (what is not named is 0), datagrams, dispositions, events, state_out (the fields named))
SESSIONS = [
    ("start: the first packet names the session and takes the control port's latency",
     5, {}, [S(1000, 11025), A(7), A(8)], [SYNC, OUTPUT, OUTPUT], [0, NEW | DELAY, 0],
     dict(started=1, running=1, frame=8, session_id=RC.SSRC, latency=11025, control_latency=11025)),
    ("a sync packet 440 samples off changes nothing, one 441 off is a delay on the next frame out",
     5, RC.running_state(10, latency=11025), [S(0, 11025 + 440), A(11), S(0, 11025 - 441 + 440), A(12), S(0, 11025 + 440 + 441), A(13), A(14)],
     [SYNC, OUTPUT, SYNC, OUTPUT, SYNC, OUTPUT, OUTPUT], [0, 0, 0, 0, 0, DELAY, 0], dict(latency=11025 + 881, control_latency=11025 + 881, frame=14)),
    ("a foreign ssrc is dropped and the stream goes on",
     5, RC.running_state(10), [A(11), A(12, ssrc=5), A(12), R(13, ssrc=5), A(13)], [OUTPUT, WRONG_SESSION, OUTPUT, WRONG_SESSION, OUTPUT], [0] * 5, dict(frame=13, session_id=RC.SSRC)),
    ("the flush window: seq and timestamp both inside it while a resume is pending",
     5, dict(RC.running_state(0), running=0, resume_pending=1, flush_seq=41, flush_time=1000),
     [A(40, timestamp=900), R(41, timestamp=1000), A(41, timestamp=1001), A(40, timestamp=2000), A(42, timestamp=1002)],
     [FLUSHED, FLUSHED, OUTPUT, DROPPED, NOT_REACHED], [0, 0, NEW, 0, 0], dict(frame=41, running=0, resume_pending=1, flush_seq=0, flush_time=0, started=1)),
    ("resume: a new stream and no delay, the session is kept, and a packet of another session starts the stream all the same",
     5, dict(RC.running_state(500, latency=11025), running=0, resume_pending=1), [A(9, ssrc=77), A(10), A(11)], [WRONG_SESSION, OUTPUT, OUTPUT], [NEW, 0, 0],
     dict(frame=11, running=1, resume_pending=0, session_id=RC.SSRC, latency=11025)),
    ("a resend response whose RTP version and type are 0 repairs the stream",
     5, RC.running_state(20), [A(22), R(21, version=0, ptype=0), A(23)], [OUTPUT, OUTPUT, OUTPUT], [0, 0, 0], dict(frame=23)),
    ("a restart outside a repair stops the stream: resume pending, what follows is not reached",
     5, RC.running_state(20), [A(21), A(21), A(22)], [OUTPUT, DROPPED, NOT_REACHED], [0, 0, 0], dict(frame=21, running=0, resume_pending=1, started=1)),
]


def main():
    suite = [dict(name=name, max_frames=5, steps=steps, outputs=outputs) for name, steps, outputs in SUITE]
    grams = [dict(name=name, port=port, hex=hexes.replace(" ", ""), want=want) for name, port, hexes, want in DATAGRAMS]
    sessions = [dict(name=name, max_frames=mf, state_in=dict(RX.new_state(), **state), datagrams=[dict(port=p, hex=g.hex()) for g, p in gs], dispositions=disp, events=ev,
                     state_out=out) for name, mf, state, gs, disp, ev, out in SESSIONS]
    with open(RC.GOLDEN, "w") as f:
        json.dump(dict(resend_suite=suite, datagrams=grams, sessions=sessions), f, indent=1)
        f.write("\n")
    print(RC.GOLDEN, os.path.getsize(RC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
