"""The receiving end of RAOP from the reference's text, independent of the library: the parse is struct.unpack; the flow is
ProtocolRaop::ProcessPacket / ShouldFlush / ProcessStreamStartOrResume / OutputAudio and RaopControlServer::Run
(Av/Raop/ProtocolRaop.cpp) as plain `if` chains; the repairer is Repairer<MaxFrames>::OutputAudio / Repair / RepairReset /
TimerRepairExpired (Av/Raop/ProtocolRaop.h:530-789) kept as the reference keeps it -- a first waiting frame and a Python list behind it,
every branch of Repair() in its place -- and not as the library's one sorted set.  TUint16 / TInt16 arithmetic is written out: u16()
truncates, i16() is the assignment to a TInt16, and what the reference computes in `int` is computed in Python integers.
It calls neither the library nor anything compiled.  TEST INFRASTRUCTURE ONLY.

Statuses, in the order the checks are made (the first that fails names the status):
  OVERSIZE    more than 1472 bytes
  TRUNCATED   fewer than 4 bytes
  audio port:    TRUNCATED  fewer than 8 bytes behind the 4
  control port:  type (byte 1 & 0x7f) 0x54: TRUNCATED with fewer than 16 bytes behind the 4
                 type 0x56: TRUNCATED when the inner datagram has fewer than 4 bytes, or fewer than 8 behind them
                 any other type: OTHER_TYPE

Quirks of TimerRepairExpired that follow from its text (and are kept):
  - the first range is (u16(frame + 1), first - 1) with `first - 1` an int stored in a TUint: first == 0 gives 0xffffffff; a first gap
    that straddles the wrap has end < start;
  - a later gap is listed only if end - start > 0 as ints, start = u16(previous + 1): a gap that straddles the wrap is never listed;
  - the first range is made whatever kMaxMissedRanges is.  (With max_frames 1 the reference's FIFO has no slot and asserts: the model,
    like the library, makes the first range.)
"""
import struct

OK, TRUNCATED, OVERSIZE, OTHER_TYPE = range(4)
OUTPUT, DUPLICATE, PENDING, DROPPED_BY_RESET, FLUSHED, WRONG_SESSION, SYNC, IGNORED, NOT_REACHED = range(1, 10)
NEW_STREAM, DELAY = 1, 2
STOP_NONE, STOP_BUFFER_FULL, STOP_RESTARTED = 0, 1, 2
AUDIO, CONTROL = 0, 1
MAX_PACKET_BYTES, MIN_DELAY_CHANGE = 1472, 441
STATE_FIELDS = ("flush_seq", "flush_time", "session_id", "latency", "control_latency", "frame", "running", "started", "resume_pending")
RECORD_FIELDS = ("status", "resend", "marker", "extension", "type", "port", "seq", "payload_offset", "payload_bytes", "timestamp", "ssrc", "sync")


def u16(x):
    return x & 0xffff


def i16(x):
    x &= 0xffff
    return x - 0x10000 if x >= 0x8000 else x


def new_state():
    """ProtocolRaop's, RaopControlServer's and the Repairer's members as Reset() and the constructors leave them"""
    return dict.fromkeys(STATE_FIELDS, 0)


def parse(gram, port):
    gram = bytes(gram)
    r = dict(status=OK, resend=0, marker=0, extension=0, type=0, port=port, seq=0, payload_offset=0, payload_bytes=0, timestamp=0, ssrc=0, sync=[0, 0, 0, 0], kind=None)

    def fail(status):
        r["status"] = status
        return r

    def rtp(at):
        b0, b1, seq = struct.unpack_from(">BBH", gram, at)
        return (b0 >> 4) & 1, b1 >> 7, b1 & 0x7f, seq

    def audio(at):
        if len(gram) - at < 4:
            return fail(TRUNCATED)
        if len(gram) - at - 4 < 8:
            return fail(TRUNCATED)
        r["extension"], r["marker"], r["type"], r["seq"] = rtp(at)
        r["timestamp"], r["ssrc"] = struct.unpack_from(">II", gram, at + 4)
        r["payload_offset"] = at + 12
        r["payload_bytes"] = len(gram) - at - 12
        r["kind"] = "audio"
        return r

    if len(gram) > MAX_PACKET_BYTES:
        return fail(OVERSIZE)
    if len(gram) < 4:
        return fail(TRUNCATED)
    if port == AUDIO:
        return audio(0)
    kind = gram[1] & 0x7f
    if kind == 0x54:
        if len(gram) - 4 < 16:
            return fail(TRUNCATED)
        r["extension"], r["marker"], r["type"], r["seq"] = rtp(0)
        r["sync"] = list(struct.unpack_from(">IIII", gram, 4))
        r["kind"] = "sync"
        return r
    if kind == 0x56:
        audio(4)
        if r["status"] == OK:
            r["resend"] = 1
        return r
    r["type"] = kind
    return fail(OTHER_TYPE)


class Stop(Exception):
    def __init__(self, reason):
        self.reason = reason


class Receiver:
    """One stream.  `recs` grows by a record per datagram; a waiting frame is its record."""

    def __init__(self, state, max_frames):
        self.st = dict(state)
        self.max_frames = max_frames
        self.first = None            # iRepairFirst
        self.frames = []             # iRepairFrames
        self.repairing = False
        self.output = []             # records in output order
        self.trace = []              # which branch each datagram took: what the tests' generators assert their coverage with

    # ---- Repairer
    def _out(self, r):
        # ProtocolRaop::OutputAudio's delay rule, in front of every frame that goes out
        st = self.st
        if st["control_latency"] != st["latency"]:
            diff = st["control_latency"] - st["latency"] if st["control_latency"] > st["latency"] else st["latency"] - st["control_latency"]
            if diff >= MIN_DELAY_CHANGE:
                st["latency"] = st["control_latency"]
                r["events"] |= DELAY
        r["disposition"] = OUTPUT
        r["order"] = len(self.output)
        self.output.append(r)

    def repair_reset(self):
        for r in ([self.first] if self.first is not None else []) + self.frames:
            r["disposition"] = DROPPED_BY_RESET
            r["order"] = 0
        self.first, self.frames = None, []
        self.st["running"] = 0
        self.repairing = False

    def _repair(self, r):
        st = self.st
        frame = u16(r["seq"])
        diff = i16(frame - st["frame"])
        if diff < 1:
            if not r["resend"]:
                self.trace.append("restart in a repair")
                self.repair_reset()
                r["disposition"] = DROPPED_BY_RESET
                raise Stop(STOP_RESTARTED)
            self.trace.append("duplicate of the past in a repair")
            r["disposition"] = DUPLICATE
            return True
        if diff == 1:
            st["frame"] = u16(st["frame"] + 1)
            self._out(r)
            while u16(self.first["seq"]) == u16(st["frame"] + 1):
                st["frame"] = u16(st["frame"] + 1)
                if st["frame"] == 0:
                    self.trace.append("wrap inside a repair")
                self._out(self.first)
                if len(self.frames) == 0:
                    self.first = None
                    return False
                self.first = self.frames.pop(0)
            return True
        diff = i16(frame - u16(self.first["seq"]))
        if diff == 0:
            self.trace.append("duplicate of the first")
            r["disposition"] = DUPLICATE
            return True
        if diff < 0:
            if len(self.frames) == self.max_frames:
                self.trace.append("full at the first")
                self.repair_reset()
                r["disposition"] = DROPPED_BY_RESET
                raise Stop(STOP_BUFFER_FULL)
            self.frames.insert(0, self.first)
            self.first = r
            return True
        if len(self.frames) == 0:
            self.frames.insert(0, r)
            return True
        diff = i16(frame - u16(self.frames[-1]["seq"]))
        if diff == 0:
            self.trace.append("duplicate of the last")
            r["disposition"] = DUPLICATE
            return True
        if diff > 0:
            if len(self.frames) == self.max_frames:
                self.trace.append("full at the last")
                self.repair_reset()
                r["disposition"] = DROPPED_BY_RESET
                raise Stop(STOP_BUFFER_FULL)
            self.frames.append(r)
            return True
        count = len(self.frames)
        for at, it in enumerate(self.frames):
            diff = i16(frame - u16(it["seq"]))
            if diff > 0:
                continue
            if diff == 0:
                self.trace.append("duplicate of a middle one")
                r["disposition"] = DUPLICATE
            else:
                if count == self.max_frames:
                    self.trace.append("full in the middle")
                    self.repair_reset()
                    r["disposition"] = DROPPED_BY_RESET
                    raise Stop(STOP_BUFFER_FULL)
                self.frames.insert(at, r)
            break
        return True

    def _repairer(self, r):
        st = self.st
        r["disposition"] = PENDING
        pushed = False
        if not st["running"]:
            st["frame"] = u16(r["seq"])
            st["running"] = 1
            self._out(r)
            pushed = True
        if self.repairing:
            before = len(self.output)
            self.repairing = self._repair(r)
            pushed = pushed or len(self.output) != before
        if not self.repairing and not pushed:
            diff = i16(u16(r["seq"]) - st["frame"])
            if diff == 1:
                st["frame"] = u16(st["frame"] + 1)
                self._out(r)
            elif diff < 1:
                if not r["resend"]:
                    self.trace.append("restart outside a repair")
                    st["running"] = 0
                    r["disposition"] = DROPPED_BY_RESET
                    raise Stop(STOP_RESTARTED)
                self.trace.append("duplicate of the past outside a repair")
                r["disposition"] = DUPLICATE
            else:
                self.first = r
                self.repairing = True

    # ---- ProtocolRaop and RaopControlServer
    def _should_flush(self, r):
        st = self.st
        return bool(st["resume_pending"]) and r["seq"] <= st["flush_seq"] and r["timestamp"] <= st["flush_time"]

    def take(self, r):
        """r: a parsed record with disposition, events, order still to be set"""
        st = self.st
        r.update(disposition=IGNORED, events=0, order=0)
        if r["status"] != OK:
            return
        if r["kind"] == "sync":
            st["control_latency"] = (r["sync"][3] - r["sync"][0]) & 0xffffffff
            r["disposition"] = SYNC
            return
        if self._should_flush(r):
            r["disposition"] = FLUSHED
            return
        if not st["started"] or st["resume_pending"]:
            if st["session_id"] == 0:
                st["session_id"] = r["ssrc"]
            r["events"] |= NEW_STREAM
            if not st["started"]:
                st["latency"] = st["control_latency"]
                r["events"] |= DELAY
            st["started"] = 1
            st["resume_pending"] = 0
            st["flush_seq"] = st["flush_time"] = 0
        if st["session_id"] != r["ssrc"] or self._should_flush(r):
            r["disposition"] = WRONG_SESSION
            return
        self._repairer(r)

    def ranges(self):
        """TimerRepairExpired's list as it would be made now: [(start, end)] as ResendRange holds them (TUint)"""
        if not self.repairing:
            return []
        kmax = self.max_frames // 2
        start = u16(self.st["frame"] + 1)
        end = u16(self.first["seq"])
        out = [(start, (end - 1) & 0xffffffff)]
        count = 1
        i = 0
        while count < kmax and i < len(self.frames):
            start = u16(end + 1)
            end = u16(self.frames[i]["seq"])
            if end - start > 0:
                out.append((start, (end - 1) & 0xffffffff))
                count += 1
                if count == kmax:
                    break
            i += 1
        return out


def run_stream(state, max_frames, grams):
    """grams: [(bytes, port)] in arrival order -> (records, result).  result: state_out, n_output, n_pending, stop_reason, ranges,
    rows [(datagram index, payload_offset, payload_bytes)] in output order, pending [datagram index] in replay order."""
    rx = Receiver(state, max_frames)
    recs = [parse(g, port) for g, port in grams]
    for k, r in enumerate(recs):
        r["index"] = k
    stop = STOP_NONE
    for k, r in enumerate(recs):
        try:
            rx.take(r)
        except Stop as s:
            stop = s.reason
            rx.st["running"] = 0          # RepairReset (the restart outside a repair clears iRunning alone: the same state)
            rx.st["resume_pending"] = 1   # OutputDiscontinuity
            for later in recs[k + 1:]:
                later.update(disposition=NOT_REACHED, events=0, order=0)
            break
    ranges = rx.ranges()
    waiting = ([rx.first] if rx.first is not None else []) + rx.frames
    for place, r in enumerate(waiting):
        r["order"] = place
    result = dict(state_out=dict(rx.st), n_output=len(rx.output), n_pending=len(waiting), stop_reason=stop, ranges=ranges,
                  rows=[(r["index"], r["payload_offset"], r["payload_bytes"]) for r in rx.output], pending=[r["index"] for r in waiting], trace=rx.trace)
    return recs, result


def drop_audio(state):
    """Repairer::DropAudio between two batches: the caller forgets the PENDING datagrams, and RepairReset clears iRunning"""
    out = dict(state)
    out["running"] = 0
    return out


def resend_request(seq_start, count):
    """RaopPacketResendRequest::Write: the 8 bytes that go to the sender's control port"""
    return struct.pack(">BBHHH", 0x80, 0x80 | 0x55, 1, seq_start & 0xffff, count & 0xffff)
