"""The receiving end of Songcast from the wire's definition and the reference's text, independent of the library: the parse is
struct.unpack over the field table of tests/ohm_textbook.py's docstring; the sequencer is ProtocolOhBase's Process(OhmMsgAudio&) /
Repair / RepairReset / OutputAudio / TimerRepairExpired (Av/Songcast/ProtocolOhBase.cpp:254-553) kept as a Python `set` of waiting
frame numbers with `min()` -- neither the library's window bitmap nor the reference's first-plus-sorted-vector; the gather is slicing.
It calls neither the oracle nor the library.  TEST INFRASTRUCTURE ONLY.

The sequencer is PARITY UNPINNED in the reference (no test of ProtocolOhBase exists there): tests/test_ohm_rx_textbook.py holds this
model to invariants instead, and to the oracle's parse.

What is NOT modelled, because it cannot happen: the three "backlog is full" resets of Repair (:345, :373, :393).  A frame waits only
while 1 < frame - iFrame, and every frame but the one a repair began on arrived with frame - iFrame <= 200, so at most 199 + 1 frames
wait, against room for 1 + 200.

Statuses, in the order the checks are made (the first that fails names the status):
  TRUNCATED   fewer than 8 bytes
  NOT_OHM     magic, major version, or a type above 7 that is not 255 (OhmHeader::Internalise throws OhmError)
  TRUNCATED   the header's total is not the datagram's size
  NOT_AUDIO   a type other than 3
  TRUNCATED   fewer than 58 bytes
  BAD_HEADER  audio header length != 50, reserved != 0, codec name over 29 bytes
  TRUNCATED   total below 58 + codec bytes
  OVERSIZE    more than 5760 audio bytes
"""
import struct

OK, NOT_OHM, NOT_AUDIO, TRUNCATED, BAD_HEADER, OVERSIZE = range(6)
OUTPUT, DUPLICATE, PENDING, DROPPED_BY_RESET, STALE, NOT_REACHED, IGNORED = range(1, 8)
NEW_STREAM, DELAY, HALT = 1, 2, 4
STOP_NONE, STOP_STALE, STOP_HALT = 0, 1, 2
FLAG_HALT, FLAG_RESENT = 1, 8
MAX_BACKLOG, MAX_MISSED = 200, 20
MASK = 0xffffffff

HEADER_FIELDS = ("flags", "samples", "frame", "network_timestamp", "media_latency", "media_timestamp", "sample_start", "samples_total",
                 "sample_rate", "bit_rate", "volume_offset", "bit_depth", "channels", "codec_bytes")


def new_state():
    """ProtocolOhBase's members as its constructor and Stream() leave them"""
    return dict(running=0, frame=0, stream_msg_due=1, last_sample_start=0xffffffff, bit_depth=0, sample_rate=0, channels=0, latency=0)


def parse(gram):
    """-> dict(status, msg_type, and for OK every header field, codec, audio_offset, audio_bytes)"""
    gram = bytes(gram)
    r = dict(status=OK, msg_type=0, codec=b"", audio_offset=0, audio_bytes=0, **{k: 0 for k in HEADER_FIELDS})

    def fail(status):
        r["status"] = status
        return r

    if len(gram) < 8:
        return fail(TRUNCATED)
    magic, major, kind, total = struct.unpack_from(">4sBBH", gram, 0)
    if magic != b"Ohm " or major != 1 or (kind > 7 and kind != 255):
        return fail(NOT_OHM)
    if total != len(gram):
        return fail(TRUNCATED)
    r["msg_type"] = kind
    if kind != 3:
        return fail(NOT_AUDIO)
    if len(gram) < 58:
        return fail(TRUNCATED)
    (hlen, flags, samples, frame, nts, latency, mts, start, total_samples, rate, bit_rate, volume, depth, channels, reserved,
     codec_bytes) = struct.unpack_from(">BBHIIIIQQIIhBBBB", gram, 8)
    if hlen != 50 or reserved != 0 or codec_bytes > 29:
        return fail(BAD_HEADER)
    if total < 58 + codec_bytes:
        return fail(TRUNCATED)
    if total - 58 - codec_bytes > 5760:
        return fail(OVERSIZE)
    r.update(flags=flags, samples=samples, frame=frame, network_timestamp=nts, media_latency=latency, media_timestamp=mts, sample_start=start,
             samples_total=total_samples, sample_rate=rate, bit_rate=bit_rate, volume_offset=volume, bit_depth=depth, channels=channels,
             codec_bytes=codec_bytes, codec=gram[58:58 + codec_bytes], audio_offset=58 + codec_bytes, audio_bytes=total - 58 - codec_bytes)
    return r


def sdiff(a, b):
    """TInt diff = a - b on TUint operands"""
    d = (a - b) & MASK
    return d - (1 << 32) if d >= 1 << 31 else d


class Receiver:
    """One stream's ProtocolOhBase over parsed records.  recs[i] gains disposition / events / order / dst_offset."""

    def __init__(self, state, recs, dst_offset):
        self.s, self.recs, self.at, self.n_out = dict(state), recs, dst_offset, 0
        self.waiting = {}                       # frame number -> record index: the set
        self.stop = STOP_NONE

    def output_audio(self, i):
        r, s, ev = self.recs[i], self.s, 0
        if r["sample_start"] < s["last_sample_start"] or s["bit_depth"] != r["bit_depth"] or s["sample_rate"] != r["sample_rate"] or s["channels"] != r["channels"]:
            s["stream_msg_due"] = 1
        s["last_sample_start"] = r["sample_start"]
        if s["stream_msg_due"]:
            ev |= NEW_STREAM
            s["stream_msg_due"], s["bit_depth"], s["channels"] = 0, r["bit_depth"], r["channels"]
        if s["sample_rate"] != r["sample_rate"] or s["latency"] != r["media_latency"]:
            s["sample_rate"], s["latency"] = r["sample_rate"], r["media_latency"]
            ev |= DELAY
        if r["flags"] & FLAG_HALT:
            ev |= HALT
        r.update(disposition=OUTPUT, events=ev, order=self.n_out, dst_offset=self.at)
        self.n_out += 1
        self.at += r["audio_bytes"]
        if ev & HALT:
            self.stop = STOP_HALT               # THROW(OhmDiscontinuity), once it has been output

    def repair_reset(self):
        for i in self.waiting.values():
            self.recs[i]["disposition"] = DROPPED_BY_RESET
        self.waiting = {}
        self.s["running"], self.s["stream_msg_due"] = 0, 1

    def first_waiting(self):
        return min(self.waiting, key=lambda f: sdiff(f, self.s["frame"]))

    def repair(self, i):
        r, s = self.recs[i], self.s
        diff = sdiff(r["frame"], s["frame"])
        if diff < 1:
            if r["flags"] & FLAG_RESENT:
                r["disposition"] = DUPLICATE
            else:
                self.repair_reset()
                r["disposition"] = DROPPED_BY_RESET
            return
        if diff > MAX_BACKLOG:
            self.repair_reset()
            r["disposition"] = DROPPED_BY_RESET
            return
        if diff == 1:
            s["frame"] = (s["frame"] + 1) & MASK
            self.output_audio(i)
            while not self.stop and self.waiting and self.first_waiting() == (s["frame"] + 1) & MASK:
                s["frame"] = (s["frame"] + 1) & MASK
                self.output_audio(self.waiting.pop(s["frame"]))
            return
        if r["frame"] in self.waiting:
            r["disposition"] = DUPLICATE
        else:
            self.waiting[r["frame"]] = i

    def process(self, i):
        r, s = self.recs[i], self.s
        r["disposition"] = PENDING
        if not s["running"]:
            s["frame"], s["running"] = r["frame"], 1
            self.output_audio(i)
        elif self.waiting:
            self.repair(i)
        else:
            diff = sdiff(r["frame"], s["frame"])
            if diff == 1:
                s["frame"] = (s["frame"] + 1) & MASK
                self.output_audio(i)
            elif diff < 1:
                if r["flags"] & FLAG_RESENT:
                    r["disposition"] = DUPLICATE
                else:
                    r["disposition"], self.stop = STALE, STOP_STALE         # THROW(ReaderError)
            else:
                self.waiting[r["frame"]] = i                                # RepairBegin: any distance ahead

    def replay_order(self):
        """the waiting frames in the order that rebuilds the set when they are processed again: a frame more than 200 ahead can only
        BEGIN a repair, so it goes first; the others ascend"""
        order = sorted(self.waiting, key=lambda f: sdiff(f, self.s["frame"]))
        if order and sdiff(order[-1], self.s["frame"]) > MAX_BACKLOG:
            order = order[-1:] + order[:-1]
        return order

    def missed(self):
        """TimerRepairExpired: `for (TUint i = start; i < end; i++)` over every gap below a waiting frame, at most twenty numbers"""
        out, start = [], (self.s["frame"] + 1) & MASK
        for end in sorted(self.waiting, key=lambda f: sdiff(f, self.s["frame"])):
            out += list(range(start, min(end, start + MAX_MISSED)))       # (empty when end < start as unsigned numbers)
            start = (end + 1) & MASK
        return out[:MAX_MISSED]


def sequence(state_in, recs, dst_offset):
    """recs: the stream's parsed records in arrival order (changed in place).  -> the stream's result"""
    rx = Receiver(state_in, recs, dst_offset)
    for r in recs:
        r.update(disposition=IGNORED, events=0, order=0, dst_offset=0)
    for i, r in enumerate(recs):
        if rx.stop:
            r["disposition"] = NOT_REACHED
        elif r["status"] == OK:
            rx.process(i)
    resend, n_pending = [], 0
    if rx.stop:
        rx.repair_reset()                       # WaitForPipelineToEmpty
    else:
        resend = rx.missed()
        for k, f in enumerate(rx.replay_order()):
            recs[rx.waiting[f]].update(disposition=PENDING, order=k)
        n_pending = len(rx.waiting)
    return dict(state_out=rx.s, out_bytes=rx.at - dst_offset, n_output=rx.n_out, n_pending=n_pending, stop_reason=rx.stop, resend=resend)


def receive(state_in, grams, dst_offset=0):
    """One stream, parse to gather: -> (records, result, the stream's output bytes)"""
    recs = [parse(g) for g in grams]
    res = sequence(state_in, recs, dst_offset)
    out = bytearray(res["out_bytes"])
    for r, g in zip(recs, grams):
        if r["disposition"] == OUTPUT:
            at = r["dst_offset"] - dst_offset
            out[at:at + r["audio_bytes"]] = bytes(g)[r["audio_offset"]:r["audio_offset"] + r["audio_bytes"]]
    return recs, res, bytes(out)


def resend_datagram(frames):
    """ProtocolOhBase::RequestResend (:93-110): an Ohm header of type resend, the count, the frame numbers"""
    body = struct.pack(">I", len(frames)) + b"".join(struct.pack(">I", f) for f in frames)
    return b"Ohm " + struct.pack(">BBH", 1, 7, 8 + len(body)) + body
