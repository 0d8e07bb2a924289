"""What the Songcast receiver's tests share: datagram makers over tests/ohm_textbook.py, the committed sessions
(tests/golden/ohm_rx_textbook.json), and the batches -- what the C ABI (or the CPU driver) is given and what the model
(tests/ohm_rx_textbook.py) says must come of it: every record, every stream result, the whole destination arena.
TEST INFRASTRUCTURE ONLY."""
import json
import os
import struct

import numpy as np

import ohm_rx_textbook as RX
import ohm_textbook as OT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ohm_rx_textbook.json")
GUARD, FILL, GAP = 24, 0xA5, 0xEE


class Lcg:
    """a fixed-seed generator that is the same everywhere"""

    def __init__(self, seed):
        self.x = (seed * 2654435761 + 12345) & 0xffffffff

    def next(self):
        self.x = (self.x * 1664525 + 1013904223) & 0xffffffff
        return self.x >> 8

    def below(self, n):
        return self.next() % n

    def bytes(self, n):
        return bytes(self.next() & 0xff for _ in range(n))


def audio_gram(frame, audio, flags=OT.FLAG_LOSSLESS, codec=b"PCM ", rate=44100, depth=16, channels=2, latency=4410, sample_start=None,
               samples_total=0, network_timestamp=0, volume_offset=0, media_timestamp=0):
    """one audio datagram; sample_start defaults to frame * 220 (it ascends with the frame number, across the 2^32 wrap too)"""
    frame_bytes = max(1, channels * depth // 8)
    start = sample_start if sample_start is not None else ((frame + 0x200) & 0xffffffff) * 220
    sh = OT.stream_header(samples_total, rate, rate * depth * channels, volume_offset, depth, channels, codec)
    return OT.audio_frame(flags, len(audio) // frame_bytes, frame, network_timestamp, latency, start, sh, audio, media_timestamp)


def other_gram(kind, body=b""):
    """a message of another type: track 4, metatext 5, join 0, listen 1, leave 2, slave 6, resend 7, audio blob 255"""
    return b"Ohm " + struct.pack(">BBH", 1, kind, 8 + len(body)) + bytes(body)


def stream(grams, state=None, align=None):
    """one stream of a Job: its datagrams in arrival order, the state it starts from (None: a new receiver's), and the source offset
    mod 16 of all its datagrams, or of each (None: the Job's)"""
    return dict(grams=[bytes(g) for g in grams], state=dict(state or RX.new_state()), align=align)


def window_shuffle(frames, rng, reach=199):
    """frames[0] stays; no other frame ends up more than `reach` places from where it was (a sort by index plus a bounded offset)"""
    rest = list(frames[1:])
    keyed = sorted(range(len(rest)), key=lambda i: (i + rng.below(reach + 1), i))
    out = [frames[0]] + [rest[i] for i in keyed]
    assert all(abs(out.index(f) - k) <= reach for k, f in enumerate(frames)) if len(frames) < 64 else True
    return out


def state_row(row, prefix, s):
    for k in ("last_sample_start", "frame", "sample_rate", "latency", "running", "stream_msg_due", "bit_depth", "channels"):
        row[k] = s[k]


class Job:
    """streams: [stream(...)].  The datagrams are laid into the source arena ROUND ROBIN over the streams, datagram number q of the
    arena at the next offset that is `aligns[q % len(aligns)]` mod 16, stray bytes in the gaps and none behind the last (the arena
    is allocated to the byte); the table is by stream, as the ABI wants it.  The destination arena: GUARD bytes, then every stream's
    run -- as long as the table alone says it may get, sum of max(bytes - 58, 0) -- with GUARD + i bytes behind stream i's, all FILL.
    `want`, `want_records`, `want_results`: the model's."""

    def __init__(self, streams, aligns=(0, 4, 8, 12), dst_lead=GUARD):
        from ohpipeline_amd import capi
        self.streams = streams
        src = bytearray()
        where = [[None] * len(s["grams"]) for s in streams]
        q = 0
        for k in range(max([len(s["grams"]) for s in streams] + [0])):
            for i, s in enumerate(streams):
                if k >= len(s["grams"]):
                    continue
                want = aligns[q % len(aligns)] if s["align"] is None else s["align"][k] if isinstance(s["align"], (list, tuple)) else s["align"]
                while len(src) % 16 != want:
                    src.append(GAP)
                where[i][k] = len(src)
                src += s["grams"][k]
                q += 1
        self.src = bytes(src)
        self.table, at = [], dst_lead
        for i, s in enumerate(streams):
            s["first"], s["n"] = len(self.table), len(s["grams"])
            self.table += [(where[i][k], len(g)) for k, g in enumerate(s["grams"])]
            s["dst_offset"], s["dst_capacity"] = at, sum(max(len(g) - 58, 0) for g in s["grams"])
            at += s["dst_capacity"] + GUARD + i
        self.dst0 = bytes([FILL]) * at
        want = bytearray(self.dst0)
        self.recs, self.results = [], []
        for s in streams:
            recs, res, out = RX.receive(s["state"], s["grams"], s["dst_offset"])
            assert len(out) <= s["dst_capacity"]
            want[s["dst_offset"]:s["dst_offset"] + len(out)] = out
            self.recs += recs
            self.results.append(res)
        self.want = bytes(want)
        # the tables and the expected arrays in the ABI's layouts
        self.d_streams = np.zeros(len(streams), dtype=capi.OHM_RX_STREAM)
        for row, s in zip(self.d_streams, streams):
            row["first_datagram"], row["n_datagrams"], row["dst_offset"], row["dst_capacity"] = s["first"], s["n"], s["dst_offset"], s["dst_capacity"]
            state_row(row, "", s["state"])
        self.d_grams = np.zeros(len(self.table), dtype=capi.OHM_RX_DATAGRAM)
        for row, (off, size) in zip(self.d_grams, self.table):
            row["src_offset"], row["bytes"] = off, size
        self.want_records = np.zeros(len(self.recs), dtype=capi.OHM_RX_RECORD)
        for row, r in zip(self.want_records, self.recs):
            for k in ("status", "disposition", "events", "msg_type", "order", "dst_offset", "audio_offset", "audio_bytes") + RX.HEADER_FIELDS:
                row[k] = r[k]
            row["codec"][:len(r["codec"])] = np.frombuffer(r["codec"], dtype=np.uint8)
        self.want_results = np.zeros(len(streams), dtype=capi.OHM_RX_STREAM_RESULT)
        for row, res in zip(self.want_results, self.results):
            state_row(row, "", res["state_out"])
            for k in ("out_bytes", "n_output", "n_pending", "stop_reason"):
                row[k] = res[k]
            row["n_resend"] = len(res["resend"])
            row["resend"][:len(res["resend"])] = res["resend"]

    def driver_blob(self):
        """the job file of tests/cpp/ohm_rx_core_driver.cpp"""
        return b"".join([struct.pack("<IIQQ", len(self.streams), len(self.table), len(self.src), len(self.dst0)), self.d_streams.tobytes(),
                         self.d_grams.tobytes(), self.src, self.dst0])


def describe(got, want):
    """the first record or result that differs, field by field (for an assertion's message)"""
    for k in range(min(len(got), len(want))):
        if got[k].tobytes() != want[k].tobytes():
            return "entry %d: " % k + ", ".join("%s %s != %s" % (n, got[k][n], want[k][n]) for n in got.dtype.names if np.any(got[k][n] != want[k][n]))
    return "lengths %d, %d" % (len(got), len(want))


def assert_same(got_results, got_records, got_arena, job):
    assert got_records.tobytes() == job.want_records.tobytes(), describe(got_records, job.want_records)
    assert got_results.tobytes() == job.want_results.tobytes(), describe(got_results, job.want_results)
    got, want = np.frombuffer(bytes(got_arena), dtype=np.uint8), np.frombuffer(job.want, dtype=np.uint8)
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d bytes differ, the first at %d" % (bad.size, bad[0])


# ---------------------------------------------------------------- the alignment and length sweep
SWEEP_AUDIO = (0, 1, 2, 3, 4, 5, 6, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1320, 1440, 5759, 5760)
SWEEP_CODEC = (0, 1, 2, 3, 29)


def sweep_job(seed=61):
    """five interleaved streams, one codec length each (0, 1, 2, 3, 29: the payload meets every residue mod 4), and in each every
    audio length at every datagram offset mod 16 (0, 4, 8, 12): the whole cross product, 400 datagrams; mono 8-bit audio so that any
    byte count is whole frames; the running destination offset meets every residue mod 16 (asserted by the tests)"""
    rng = Lcg(seed)
    streams = []
    for i, codec in enumerate(SWEEP_CODEC):
        lengths = [(n, a) for a in (0, 4, 8, 12) for n in SWEEP_AUDIO[i:] + SWEEP_AUDIO[:i]]
        grams = [audio_gram(100 + k, rng.bytes(n), codec=b"c" * codec, depth=8, channels=1) for k, (n, _) in enumerate(lengths)]
        streams.append(stream(grams, align=[a for _, a in lengths]))
    return Job(streams)


# ---------------------------------------------------------------- the committed sessions
def load_sessions():
    with open(GOLDEN) as f:
        return json.load(f)["sessions"]


def session_stream(s):
    return stream([bytes.fromhex(g) for g in s["datagrams"]], state=s["state_in"])
