"""What the RAOP receiver's tests share (tests/test_raop_rx_*.py, tests/test_gpu_raop_rx_*.py): datagram builders, the committed
cases, fixed-seed lossy sessions, the shapes at which the wave sequencer can go wrong, and Job -- streams laid out in a source arena
as the C ABI's tables, with the answers of tests/raop_rx_textbook.py beside them.  TEST INFRASTRUCTURE ONLY."""
import json
import os
import struct

import numpy as np

import raop_rx_textbook as RX
from ohm_rx_cases import Lcg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "raop_rx_textbook.json")
SSRC = 0x1234abcd


def audio_gram(seq, payload=b"\1\2\3\4", timestamp=None, ssrc=SSRC, marker=0, extension=0, version=2, ptype=0x60):
    """a datagram of the audio port: the 4 header bytes, timestamp, ssrc, the encrypted payload"""
    timestamp = (seq * 352) & 0xffffffff if timestamp is None else timestamp
    return struct.pack(">BBHII", (version << 6) | (extension << 4), (marker << 7) | ptype, seq & 0xffff, timestamp, ssrc) + bytes(payload)


def resend_gram(seq, payload=b"\1\2\3\4", outer_seq=1, **inner):
    """a resend response of the control port: a 0x56 header around a whole audio datagram"""
    return struct.pack(">BBH", 0x80, 0x80 | 0x56, outer_seq) + audio_gram(seq, payload, **inner)


def sync_gram(rtp_timestamp, latency, extension=0, seq=7):
    return struct.pack(">BBHIIII", 0x80 | (extension << 4), 0x80 | 0x54, seq, (rtp_timestamp - latency) & 0xffffffff, 0x83aa7e80, 0x1000, rtp_timestamp)


def other_gram(kind, body=b"\0" * 8):
    return struct.pack(">BBH", 0x80, 0x80 | kind, 1) + bytes(body)


def A(seq, **kw):
    return (audio_gram(seq, **kw), RX.AUDIO)


def R(seq, **kw):
    return (resend_gram(seq, **kw), RX.CONTROL)


def S(rtp_timestamp, latency, **kw):
    return (sync_gram(rtp_timestamp, latency, **kw), RX.CONTROL)


def stream(grams, state=None, max_frames=50, align=None):
    """one stream of a Job: [(bytes, port)] in arrival order, the state it starts from (None: a new receiver's), and the source offset
    mod 16 of all its datagrams (None: any multiple of 4)"""
    return dict(grams=[(bytes(g), p) for g, p in grams], state=dict(state or RX.new_state()), max_frames=max_frames, align=align)


def running_state(frame, latency=0, **more):
    """a stream in the middle of a session: started, running, the last frame output `frame`"""
    return dict(RX.new_state(), running=1, started=1, session_id=SSRC, frame=frame & 0xffff, latency=latency, control_latency=latency, **more)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_grams(session):
    return [(bytes.fromhex(g["hex"]), g["port"]) for g in session["datagrams"]]


# ---- the reference's SuiteRaopResend as batches: a step list is cut wherever the timer fires, DropAudio is called or a stop is thrown
def suite_batches(case):
    """-> [(grams, what)] with what = ("timer", ranges) | ("drop",) | ("throws", reason) | ("end",)"""
    batches, grams = [], []
    for step in case["steps"]:
        if step[0] == "in":
            grams.append(R(step[1]) if step[2] else A(step[1]))
        elif step[0] == "throws":
            grams.append(R(step[1]) if step[2] else A(step[1]))
            batches.append((grams, ("throws", step[3])))
            grams = []
        else:
            batches.append((grams, tuple(step)))
            grams = []
    batches.append((grams, ("end",)))
    return batches


def play(batches, max_frames, run=None, state=None):
    """The caller's side of the hand-over: each batch is the PENDING datagrams of the one before, by `order`, then its own; state_out
    becomes state_in; DropAudio forgets the pending ones.  -> per batch (grams as run, records, result).  `run(state, max_frames, grams)`
    defaults to the model."""
    run = run or RX.run_stream
    state = dict(state or RX.new_state())
    carried, out = [], []
    for grams, what in batches:
        todo = carried + list(grams)
        recs, res = run(state, max_frames, todo)
        out.append((todo, recs, res))
        state = dict(res["state_out"])
        carried = [todo[i] for i in res["pending"]]
        if what[0] == "drop":
            state, carried = RX.drop_audio(state), []
    return out


# ---- fixed-seed lossy sessions: one list of (gram, port) in arrival order, over a sender that counts up from `first`
def lossy_session(seed, n=80, first=None, max_frames=5):
    rng = Lcg(seed)
    first = rng.below(65536) if first is None else first
    if rng.below(3) == 0:
        first = (65536 - rng.below(n)) & 0xffff                 # the wrap falls inside the session
    late = {}                                                   # arrival slot -> [(seq, as a resend)]
    grams = []
    for k in range(n):
        seq = (first + k) & 0xffff
        what = rng.below(100)
        if k and what < 12:                                     # lost: a resend comes 1..2 * max_frames + 2 packets later
            late.setdefault(k + 1 + rng.below(2 * max_frames + 2), []).append((seq, True))
        elif k and what < 16:                                   # late on the audio port itself
            late.setdefault(k + 1 + rng.below(max_frames), []).append((seq, False))
        else:
            grams.append(A(seq, payload=rng.bytes(1 + rng.below(9))))
            if what >= 96:
                grams.append(R(seq - rng.below(max_frames + 2), payload=b"dup"))      # an answer nobody needs any more
            if what == 95:
                grams.append(S(seq * 352, 11025 + 441 * rng.below(3)))
            if what == 94:
                grams.append(A(seq, ssrc=SSRC + 1))
            if what == 93:
                grams.append((other_gram(0x55), RX.CONTROL))
            if what == 92:
                grams.append((audio_gram(seq)[:6 + rng.below(6)], RX.AUDIO))
        for seq2, resend in late.pop(k, []):
            grams.append(R(seq2, payload=rng.bytes(3)) if resend else A(seq2, payload=rng.bytes(3)))
            if rng.below(4) == 0:
                grams.append(R(seq2, payload=rng.bytes(3)))                          # the answer comes twice
    return grams


LOSSY_SEEDS = tuple(range(1, 41)) + (258,)     # (258: the one below 500 in which the set is full when a frame below its first one comes)
COVERAGE = ("full at the first", "full in the middle", "full at the last", "restart in a repair", "restart outside a repair", "wrap inside a repair",
            "duplicate of the first", "duplicate of the last", "duplicate of a middle one", "duplicate of the past in a repair", "duplicate of the past outside a repair")


def lossy_streams():
    return [stream(lossy_session(seed), max_frames=5 if seed % 4 else 50) for seed in LOSSY_SEEDS]


# ---- the shapes at which the wave sequencer can go wrong (a trip is 64 datagrams)
def fill(first, max_frames, extra, where):
    """frame `first` goes out, first + 1 is missing; then frames that wait until max_frames + 1 wait (`extra` 0) or one more comes
    (`extra` 1) at the first, a middle or the last place of the waiting set"""
    base = first + 10
    count = max_frames + 1 + extra
    seqs = [base + 2 * k for k in range(count)]
    chosen = seqs[{"first": 0, "middle": count // 2, "last": count - 1}[where]]
    return [A(first)] + [A(s) for s in seqs if s != chosen] + [A(chosen)]


def shape_streams():
    out = []
    for n in (1, 63, 64, 65, 128, 129):                                    # in-order runs
        out.append(stream([A(100 + k) for k in range(n)], running_state(99)))
    for lane in (0, 31, 63, 64):                                           # the 65535 -> 0 wrap at a lane
        out.append(stream([A(65536 - lane + k) for k in range(130)], running_state(65535 - lane)))
    for lane in (0, 1, 63):                                                # what breaks a trip, at a lane
        for odd in (S(5000, 11025), A(7, ssrc=SSRC ^ 1), (audio_gram(9)[:11], RX.AUDIO)):
            grams = [A(200 + k) for k in range(140)]
            grams.insert(lane, odd)
            grams.insert(64 + lane + 1, odd)
            out.append(stream(grams, running_state(199)))
    for max_frames in (1, 5, 50, 63):
        for extra in (0, 1):
            for where in ("first", "middle", "last"):
                out.append(stream(fill(300, max_frames, extra, where), None, max_frames))
        # a drain of 1, 2 and max_frames + 1 waiting frames, and then the stream goes on in order
        for drain in sorted({1, min(2, max_frames + 1), max_frames + 1}):
            out.append(stream([A(10)] + [A(12 + k) for k in range(drain)] + [R(11)] + [A(12 + drain + k) for k in range(70)], None, max_frames))
    # a drain that ends exactly at a trip boundary: 60 in order, 3 wait, the missing one is datagram 64 of the batch
    out.append(stream([A(k) for k in range(60)] + [A(61), A(62), A(63), R(60)] + [A(64 + k) for k in range(70)], None, 5))
    # duplicates of the first, the last and a middle waiting frame, of the past, and the late non-resend in and outside a repair
    waits = [A(500), A(510), A(520), A(530)]
    out.append(stream(waits + [A(510), R(530), A(520), R(499), R(500)] + [R(501 + k) for k in range(9)], None, 5))
    out.append(stream(waits + [A(499)] + [A(531)], None, 5))
    out.append(stream([A(500), A(501), A(500), A(502)], None, 5))
    out.append(stream([A(500), A(501), R(500), R(501), A(502)], None, 5))
    # start and resume, the flush window, a delay on both sides of the threshold
    out.append(stream([S(1000, 11025), A(1), A(2), S(2000, 11025 + 440), A(3), S(3000, 11025 + 441), A(4), A(5)]))
    out.append(stream([A(40, timestamp=900), A(41, timestamp=1001), A(39, timestamp=2000), A(42, timestamp=1002)],
                      dict(running_state(0), running=0, resume_pending=1, flush_seq=41, flush_time=1000)))
    return out


SWEEP_LENGTHS = tuple(range(21)) + tuple(range(1470, 1475))


def sweep_streams():
    """every datagram length 0..20 and 1470..1474 of every kind, at each of the four source offsets mod 16"""
    kinds = [(audio_gram(1, bytes(1500)), RX.AUDIO), (resend_gram(2, bytes(1500)), RX.CONTROL), (sync_gram(9000, 11025) + bytes(1500), RX.CONTROL),
             (other_gram(0x55, bytes(1500)), RX.CONTROL)]
    return [stream([(g[:n], port) for n in SWEEP_LENGTHS for g, port in kinds], align=a) for a in (0, 4, 8, 12)]


def mixed_streams(n=64):
    """n streams of mixed shapes, empty ones between full ones"""
    shapes, lossy = shape_streams(), lossy_streams()
    out = []
    for k in range(n):
        out.append(stream([]) if k % 5 == 2 else (shapes[(7 * k) % len(shapes)] if k % 2 else lossy[k % len(lossy)]))
    return out


# ---- the C ABI's tables with the model's answers beside them
class Job:
    def __init__(self, streams, base=0):
        """`base`: where the first datagram lies in the source arena (a multiple of 4); the arena ends with the last datagram"""
        from ohpipeline_amd import capi
        self.streams = streams
        rng = Lcg(len(streams) + 17)
        src = bytearray(base)
        table = []
        for s in streams:
            for g, port in s["grams"]:
                if s["align"] is None:
                    src += rng.bytes((-len(src)) % 4 + 4 * rng.below(3))              # junk between datagrams, each at a multiple of 4
                else:
                    src += rng.bytes((s["align"] - len(src)) % 16)
                table.append((len(src), len(g), port))
                src += g
        self.src = bytes(src)
        self.table = table
        n = len(table)
        self.d_grams = np.zeros(n, dtype=capi.RAOP_RX_DATAGRAM)
        self.d_streams = np.zeros(len(streams), dtype=capi.RAOP_RX_STREAM)
        self.want_records = np.zeros(n, dtype=capi.RAOP_RX_RECORD)
        self.want_results = np.zeros(len(streams), dtype=capi.RAOP_RX_STREAM_RESULT)
        self.want_rows = np.zeros(n, dtype=capi.ALAC_PACKET)
        for k, (off, size, port) in enumerate(table):
            self.d_grams[k] = (off, size, port, 0)
        self.recs, self.results = [], []
        at = 0
        for i, s in enumerate(streams):
            row = self.d_streams[i]
            row["first_datagram"], row["n_datagrams"], row["max_frames"] = at, len(s["grams"]), s["max_frames"]
            for f in RX.STATE_FIELDS:
                row[f] = s["state"][f]
            recs, res = RX.run_stream(s["state"], s["max_frames"], s["grams"])
            self.recs.append(recs)
            self.results.append(res)
            for k, r in enumerate(recs):
                w = self.want_records[at + k]
                for f in ("status", "disposition", "events", "resend", "marker", "extension", "type", "port", "seq", "payload_offset", "payload_bytes", "timestamp",
                          "ssrc", "sync", "order"):
                    w[f] = r[f]
            w = self.want_results[i]
            for f in RX.STATE_FIELDS:
                w[f] = res["state_out"][f]
            w["n_output"], w["n_pending"], w["stop_reason"], w["n_ranges"] = res["n_output"], res["n_pending"], res["stop_reason"], len(res["ranges"])
            for j, (a, b) in enumerate(res["ranges"]):
                w["ranges"][j] = (a, b)
            for j, (index, poff, pbytes) in enumerate(res["rows"]):
                self.want_rows[at + j] = (table[at + index][0] + poff, pbytes, 0)
            at += len(s["grams"])

    def driver_blob(self):
        """the job file of tests/cpp/raop_rx_core_driver.cpp"""
        return b"".join([struct.pack("<IIQ", len(self.streams), len(self.table), len(self.src)), self.d_streams.tobytes(), self.d_grams.tobytes(), self.src])


def describe(got, want):
    """the first row that differs, field by field (for an assertion's message)"""
    for k in range(min(len(got), len(want))):
        if got[k].tobytes() != want[k].tobytes():
            return f"row {k}: " + "; ".join(f"{f}: got {got[k][f]}, want {want[k][f]}" for f in want.dtype.names if np.any(got[k][f] != want[k][f]))
    return f"{len(got)} rows where {len(want)} are wanted"


def assert_same(got_results, got_records, got_rows, job):
    assert got_records.tobytes() == job.want_records.tobytes(), describe(got_records, job.want_records)
    assert got_results.tobytes() == job.want_results.tobytes(), describe(got_results, job.want_results)
    assert got_rows.tobytes() == job.want_rows.tobytes(), describe(got_rows, job.want_rows)
