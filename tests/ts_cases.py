"""What the transport stream and ADTS tests share: a test-side muxer (packets, sections, PES packets, ADTS frames), the named streams,
and two Jobs -- streams laid into a source arena allocated to the byte (and, layer 1, a destination arena of FILL with guard bytes
round every run), the descriptors, and what the model (tests/ts_textbook.py) says the results, the tables and the destination arena
must be.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import ts_textbook as TX

FILL, GUARD = 0xA5, 24
PMT_PID, AUDIO_PID, OTHER_PID = 0x1000, 0x0100, 0x0101


class Lcg:
    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFF

    def next(self):
        self.s = (self.s * 1664525 + 1013904223) & 0xFFFFFFFF
        return self.s >> 8

    def below(self, n):
        return self.next() % n

    def bytes(self, n):
        return bytes(self.next() & 0xFF for _ in range(n))


# ---------------------------------------------------------------- the muxer
def packet(pid, payload=b"", start=False, cc=0, adaptation=None, payload_bit=True, tei=False, scrambling=0, sync=0x47):
    """One 188-byte packet.  adaptation: the field's length byte L (None: whatever fills the packet; no field for 184 payload bytes).
    L > 183 is written as it stands, with filler behind it."""
    payload = bytes(payload)
    if adaptation is None and len(payload) < 184:
        adaptation = 183 - len(payload)
    head = bytes([sync, (0x80 if tei else 0) | (0x40 if start else 0) | pid >> 8, pid & 0xFF,
                  scrambling << 6 | (0x20 if adaptation is not None else 0) | (0x10 if payload_bit else 0) | cc & 15])
    if adaptation is None:
        body = payload
    elif adaptation > 183:
        body = bytes([adaptation]) + b"\xff" * 183
    else:
        body = bytes([adaptation]) + (b"\x00" + b"\xff" * (adaptation - 1) if adaptation else b"") + payload
    out = head + body
    assert len(out) == 188, (len(out), adaptation, len(payload))
    return out


def with_crc(section_without_crc):
    return bytes(section_without_crc) + TX.crc(section_without_crc).to_bytes(4, "big")


def refit(section, at, value):
    """The section with byte `at` replaced and its CRC made right again: only the check on that byte can fail."""
    body = bytearray(section[:-4])
    body[at] = value
    return with_crc(body)


def section(table_id, body, ext=1):
    length = 5 + len(body) + 4
    return with_crc(bytes([table_id, 0xB0 | length >> 8, length & 0xFF, ext >> 8, ext & 0xFF, 0xC1, 0, 0]) + bytes(body))


def pat(programs=((1, PMT_PID),)):
    return section(0, b"".join(bytes([n >> 8, n & 0xFF, 0xE0 | pid >> 8, pid & 0xFF]) for n, pid in programs))


def pmt(streams=((0x0F, AUDIO_PID, b""),), program_info=b"", pcr_pid=0x1FFF):
    body = bytes([0xE0 | pcr_pid >> 8, pcr_pid & 0xFF, 0xF0 | len(program_info) >> 8, len(program_info) & 0xFF]) + bytes(program_info)
    for kind, pid, desc in streams:
        body += bytes([kind, 0xE0 | pid >> 8, pid & 0xFF, 0xF0 | len(desc) >> 8, len(desc) & 0xFF]) + bytes(desc)
    return section(2, body)


def psi(pid, sec, pointer=0, cc=0, start=True):
    payload = bytes([pointer]) + b"\x55" * pointer + bytes(sec)
    return packet(pid, payload + b"\xff" * (184 - len(payload)), start=start, cc=cc)


def pes(es, stream_id=0xC0, pts=None, stuffing=0, length="right", marker=0x80):
    """A PES packet.  h = 5 with a PTS, plus `stuffing`.  length: "right", 0, or the 16-bit field as it is to stand."""
    h = (5 if pts is not None else 0) + stuffing
    head = b""
    if pts is not None:
        head = bytes([0x21 | (pts >> 30 & 7) << 1, pts >> 22 & 0xFF, (pts >> 15 & 0x7F) << 1 | 1, pts >> 7 & 0xFF, (pts & 0x7F) << 1 | 1])
    n = 3 + h + len(es) if length == "right" else length
    return b"\x00\x00\x01" + bytes([stream_id, n >> 8, n & 0xFF, marker, 0x80 if pts is not None else 0, h]) + head + b"\xff" * stuffing + bytes(es)


def carry(pid, data, cc=0, sizes=None, start=True):
    """The packets that carry `data` on `pid`: payloads of `sizes` bytes in turn (then 184), the first with payload_unit_start."""
    out, at, k = [], 0, 0
    data = bytes(data)
    while at < len(data) or not out:
        n = min(sizes[k] if sizes and k < len(sizes) else 184, len(data) - at)
        out.append(packet(pid, data[at:at + n], start=start and k == 0, cc=cc + k))
        at += n
        k += 1
    return out


def head_packets(cc=0):
    return [psi(0, pat(), cc=cc), psi(PMT_PID, pmt(), cc=cc)]


def adts_frame(payload, protection_absent=True, profile=1, sf_index=4, channels=2, blocks=0, layer=0, length=None):
    header_bytes = 7 if protection_absent else 9
    n = header_bytes + len(payload) if length is None else length
    head = bytes([0xFF, 0xF0 | layer << 1 | (1 if protection_absent else 0), profile << 6 | sf_index << 2 | channels >> 2, (channels & 3) << 6 | n >> 11,
                  n >> 3 & 0xFF, (n & 7) << 5 | 0x1F, 0xFC | blocks])
    return head + (b"\x12\x34" if not protection_absent else b"") + bytes(payload)


def clean(data):
    """Random bytes with no 0xff in them: junk that holds no header by accident."""
    return bytes(b if b != 0xFF else 0x7F for b in data)


# ---------------------------------------------------------------- layer 1's Job
def stream(data, flags=0, pmt_pid=0, audio_pid=0, pes_open_bytes=0, pes_capacity=None, es=None):
    return dict(data=bytes(data), flags=flags, pmt_pid=pmt_pid, audio_pid=audio_pid, pes_open_bytes=pes_open_bytes, pes_capacity=pes_capacity, es=es)


RESULT_FIELDS = ("status", "trailing_bytes", "pmt_pid", "audio_pid", "packets", "bad_sync", "tei_packets", "scrambled_packets", "pat_packet", "pmt_packet",
                 "audio_packets", "bad_pes_starts", "dropped_bytes", "cc_jumps", "pes_open_bytes", "corrupt_packet")
PES_FIELDS = ("es_offset", "pts", "bytes", "packet", "flags", "stream_id")


class Job:
    def __init__(self, streams, seed=5, src_phase=None, dst_phase=None):
        from ohpipeline_amd import capi
        rng = Lcg(seed)
        self.streams = streams
        self.models = [TX.demux(s["data"], s["flags"], s["pmt_pid"], s["audio_pid"], s["pes_open_bytes"]) for s in streams]
        n = len(streams)
        self.descs = np.zeros(n, dtype=capi.TS_STREAM_DESC)
        src, dst_at, pes_at = bytearray(), GUARD, 0
        for i, (s, m) in enumerate(zip(streams, self.models)):
            if src_phase is not None:
                src += rng.bytes((src_phase[i] - len(src)) % 16)
            elif i:
                src += rng.bytes(1 + rng.below(7))                      # streams at every alignment, junk between them
            if dst_phase is not None:
                dst_at += (dst_phase[i] - dst_at) % 16
            d = self.descs[i]
            cap = len(m["pes"]) if s["pes_capacity"] is None else s["pes_capacity"]
            room = len(s["data"]) // 188 * 184
            d["src_offset"], d["src_bytes"], d["dst_offset"], d["dst_capacity"] = len(src), len(s["data"]), dst_at, room
            d["flags"], d["pmt_pid"], d["audio_pid"], d["pes_open_bytes"] = s["flags"], s["pmt_pid"], s["audio_pid"], s["pes_open_bytes"]
            d["pes_first"], d["pes_capacity"] = pes_at, cap
            src += s["data"]
            dst_at += room + GUARD + rng.below(5)
            pes_at += cap + (i % 2)                                     # (a gap in the table now and then)
        self.src = np.frombuffer(bytes(src), dtype=np.uint8) if src else np.zeros(0, dtype=np.uint8)
        self.n_pes = pes_at
        self.dst0 = np.full(dst_at if n else 0, FILL, dtype=np.uint8)
        self.want = self.dst0.copy()
        for d, m in zip(self.descs, self.models):
            a = int(d["dst_offset"])
            self.want[a:a + len(m["run"])] = np.frombuffer(m["run"], dtype=np.uint8)

    def driver_blob(self):
        head = np.array([len(self.streams), self.n_pes, self.src.size, self.dst0.size], dtype="<u8")
        return head.tobytes() + self.descs.tobytes() + self.src.tobytes() + self.dst0.tobytes()


def assert_same(results, pes, arena, job):
    """Every result, every record a stream has room for, and the whole destination arena are the model's."""
    arena = np.frombuffer(bytes(arena), dtype=np.uint8)
    for i, (d, m) in enumerate(zip(job.descs, job.models)):
        r = results[i]
        got = {f: int(r[f]) for f in RESULT_FIELDS}
        assert got == {f: m[f] for f in RESULT_FIELDS}, (i, got, {f: m[f] for f in RESULT_FIELDS})
        assert int(r["pes_packets"]) == len(m["pes"]) and int(r["bytes_delivered"]) == len(m["run"]), (i, int(r["pes_packets"]), len(m["pes"]), int(r["bytes_delivered"]), len(m["run"]))
        first, cap = int(d["pes_first"]), int(d["pes_capacity"])
        for k, want in enumerate(m["pes"][:cap]):
            rec = pes[first + k]
            assert {f: int(rec[f]) for f in PES_FIELDS} == {f: want[f] for f in PES_FIELDS}, (i, k, {f: int(rec[f]) for f in PES_FIELDS}, want)
    bad = np.flatnonzero(arena != job.want)
    assert bad.size == 0, f"{bad.size} of {job.want.size} destination bytes differ, first at {bad[:8].tolist()}"


# ---------------------------------------------------------------- layer 2's Job
def adts_stream(data, flags=0, frame_capacity=None):
    return dict(data=bytes(data), flags=flags, frame_capacity=frame_capacity)


ADTS_RESULT_FIELDS = ("status", "bytes_consumed", "first_frame_offset", "interruptions", "skipped_bytes", "mean_payload_bytes", "profile", "sf_index", "channel_config")
FRAME_FIELDS = ("offset", "bytes", "flags", "header_bytes", "profile", "sf_index", "channel_config")


class AdtsJob:
    def __init__(self, streams, seed=6, lead=0):
        from ohpipeline_amd import capi
        rng = Lcg(seed)
        self.streams = streams
        self.models = [TX.adts_chain(s["data"], s["flags"]) for s in streams]
        self.descs = np.zeros(len(streams), dtype=capi.ADTS_STREAM_DESC)
        src, at = bytearray(rng.bytes(lead)), 0
        for i, (s, m) in enumerate(zip(streams, self.models)):
            if i:
                src += rng.bytes(1 + rng.below(7))
            d = self.descs[i]
            cap = len(m["frames"]) if s["frame_capacity"] is None else s["frame_capacity"]
            d["src_offset"], d["src_bytes"], d["flags"], d["frame_first"], d["frame_capacity"] = len(src), len(s["data"]), s["flags"], at, cap
            src += s["data"]
            at += cap + (i % 2)
        self.src = np.frombuffer(bytes(src), dtype=np.uint8) if src else np.zeros(0, dtype=np.uint8)
        self.n_frames = at

    def driver_blob(self):
        head = np.array([len(self.streams), self.n_frames, self.src.size, 0], dtype="<u8")
        return head.tobytes() + self.descs.tobytes() + self.src.tobytes()


def assert_same_adts(results, frames, job):
    for i, (d, m) in enumerate(zip(job.descs, job.models)):
        r = results[i]
        got = {f: int(r[f]) for f in ADTS_RESULT_FIELDS}
        assert got == {f: m[f] for f in ADTS_RESULT_FIELDS}, (i, got, {f: m[f] for f in ADTS_RESULT_FIELDS})
        assert int(r["frames"]) == len(m["frames"]), (i, int(r["frames"]), len(m["frames"]))
        first, cap = int(d["frame_first"]), int(d["frame_capacity"])
        for k, want in enumerate(m["frames"][:cap]):
            rec = frames[first + k]
            assert {f: int(rec[f]) for f in FRAME_FIELDS} == {f: want[f] for f in FRAME_FIELDS}, (i, k)


# ---------------------------------------------------------------- the named streams of layer 1: every rule at least once
def audio_run(rng, n_pes=3, cc=0, sizes=None, es_bytes=(300, 41, 700), **kw):
    """(packets, the elementary bytes) of n_pes PES packets on the audio PID, counters in order."""
    out, es = [], b""
    for k in range(n_pes):
        part = rng.bytes(es_bytes[k % len(es_bytes)])
        got = carry(AUDIO_PID, pes(part, pts=90000 * k + 7, **kw), cc=cc + len(out), sizes=sizes)
        out += got
        es += part
    return out, es


def named():
    rng = Lcg(2025)
    out = {}

    def put(name, packets, es=None, **kw):
        out[name] = stream(b"".join(packets), es=es, **kw)

    # ---- packet counts
    audio, es = audio_run(rng, n_pes=70, es_bytes=(700, 150, 1200))
    whole = head_packets() + audio
    for n in (0, 1, 2, 3, 63, 64, 65, 255, 256, 257):
        put(f"packets_{n}", whole[:n])
    put("bytes_187", [whole[0][:187]])
    put("bytes_188_187", [whole[0], whole[1][:187]])
    put("ten_pes", head_packets() + audio_run(rng, n_pes=10)[0])
    # ---- every adaptation length, hence every payload length; 184 is corrupt, and the packets behind it are not looked at
    body = rng.bytes(184 + sum(range(185)) + 300)
    lengths = list(range(184, -1, -1))
    put("every_payload_length", head_packets() + carry(AUDIO_PID, pes(body, length=0), sizes=[184] + lengths))
    tail, _ = audio_run(rng, n_pes=2, cc=5)
    put("corrupt", head_packets() + audio_run(rng, n_pes=2)[0] + [packet(OTHER_PID, b"", adaptation=184)] + tail + [psi(0, pat())])
    put("corrupt_before_pat", [packet(OTHER_PID, b"", adaptation=200)] + whole[:9])
    put("corrupt_skipped", head_packets() + [packet(OTHER_PID, b"", adaptation=184, tei=True)] + audio_run(rng, n_pes=2)[0])
    tiny = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 1, 0, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1]
    put("tiny_payloads", head_packets() + carry(AUDIO_PID, pes(rng.bytes(600), length=0), sizes=[100] + tiny))
    # ---- PAT and PMT
    put("pointer_field", [psi(0, pat(), pointer=7), psi(PMT_PID, pmt(), pointer=30)] + audio_run(rng)[0])
    put("program_zero_first", [psi(0, pat(((0, 0x0010), (3, PMT_PID))))] + [psi(PMT_PID, pmt())] + audio_run(rng)[0])
    bad_pat = bytearray(pat(((1, 0x0FFF),)))
    bad_pat[-1] ^= 1
    put("bad_crc_then_good", [psi(0, bad_pat), psi(0x0FFF, pmt()), psi(0, pat()), psi(PMT_PID, pmt())] + audio_run(rng)[0])
    rich = pmt(((0x1B, 0x0200, b"\x28\x04abcd"), (0x03, 0x0201, b""), (0x0F, AUDIO_PID, b"\x0a\x04eng\x00")), program_info=b"\x05\x04HDMV")
    put("rich_pmt", [psi(0, pat()), psi(PMT_PID, rich)] + audio_run(rng)[0])
    put("pmt_without_audio", [psi(0, pat()), psi(PMT_PID, pmt(((0x1B, 0x0200, b""), (0x03, AUDIO_PID, b""))))] + audio_run(rng)[0])
    put("pmt_before_pat", [psi(PMT_PID, pmt(((0x0F, OTHER_PID, b""),)))] + head_packets() + audio_run(rng)[0])
    early, _ = audio_run(rng, n_pes=1)
    late, _ = audio_run(rng, n_pes=2, cc=len(early))
    put("audio_before_pmt", [psi(0, pat())] + early + [psi(PMT_PID, pmt())] + late)
    fits = pmt(((0x0F, AUDIO_PID, b"\x0a" + bytes([160]) + b"x" * 160),))
    fits = pmt(((0x0F, AUDIO_PID, b"\x0a" + bytes([160 + 183 - len(fits)]) + b"x" * (160 + 183 - len(fits))),))
    assert len(fits) == 183
    put("section_ends_with_packet", [psi(0, pat()), psi(PMT_PID, fits)] + audio_run(rng)[0])
    over = bytearray(fits[:-4])
    over[2] += 1                                                         # one byte behind the packet's last
    put("section_one_byte_over", [psi(0, pat()), psi(PMT_PID, with_crc(over)[:183]), psi(PMT_PID, pmt())] + audio_run(rng)[0])
    good_pat, good_pmt = pat(), pmt(((0x03, 0x0201, b""), (0x0F, AUDIO_PID, b"")))
    breaks = [("pat_syntax_indicator", 0, refit(good_pat, 1, good_pat[1] & 0x7F)), ("pat_private_bit", 0, refit(good_pat, 1, good_pat[1] | 0x40)),
              ("pat_reserved", 0, refit(good_pat, 1, good_pat[1] & ~0x10 & 0xFF)), ("pat_length_bits", 0, refit(good_pat, 1, good_pat[1] | 0x04)),
              ("pat_version_reserved", 0, refit(good_pat, 5, 0x41)), ("pat_entry_reserved", 0, refit(good_pat, 10, good_pat[10] & 0x1F)),
              ("pat_table_id", 0, refit(good_pat, 0, 2)),
              ("pmt_pcr_reserved", 2, refit(good_pmt, 8, good_pmt[8] & 0x1F)), ("pmt_info_reserved", 2, refit(good_pmt, 10, good_pmt[10] & 0x7F)),
              ("pmt_info_length_bits", 2, refit(good_pmt, 10, good_pmt[10] | 0x08)), ("pmt_stream_reserved", 2, refit(good_pmt, 13, good_pmt[13] & 0x1F)),
              ("pmt_es_reserved", 2, refit(good_pmt, 15, good_pmt[15] & 0xEF)), ("pmt_es_length_bits", 2, refit(good_pmt, 15, good_pmt[15] | 0x04)),
              ("pmt_es_overruns", 2, refit(good_pmt, 16, 40)), ("pmt_table_id", 2, refit(good_pmt, 0, 0))]
    for name, table, broken in breaks:
        first = [psi(0, broken), psi(0, pat())] if table == 0 else [psi(0, pat()), psi(PMT_PID, broken)]
        put("break_" + name, first + [psi(PMT_PID, pmt())] + audio_run(rng)[0])
    put("audio_pid_given", [psi(0, pat(((1, 0x0999),)))] + audio_run(rng)[0], audio_pid=AUDIO_PID)
    put("pmt_pid_given", [psi(0, pat(((1, 0x0999),))), psi(PMT_PID, pmt())] + audio_run(rng)[0], pmt_pid=PMT_PID)
    put("no_pat", audio_run(rng)[0])
    put("no_pmt", [psi(0, pat())] + audio_run(rng)[0])
    # ---- PES
    h = []
    for stuffing, pts in ((0, None), (0, 12345678), (5, 0x1FFFFFFFF), (10, None)):
        h += carry(AUDIO_PID, pes(rng.bytes(260), pts=pts, stuffing=stuffing), cc=len(h))
    put("header_lengths", head_packets() + h)
    fills = pes(b"", pts=5, stuffing=170, length=0)
    assert len(fills) == 184
    put("header_fills_packet", head_packets() + [packet(AUDIO_PID, fills, start=True, cc=0), packet(AUDIO_PID, rng.bytes(184), cc=1), packet(AUDIO_PID, rng.bytes(20), cc=2)])
    too_long = bytearray(fills)
    too_long[8] += 1
    put("header_one_byte_too_long", head_packets() + [packet(AUDIO_PID, too_long, start=True, cc=0), packet(AUDIO_PID, rng.bytes(184), cc=1)] +
        carry(AUDIO_PID, pes(rng.bytes(100)), cc=2))
    ids = []
    for sid in (0xBF, 0xC0, 0xDF, 0xE0):
        ids += carry(AUDIO_PID, pes(rng.bytes(200), stream_id=sid, pts=sid), cc=len(ids))
    put("stream_ids", head_packets() + ids)
    put("bad_marker_and_prefix", head_packets() + carry(AUDIO_PID, pes(rng.bytes(200), marker=0x40)) + carry(AUDIO_PID, b"\x00\x00\x02" + pes(rng.bytes(90))[3:], cc=2) +
        carry(AUDIO_PID, pes(rng.bytes(5))[:8], cc=3) + carry(AUDIO_PID, pes(rng.bytes(30), stuffing=3, length=5), cc=4) + carry(AUDIO_PID, pes(rng.bytes(77)), cc=5))
    put("length_zero", head_packets() + carry(AUDIO_PID, pes(rng.bytes(500), length=0)) + carry(AUDIO_PID, pes(rng.bytes(100), length=0), cc=3))
    short = pes(rng.bytes(400), pts=1, length=3 + 5 + 250)              # N 150 short of what arrives
    beyond = pes(rng.bytes(400), pts=2, length=3 + 5 + 900)             # N 500 beyond it
    nxt = carry(AUDIO_PID, pes(rng.bytes(60)), cc=6)
    put("length_short_before_start", head_packets() + carry(AUDIO_PID, short) + nxt)
    put("length_short_at_end", head_packets() + carry(AUDIO_PID, short))
    put("length_beyond_before_start", head_packets() + carry(AUDIO_PID, beyond) + nxt)
    put("length_beyond_at_end", head_packets() + carry(AUDIO_PID, beyond))
    lead = [packet(AUDIO_PID, rng.bytes(184), cc=3), packet(AUDIO_PID, rng.bytes(100), cc=4)]
    rest = carry(AUDIO_PID, pes(rng.bytes(300), pts=9), cc=5)
    put("before_first_start_dropped", lead + rest, audio_pid=AUDIO_PID)
    put("before_first_start_open", lead + rest, audio_pid=AUDIO_PID, flags=TX.PES_OPEN, pes_open_bytes=284)
    put("before_first_start_open_more", lead + rest, audio_pid=AUDIO_PID, flags=TX.PES_OPEN, pes_open_bytes=1000)
    put("before_first_start_open_less", lead + rest, audio_pid=AUDIO_PID, flags=TX.PES_OPEN, pes_open_bytes=200)
    put("before_first_start_open_unbounded", lead + rest, audio_pid=AUDIO_PID, flags=TX.PES_OPEN, pes_open_bytes=0xFFFFFFFF)
    put("open_and_no_start", lead, audio_pid=AUDIO_PID, flags=TX.PES_OPEN, pes_open_bytes=5000)
    put("open_and_no_audio", [psi(0, pat())], audio_pid=AUDIO_PID, flags=TX.PES_OPEN, pes_open_bytes=77)
    put("open_and_a_start_first", rest, audio_pid=AUDIO_PID, flags=TX.PES_OPEN, pes_open_bytes=77)
    jumpy = carry(AUDIO_PID, pes(rng.bytes(700), pts=3), cc=0)           # counters 0..3
    jumpy[2] = jumpy[2][:3] + bytes([jumpy[2][3] & 0xF0 | 9]) + jumpy[2][4:]   # a jump (and the one behind it jumps back)
    again = carry(AUDIO_PID, pes(rng.bytes(300), pts=4), cc=3)           # a repeated counter on a start
    no_payload = packet(AUDIO_PID, b"", adaptation=183, payload_bit=False, cc=5)
    put("counter_jumps", head_packets() + jumpy + again + [no_payload] + carry(AUDIO_PID, pes(rng.bytes(10)), cc=5))
    put("no_room_for_records", head_packets() + audio_run(rng, n_pes=4)[0], pes_capacity=0)
    put("little_room_for_records", head_packets() + audio_run(rng, n_pes=4)[0], pes_capacity=2)
    # ---- T1 among good packets
    a, es = audio_run(rng, n_pes=2)
    mixed = head_packets() + [a[0], packet(AUDIO_PID, rng.bytes(184), cc=1, sync=0x48), a[1], packet(AUDIO_PID, rng.bytes(184), cc=2, tei=True),
                              packet(AUDIO_PID, rng.bytes(184), cc=2, scrambling=2), packet(OTHER_PID, rng.bytes(184), cc=0)] + a[2:]
    put("skipped_kinds", mixed, es=es)
    put("start_without_payload", head_packets() + [packet(AUDIO_PID, b"", adaptation=183, payload_bit=False, start=True)] + audio_run(rng, cc=0)[0])
    return out


# ---------------------------------------------------------------- the named streams of layer 2
def adts_named():
    rng = Lcg(77)
    out = {}
    frames = [adts_frame(clean(rng.bytes(n)), protection_absent=bool(k % 3)) for k, n in enumerate((0, 100, 371, 0, 64, 2, 500))]
    out["plain"] = adts_stream(b"".join(frames))
    out["seven_and_nine"] = adts_stream(adts_frame(b"") + adts_frame(b"", protection_absent=False) + adts_frame(b"z"))
    out["largest"] = adts_stream(adts_frame(clean(rng.bytes(8191 - 7))) + adts_frame(b"abc"))
    whole = b"".join(frames[:3])
    out["ends_with_last_byte"] = adts_stream(whole)
    out["one_byte_short"] = adts_stream(whole[:-1])
    out["six_left_over"] = adts_stream(whole + frames[3][:6])
    out["seven_left_over"] = adts_stream(whole + frames[4][:7])
    junk = clean(rng.bytes(40)) + adts_frame(b"", sf_index=13)[:7] + clean(rng.bytes(9)) + adts_frame(b"", layer=1)[:7] + b"\x00" + adts_frame(b"", length=6)[:7] + \
        adts_frame(b"", blocks=1)[:7] + clean(rng.bytes(3))
    out["junk_between"] = adts_stream(frames[1] + junk + frames[2] + frames[4] + junk[:50] + frames[5])
    out["junk_at_the_end"] = adts_stream(frames[1] + clean(rng.bytes(100)))
    out["nothing_valid"] = adts_stream(clean(rng.bytes(3000)))
    out["empty"] = adts_stream(b"")
    out["short"] = adts_stream(frames[1][:6])
    # frame starts on both sides of a word of the map (32), a wave's and a lane-step's reach (64, 2048), a workgroup's tile (1024), after a search
    for edge in (32, 64, 256, 1024, 2048, 4096):
        for at in (edge - 1, edge, edge + 1):
            out[f"start_at_{at}"] = adts_stream(clean(rng.bytes(at)) + frames[2] + frames[5])
    for edge in (64, 1024, 2048):                                      # ... and reached by the chain itself, without a search
        for at in (edge - 1, edge, edge + 1):
            out[f"chained_to_{at}"] = adts_stream(adts_frame(clean(rng.bytes(at - 7))) + frames[2] + frames[5])
    out["little_room"] = adts_stream(b"".join(frames), frame_capacity=3)
    out["no_room"] = adts_stream(b"".join(frames), frame_capacity=0)
    # ---- recognition
    five = [adts_frame(clean(rng.bytes(n)), profile=2, sf_index=3, channels=1) for n in (30, 41, 52, 63, 74, 85, 96)]
    out["recognise_at_0"] = adts_stream(b"".join(five), flags=TX.RECOGNISE)
    out["recognise_four_then_five"] = adts_stream(b"".join(frames[:4]) + clean(rng.bytes(33)) + b"".join(five), flags=TX.RECOGNISE)
    out["recognise_at_1001"] = adts_stream(clean(rng.bytes(1001)) + b"".join(five), flags=TX.RECOGNISE)
    out["recognise_at_1002"] = adts_stream(clean(rng.bytes(1002)) + b"".join(five), flags=TX.RECOGNISE)
    out["recognise_nothing"] = adts_stream(clean(rng.bytes(1500)), flags=TX.RECOGNISE)
    out["recognise_fifth_lacks_ten"] = adts_stream(b"".join(five[:4]) + five[4][:9], flags=TX.RECOGNISE)
    out["recognise_fifth_has_ten"] = adts_stream(b"".join(five[:4]) + five[4][:10], flags=TX.RECOGNISE)
    out["recognise_little_room"] = adts_stream(clean(rng.bytes(70)) + b"".join(five), flags=TX.RECOGNISE, frame_capacity=2)
    return out


def fnv1a32(data):
    h = 2166136261
    for b in data:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def segment(rng, n_frames, frames_per_pes=4, cc=0, tables_every=6, payload=(90, 260)):
    """An HLS-like segment: ADTS frames, frames_per_pes to a PES packet with a PTS, the PAT and the PMT again every tables_every PES
    packets, and a packet of another PID now and then.  Returns (packets, the elementary bytes)."""
    frames = [adts_frame(rng.bytes(payload[0] + rng.below(payload[1] - payload[0])), profile=1, sf_index=4, channels=2) for _ in range(n_frames)]
    out, es, k = [], b"", 0
    for a in range(0, n_frames, frames_per_pes):
        if (a // frames_per_pes) % tables_every == 0:
            out += head_packets(cc=a // frames_per_pes // tables_every)
        part = b"".join(frames[a:a + frames_per_pes])
        got = carry(AUDIO_PID, pes(part, pts=(a * 1024 * 90000 // 44100) & 0x1FFFFFFFF), cc=cc + k)
        k += len(got)
        out += got
        es += part
        if a % 3 == 0:
            out.append(packet(OTHER_PID, rng.bytes(184), cc=a))
    return out, es


def phases_job():
    """Sixteen streams whose src_offset takes every value mod 16, each delivering to a dst_offset that walks through every value mod 16
    against it in sixteen jobs' worth of pairs: stream i of round r starts at source phase i and destination phase (i + r) % 16."""
    rng = Lcg(16)
    streams, src_phase, dst_phase = [], [], []
    for r in range(16):
        for i in range(16):
            packets, _ = segment(rng, 3, frames_per_pes=2, payload=(20, 60))
            streams.append(stream(b"".join(packets)))
            src_phase.append(i)
            dst_phase.append((i + r) % 16)
    job = Job(streams, src_phase=src_phase, dst_phase=dst_phase)
    seen = {(int(d["src_offset"]) % 16, int(d["dst_offset"]) % 16) for d in job.descs}
    assert seen == {(a, b) for a in range(16) for b in range(16)}
    assert all(m["status"] == TX.OK and len(m["run"]) > 60 for m in job.models)
    return job


def long_stream(rng, n_packets):
    """A stream of n_packets packets for the sums' tiles (256 packets each): PES packets of 1-9 packets drawn from a few payloads, the
    tables again now and then, a counter jump and a bad start among them."""
    pool = [rng.bytes(184) for _ in range(12)]
    out, cc, k = head_packets(), 0, 0
    while len(out) < n_packets:
        n = 1 + rng.below(9)
        es = b"".join(pool[rng.below(len(pool))] for _ in range(n))[:n * 184 - 20 - rng.below(150)]
        kind = rng.below(40)
        data = pes(es, pts=k * 1920, length=0 if kind == 1 else "right", stream_id=0xBD if kind == 2 else 0xC1)
        got = carry(AUDIO_PID, data, cc=cc + (3 if kind == 3 else 0))
        cc += len(got) + (3 if kind == 3 else 0)
        out += got
        k += 1
        if k % 25 == 0:
            out += head_packets(cc=k)
    return b"".join(out[:n_packets])
