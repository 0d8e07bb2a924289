"""An independent model of the MPEG transport stream demultiplexer and the ADTS frame table (include/ohgpu_ts.h: T1-T5, P1-P5, A1-A3):
plain Python, serial, a packet at a time with the state a reader would keep -- written from the rules, not from csrc/ts_packet_core.h
(which has no such state: it scans an operator).  TEST INFRASTRUCTURE ONLY."""

PACKET = 188
NONE, NO_PTS, UNBOUNDED = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
OK, NO_PAT, NO_PMT, NO_AUDIO, CORRUPT = range(5)
PES_OPEN = 1
CONTINUATION, EXCESS, TRUNCATED, CC_JUMP = 1, 2, 4, 8
ADTS_OK, NOT_ADTS = 0, 1
RECOGNISE, INTERRUPTED = 1, 1


def crc(data, start=0xFFFFFFFF):
    c = start
    for b in data:
        c ^= b << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
    return c


def _section(payload, table_id, least):
    """The section behind the pointer field, checks passed, CRC right; or None."""
    if len(payload) < 1:
        return None
    at = 1 + payload[0]
    if at + 3 > len(payload):
        return None
    head = payload[at:at + 3]
    if head[0] != table_id or head[1] & 0x80 != 0x80 or head[1] & 0x40 or head[1] & 0x30 != 0x30 or head[1] & 0x0C:
        return None
    length = (head[1] & 3) << 8 | head[2]
    if length > 1021 or length < least or at + 3 + length > len(payload):
        return None
    sec = payload[at:at + 3 + length]
    if sec[5] & 0xC0 != 0xC0 or crc(sec) != 0:
        return None
    return sec


def pat_pid(payload):
    sec = _section(payload, 0, 9)
    if sec is None:
        return None
    for e in range(8, len(sec) - 4 - 3, 4):
        if sec[e + 2] & 0xE0 != 0xE0:
            return None
        if sec[e] << 8 | sec[e + 1]:
            pid = (sec[e + 2] & 0x1F) << 8 | sec[e + 3]
            return pid or None
    return None


def pmt_audio_pid(payload):
    """None: no valid PMT; 0: a valid one without a stream of type 0x0f."""
    sec = _section(payload, 2, 13)
    if sec is None:
        return None
    if sec[8] & 0xE0 != 0xE0 or sec[10] & 0xF0 != 0xF0 or sec[10] & 0x0C:
        return None
    end = len(sec) - 4
    e = 12 + ((sec[10] & 3) << 8 | sec[11])
    if e > end:
        return None
    while e < end:
        if end - e < 5 or sec[e + 1] & 0xE0 != 0xE0 or sec[e + 3] & 0xF0 != 0xF0 or sec[e + 3] & 0x0C:
            return None
        if sec[e] == 0x0F:
            return (sec[e + 1] & 0x1F) << 8 | sec[e + 2]
        e += 5 + ((sec[e + 3] & 3) << 8 | sec[e + 4])
        if e > end:
            return None
    return 0


def pes_head(payload):
    """(header bytes, expected elementary bytes or None, pts, stream id) of a good start, else None."""
    if len(payload) < 9 or payload[:3] != b"\x00\x00\x01" or not 0xC0 <= payload[3] <= 0xDF or payload[6] & 0xC0 != 0x80:
        return None
    n, h = payload[4] << 8 | payload[5], payload[8]
    if 9 + h > len(payload) or (n and n < 3 + h):
        return None
    pts = NO_PTS
    if payload[7] & 0x80 and h >= 5:
        b = payload[9:14]
        pts = ((b[0] >> 1) & 7) << 30 | b[1] << 22 | (b[2] >> 1) << 15 | b[3] << 7 | b[4] >> 1
    return 9 + h, (n - 3 - h if n else None), pts, payload[3]


def demux(data, flags=0, pmt_pid=0, audio_pid=0, pes_open_bytes=0):
    data = bytes(data)
    n_packets = len(data) // PACKET
    r = dict(status=OK, trailing_bytes=len(data) % PACKET, packets=n_packets, bad_sync=0, tei_packets=0, scrambled_packets=0, pat_packet=NONE, pmt_packet=NONE,
             pmt_pid=pmt_pid, audio_pid=audio_pid, audio_packets=0, bad_pes_starts=0, dropped_bytes=0, cc_jumps=0, pes_open_bytes=0, corrupt_packet=NONE)
    looking = "audio" if audio_pid else ("pmt" if pmt_pid else "pat")
    run, records, cur, last_cc = bytearray(), [], None, None
    for k in range(n_packets):
        p = data[k * PACKET:(k + 1) * PACKET]
        if p[0] != 0x47:
            r["bad_sync"] += 1
            continue
        if p[1] & 0x80:
            r["tei_packets"] += 1
            continue
        if p[3] & 0xC0:
            r["scrambled_packets"] += 1
            continue
        at = 4
        if p[3] & 0x20:
            if p[4] > 183:
                r["corrupt_packet"] = k
                break
            at = 5 + p[4]
        payload = p[at:] if p[3] & 0x10 else b""
        pid, start = (p[1] & 0x1F) << 8 | p[2], bool(p[1] & 0x40)
        if looking == "pat":
            got = pat_pid(payload) if pid == 0 and start else None
            if got is not None:
                r["pat_packet"], r["pmt_pid"], looking = k, got, "pmt"
            continue
        if looking == "pmt":
            got = pmt_audio_pid(payload) if pid == r["pmt_pid"] and start else None
            if got is not None:
                r["pmt_packet"], r["audio_pid"], looking = k, got, "audio"
            continue
        if not r["audio_pid"] or pid != r["audio_pid"]:
            continue
        # ---- an audio packet
        first = r["audio_packets"] == 0
        r["audio_packets"] += 1
        jump = False
        if p[3] & 0x10:
            jump = last_cc is not None and p[3] & 15 != (last_cc + 1) & 15
            last_cc = p[3] & 15
        if start:
            _close(cur, True)
            head = pes_head(payload)
            if head is None:
                r["bad_pes_starts"] += 1
                cur, es = dict(rec=None, expect=0, got=0), payload
            else:
                rec = dict(es_offset=len(run), bytes=0, packet=k, pts=head[2], flags=0, stream_id=head[3])
                records.append(rec)
                cur, es = dict(rec=rec, expect=head[1], got=0), payload[head[0]:]
        else:
            if cur is None and first and flags & PES_OPEN:
                rec = dict(es_offset=0, bytes=0, packet=k, pts=NO_PTS, flags=CONTINUATION, stream_id=0)
                records.append(rec)
                cur = dict(rec=rec, expect=None if pes_open_bytes == UNBOUNDED else pes_open_bytes, got=0)
            elif cur is None:
                cur = dict(rec=None, expect=0, got=0)
            es = payload
        if jump:
            r["cc_jumps"] += 1
            if cur["rec"] is not None:
                cur["rec"]["flags"] |= CC_JUMP
        take = len(es) if cur["expect"] is None else max(0, min(len(es), cur["expect"] - cur["got"]))
        run += es[:take]
        cur["got"] += len(es)
        r["dropped_bytes"] += len(es) - take
        if cur["rec"] is not None:
            cur["rec"]["bytes"] += take
    _close(cur, False)
    if r["audio_packets"] == 0:
        r["pes_open_bytes"] = pes_open_bytes if flags & PES_OPEN else 0
    elif cur["rec"] is not None:
        r["pes_open_bytes"] = UNBOUNDED if cur["expect"] is None else max(0, cur["expect"] - cur["got"])
    if r["corrupt_packet"] != NONE:
        r["status"] = CORRUPT
    elif not r["audio_pid"]:
        r["status"] = NO_AUDIO if r["pmt_packet"] != NONE else (NO_PMT if r["pmt_pid"] else NO_PAT)
    r["pes"], r["run"] = records, bytes(run)
    return r


def _close(cur, before_start):
    if cur is None or cur["rec"] is None or cur["expect"] is None:
        return
    if cur["got"] > cur["expect"]:
        cur["rec"]["flags"] |= EXCESS
    elif cur["got"] < cur["expect"] and before_start:
        cur["rec"]["flags"] |= TRUNCATED


# ---------------------------------------------------------------- ADTS
def adts_header(b):
    """dict(bytes, header_bytes, profile, sf_index, channel_config) of a valid header at the head of b, else None."""
    if len(b) < 7 or b[0] != 0xFF or b[1] & 0xF0 != 0xF0 or b[1] & 0x06:
        return None
    header_bytes = 7 if b[1] & 1 else 9
    sf = (b[2] >> 2) & 15
    length = (b[3] & 3) << 11 | b[4] << 3 | b[5] >> 5
    if sf > 12 or length < header_bytes or b[6] & 3:
        return None
    return dict(bytes=length, header_bytes=header_bytes, profile=b[2] >> 6, sf_index=sf, channel_config=(b[2] & 1) << 2 | b[3] >> 6)


def adts_recognise(data):
    """(start, mean payload bytes) or None."""
    for p in range(0, 1002):
        j, payload = p, 0
        for _ in range(5):
            h = adts_header(data[j:j + 10]) if j + 10 <= len(data) else None
            if h is None:
                break
            payload += h["bytes"] - h["header_bytes"]
            j += h["bytes"]
        else:
            return p, payload // 5
    return None


def adts_chain(data, flags=0):
    data = bytes(data)
    r = dict(status=ADTS_OK, bytes_consumed=0, first_frame_offset=0, interruptions=0, skipped_bytes=0, mean_payload_bytes=0, profile=0, sf_index=0, channel_config=0)
    frames, p = [], 0
    if flags & RECOGNISE:
        got = adts_recognise(data)
        if got is None:
            r["status"], r["frames"] = NOT_ADTS, frames
            return r
        p, r["mean_payload_bytes"] = got
        h = adts_header(data[p:p + 7])
        r.update(first_frame_offset=p, profile=h["profile"], sf_index=h["sf_index"], channel_config=h["channel_config"])
    interrupted = False
    while p + 7 <= len(data):
        h = adts_header(data[p:p + 7])
        if h is None:
            p += 1
            r["skipped_bytes"] += 1
            interrupted = True
            continue
        if p + h["bytes"] > len(data):
            break
        if not frames and not flags & RECOGNISE:
            r.update(first_frame_offset=p, profile=h["profile"], sf_index=h["sf_index"], channel_config=h["channel_config"])
        frames.append(dict(h, offset=p, flags=INTERRUPTED if interrupted else 0))
        r["interruptions"] += interrupted
        interrupted = False
        p += h["bytes"]
    r["bytes_consumed"], r["frames"] = p, frames
    return r


def id3v2_skip(data):
    at = 0
    while len(data) - at >= 10:
        t = data[at:at + 10]
        if t[:3] != b"ID3" or t[3] == 0xFF or t[4] == 0xFF or any(x & 0x80 for x in t[6:10]):
            break
        at += 10 + (t[6] << 21 | t[7] << 14 | t[8] << 7 | t[9]) + (10 if t[5] & 0x10 else 0)
        if at > len(data):
            break
    return at
