"""An independent model of the Ogg page layer (include/ohgpu.h, the Ogg section; RFC 3533), written from those two texts and not from
csrc/ogg_page_core.h.  It works the other way round: a page is cut out of the byte string whole, its checksum is taken over a copy
with the field blanked, its segments are put on a list, and a packet is the joined bytes of the segments on that list once one below
255 arrives.  Nothing streams, nothing is planned; the run is the concatenation of the packets' bytes."""

OK, LOST_SYNC, HOLE, NOT_FLAC, UNSUPPORTED_MAPPING, BAD_RESUME = range(6)
ANY_SEQ, FLAC_MAPPING, ANY_SERIAL = 1, 2, 4
CONTINUED, BOS, EOS = 1, 2, 4
PACKET_BOS, PACKET_EOS, PACKET_MAPPING_HEADER = 1, 2, 4
POLY = 0x04C11DB7


def crc_bitwise(data):
    """The definition: a 32-bit register, zero at the start, message bits in from the top, most significant first."""
    reg = 0
    for byte in data:
        for k in range(7, -1, -1):
            feedback = (reg >> 31) ^ ((byte >> k) & 1)
            reg = (reg << 1) & 0xFFFFFFFF
            if feedback:
                reg ^= POLY
    return reg


_TABLE = [crc_bitwise(bytes([i])) for i in range(256)]


def crc(data):
    """The same function a byte at a time (a single byte's register is its table entry; tests hold it to crc_bitwise)."""
    reg = 0
    for byte in data:
        reg = ((reg << 8) & 0xFFFFFFFF) ^ _TABLE[(reg >> 24) ^ byte]
    return reg


def page_crc(page):
    return crc(page[:22] + bytes(4) + page[26:])


def demux(data, serial=0, expect_seq=0, first_page_segment=0, flags=0):
    """The walk over one stream's bytes.  Returns a dict: the result's fields, `packets` (dicts with the record's fields and `data`)
    and `run`."""
    data = bytes(data)
    stream_serial = None if flags & ANY_SERIAL else serial
    expect = None if flags & ANY_SEQ else expect_seq
    status, p, pages, ignored = OK, 0, 0, 0
    first, bos_seen, eos_seen = True, 0, 0
    packets, pending, begun = [], [], None          # pending: (offset, length) of the open packet's segments; begun: where it began
    while True:
        left = len(data) - p
        if left < 27:
            break
        if data[p:p + 4] != b"OggS":
            status = LOST_SYNC
            break
        n = data[p + 26]
        if left < 27 + n:
            break
        lacing = list(data[p + 27:p + 27 + n])
        size = 27 + n + sum(lacing)
        if left < size:
            break
        page = data[p:p + size]
        if page_crc(page) != int.from_bytes(page[22:26], "little"):
            status = LOST_SYNC
            break
        version, page_flags = page[4], page[5]
        granule = int.from_bytes(page[6:14], "little", signed=True)
        page_serial, seq = int.from_bytes(page[14:18], "little"), int.from_bytes(page[18:22], "little")
        if stream_serial is None:
            stream_serial = page_serial
        if page_serial != stream_serial or version != 0:
            ignored += 1
            p += size
            continue
        if expect is not None and seq != expect:
            status = HOLE
            break
        start = 0
        if first and first_page_segment > 0:
            if first_page_segment > n:
                status = BAD_RESUME
                break
            start = first_page_segment
        elif (page_flags & CONTINUED) and not pending:
            start = next((i + 1 for i, v in enumerate(lacing) if v < 255), n)
        fresh_page = start == 0                       # nothing of the page was passed over
        first, expect, pages = False, (seq + 1) & 0xFFFFFFFF, pages + 1
        bos_seen |= 1 if page_flags & BOS else 0
        eos_seen |= 1 if page_flags & EOS else 0
        if (page_flags & EOS) and n == 0 and pending:
            begun["flags"] |= PACKET_EOS
        offsets = [p + 27 + n + sum(lacing[:i]) for i in range(n)]
        ended_here, stop = [], False
        for i in range(start, n):
            if not pending:
                begun = dict(page_offset=p, page_seq=seq, segment=i, flags=PACKET_BOS if (page_flags & BOS) and i == 0 and fresh_page else 0)
            pending.append((offsets[i], lacing[i]))
            if (page_flags & EOS) and i == n - 1:
                begun["flags"] |= PACKET_EOS
            if lacing[i] == 255:
                continue
            body = b"".join(data[a:a + l] for a, l in pending)
            if (flags & FLAC_MAPPING) and body[:1] == b"\x7f":
                if len(body) < 9 or body[1:5] != b"FLAC":
                    status = NOT_FLAC
                elif body[5] != 1:
                    status = UNSUPPORTED_MAPPING
                if status != OK:
                    stop = True
                    break
                body = body[9:]
                begun["flags"] |= PACKET_MAPPING_HEADER
            packets.append(dict(begun, data=body, granule=-1))
            ended_here.append(packets[-1])
            pending, begun = [], None
        if stop:
            break
        if ended_here:
            ended_here[-1]["granule"] = granule
        p += size
    out = dict(status=status, pages=pages, pages_ignored=ignored, bytes_consumed=p, resume_segment=0,
               next_seq=expect_seq if expect is None else expect, serial=serial if stream_serial is None else stream_serial,
               bos_seen=bos_seen, eos_seen=eos_seen)
    if status == OK and pending:
        out.update(bytes_consumed=begun["page_offset"], resume_segment=begun["segment"], next_seq=begun["page_seq"])
    at = 0
    for k in packets:
        k["run_pos"], k["bytes"] = at, len(k["data"])
        at += len(k["data"])
    granules = [k["granule"] for k in packets if k["granule"] != -1]
    out.update(packets=packets, run=b"".join(k["data"] for k in packets), last_granule=granules[-1] if granules else -1)
    return out
