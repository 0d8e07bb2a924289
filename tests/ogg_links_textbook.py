"""An independent model of the chained-stream rules L1-L5 (include/ohgpu.h, the Ogg section) on top of rules 1-7, written from that
text and not from csrc/ogg_page_core.h.  It does not walk with a state: it looks for the pages that begin a link, cuts the byte
string there, gives every part to the plain model (tests/ogg_textbook.py: a part of one link is a plain stream of one serial whose
first page may carry any number), and joins what comes back.  A packet open where a part ends is not delivered by the plain model,
which is rule L2's "dropped"."""
import ogg_textbook as OX

FOLLOW_LINKS = 16
PACKET_LINK = 8
VORBIS_MAGIC, FLAC_MAGIC = b"\x01vorbis", b"\x7fFLAC"
MASK = 0xFFFFFFFF


def whole_page(data, p):
    """The page at p as a dict, or None where rule 1 or rule 2 ends the walk."""
    if len(data) - p < 27 or data[p:p + 4] != b"OggS":
        return None
    n = data[p + 26]
    if len(data) - p < 27 + n:
        return None
    size = 27 + n + sum(data[p + 27:p + 27 + n])
    if len(data) - p < size:
        return None
    page = data[p:p + size]
    if OX.page_crc(page) != int.from_bytes(page[22:26], "little"):
        return None
    return dict(size=size, version=page[4], flags=page[5], serial=int.from_bytes(page[14:18], "little"), seq=int.from_bytes(page[18:22], "little"),
                body=page[27 + n:])


def demux(data, serial=0, expect_seq=0, first_page_segment=0, flags=0, magic=b""):
    """ogg_textbook.demux's dict with `links`; without FOLLOW_LINKS it is that function's answer and links = 0."""
    data = bytes(data)
    plain = flags & ~FOLLOW_LINKS
    if not flags & FOLLOW_LINKS:
        return dict(OX.demux(data, serial, expect_seq, first_page_segment, plain), links=0)
    assert len(magic) <= 8
    parts = []                                           # (where the part begins, the plain model's answer, what a later call's expect_seq would be at its end)
    start, args = 0, dict(serial=serial, expect_seq=expect_seq, first_page_segment=first_page_segment, flags=plain)
    followed = None if flags & OX.ANY_SERIAL else serial
    while True:
        q, last_was_first, expect, cut = start, False, args["expect_seq"], None
        while cut is None:
            pg = whole_page(data, q)
            if pg is None:
                break
            if followed is None:
                followed = pg["serial"]
            if pg["serial"] == followed:
                if pg["version"] == 0:                   # an accepted page, if the walk gets here at all
                    last_was_first, expect = bool(pg["flags"] & OX.BOS), (pg["seq"] + 1) & MASK
            elif pg["version"] == 0 and (pg["flags"] & OX.BOS) and not last_was_first and pg["body"][:len(magic)] == magic:
                before = OX.demux(data[start:q], **args)
                if before["status"] != OX.OK:            # the walk stopped in front of it
                    break
                cut = (q, before, pg["serial"])
                break
            q += pg["size"]
        if cut is None:
            parts.append((start, OX.demux(data[start:], **args), None))
            break
        parts.append((start, cut[1], expect))
        start, followed = cut[0], cut[2]
        args = dict(serial=followed, expect_seq=0, first_page_segment=0, flags=(plain & OX.FLAC_MAPPING) | OX.ANY_SEQ)
    rolled_back = None
    if len(parts) > 1 and parts[-1][1]["status"] == OX.OK and not parts[-1][1]["packets"]:      # L4: the later call's to find
        rolled_back = parts.pop()[0]
    packets = []
    for k, (at, part, _) in enumerate(parts):
        for j, pk in enumerate(part["packets"]):
            packets.append(dict(pk, page_offset=pk["page_offset"] + at, flags=pk["flags"] | (PACKET_LINK if k and j == 0 else 0)))
    pos = 0
    for pk in packets:
        pk["run_pos"] = pos
        pos += pk["bytes"]
    at, last, _ = parts[-1]
    granules = [pk["granule"] for pk in packets if pk["granule"] != -1]
    out = dict(status=last["status"], pages=sum(p["pages"] for _, p, _ in parts), pages_ignored=sum(p["pages_ignored"] for _, p, _ in parts),
               bytes_consumed=at + last["bytes_consumed"], resume_segment=last["resume_segment"], next_seq=last["next_seq"], serial=last["serial"],
               bos_seen=max(p["bos_seen"] for _, p, _ in parts), eos_seen=max(p["eos_seen"] for _, p, _ in parts), links=len(parts) - 1,
               packets=packets, run=b"".join(pk["data"] for pk in packets), last_granule=granules[-1] if granules else -1)
    if rolled_back is not None:
        out.update(bytes_consumed=rolled_back, resume_segment=0, next_seq=parts[-1][2])
    return out
