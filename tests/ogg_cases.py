"""What the Ogg page layer's tests share: a test-side page writer and muxer, the named sessions, and a Job -- streams laid into a
source arena allocated to the byte and a destination arena of FILL with guard bytes round every run, the descriptors, and what the
model (tests/ogg_textbook.py) says the results, the packet table and the destination arena must be."""
import gzip
import json
import os

import numpy as np

import ogg_textbook as OX

FILL, GUARD = 0xA5, 24
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ogg")


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


def page(serial, seq, lacing, body, flags=0, granule=0, version=0, bad_crc=False):
    assert len(lacing) <= 255 and sum(lacing) == len(body)
    head = b"OggS" + bytes([version, flags]) + int(granule).to_bytes(8, "little", signed=True) + serial.to_bytes(4, "little") + \
        (seq & 0xFFFFFFFF).to_bytes(4, "little") + bytes(4) + bytes([len(lacing)]) + bytes(lacing)
    c = OX.crc(head + body) ^ (1 if bad_crc else 0)
    return head[:22] + c.to_bytes(4, "little") + head[26:] + body


def lacing_of(n):
    return [255] * (n // 255) + [n % 255]


def mux(packets, serial, seq0=0, max_segments=255, granules=None, bos=True, eos=True):
    """Packets -> pages of up to max_segments segments: "continued" where a page starts inside a packet, the granule position of the
    last packet that ends on a page (-1 where none does)."""
    segs = []                                           # (value, bytes, packet index or None while the packet goes on)
    for k, data in enumerate(packets):
        lace, at = lacing_of(len(data)), 0
        for j, v in enumerate(lace):
            segs.append((v, data[at:at + v], k if j == len(lace) - 1 else None))
            at += v
    pages, seq = [], seq0
    for a in range(0, max(len(segs), 1), max_segments):
        part = segs[a:a + max_segments]
        ended = [k for _, _, k in part if k is not None]
        g = -1 if not ended else (granules[ended[-1]] if granules else ended[-1] + 1)
        f = (OX.CONTINUED if a > 0 and segs[a - 1][0] == 255 else 0) | (OX.BOS if bos and a == 0 else 0) | (OX.EOS if eos and a + max_segments >= len(segs) else 0)
        pages.append(page(serial, seq, [v for v, _, _ in part], b"".join(d for _, d, _ in part), f, g))
        seq += 1
    return pages


def page_of_size(size, serial, seq, rng, flags=0):
    """One page of exactly `size` bytes: one packet, and an empty one behind it where one packet cannot make the size."""
    if size == 27:
        return page(serial, seq, [], b"", flags)
    if size == 65307:                                   # the largest: 255 segments of 255 bytes, a packet that goes on
        return page(serial, seq, [255] * 255, rng.bytes(255 * 255), flags, granule=-1)
    for zeros in (0, 1):
        for body in range(max(size - 27 - 256 - zeros, 0), size - 27):
            lace = lacing_of(body) + [0] * zeros
            if 27 + len(lace) + body == size and len(lace) <= 255:
                return page(serial, seq, lace, rng.bytes(body), flags, granule=seq)
    raise AssertionError(size)


def stream(data, serial=0, expect_seq=0, first_page_segment=0, flags=0, packet_capacity=None):
    return dict(data=bytes(data), serial=serial, expect_seq=expect_seq, first_page_segment=first_page_segment, flags=flags, packet_capacity=packet_capacity)


RESULT_FIELDS = ("status", "pages", "pages_ignored", "bytes_consumed", "resume_segment", "next_seq", "last_granule", "serial", "bos_seen", "eos_seen")
PACKET_FIELDS = ("run_pos", "bytes", "flags", "granule", "page_offset", "page_seq", "segment")


class Job:
    def __init__(self, streams, seed=5):
        from ohpipeline_amd import capi
        rng = Lcg(seed)
        self.streams = streams
        self.models = [OX.demux(s["data"], s["serial"], s["expect_seq"], s["first_page_segment"], s["flags"]) for s in streams]
        n = len(streams)
        self.descs = np.zeros(n, dtype=capi.OGG_STREAM_DESC)
        src, dst_at, pk_at = bytearray(), GUARD, 0
        for i, (s, m) in enumerate(zip(streams, self.models)):
            if i:
                src += rng.bytes(1 + rng.below(7))                      # streams at every alignment, junk between them
            d = self.descs[i]
            cap = len(m["packets"]) if s["packet_capacity"] is None else s["packet_capacity"]
            d["src_offset"], d["src_bytes"], d["dst_offset"], d["dst_capacity"] = len(src), len(s["data"]), dst_at, len(s["data"])
            d["serial"], d["expect_seq"], d["first_page_segment"], d["flags"] = s["serial"], s["expect_seq"], s["first_page_segment"], s["flags"]
            d["packet_first"], d["packet_capacity"] = pk_at, cap
            src += s["data"]
            dst_at += len(s["data"]) + GUARD + rng.below(5)
            pk_at += cap + (i % 2)                                      # (a gap in the table now and then)
        self.src = np.frombuffer(bytes(src), dtype=np.uint8) if src else np.zeros(0, dtype=np.uint8)
        self.n_packets = pk_at
        self.dst0 = np.full(dst_at if n else 0, FILL, dtype=np.uint8)
        self.want = self.dst0.copy()
        for d, m in zip(self.descs, self.models):
            a = int(d["dst_offset"])
            self.want[a:a + len(m["run"])] = np.frombuffer(m["run"], dtype=np.uint8)

    def driver_blob(self):
        head = np.array([len(self.streams), self.n_packets, self.src.size, self.dst0.size], dtype="<u8")
        return head.tobytes() + self.descs.tobytes() + self.src.tobytes() + self.dst0.tobytes()


def assert_same(results, packets, arena, job):
    """Every result, every record a stream has room for, and the whole destination arena are the model's."""
    arena = np.frombuffer(bytes(arena), dtype=np.uint8)
    for i, (d, m) in enumerate(zip(job.descs, job.models)):
        r = results[i]
        got = {f: int(r[f]) for f in RESULT_FIELDS}
        assert got == {f: m[f] for f in RESULT_FIELDS}, (i, got, {f: m[f] for f in RESULT_FIELDS})
        assert int(r["packets"]) == len(m["packets"]) and int(r["bytes_delivered"]) == len(m["run"]), i
        first, cap = int(d["packet_first"]), int(d["packet_capacity"])
        for k, want in enumerate(m["packets"][:cap]):
            rec = packets[first + k]
            assert {f: int(rec[f]) for f in PACKET_FIELDS} == {f: want[f] for f in PACKET_FIELDS}, (i, k)
    bad = np.flatnonzero(arena != job.want)
    assert bad.size == 0, f"{bad.size} of {job.want.size} destination bytes differ, first at {bad[:8].tolist()}"


# ---- the named sessions: every rule of the walk at least once (each returns the keyword arguments of stream())
def sessions():
    rng = Lcg(2024)
    out = {}
    sizes = [0, 1, 254, 255, 256, 510, 65025 + 3]
    out["sizes"] = stream(b"".join(mux([rng.bytes(n) for n in sizes], 7)), serial=7)
    out["three_pages"] = stream(b"".join(mux([rng.bytes(10), rng.bytes(255 * 7 + 3), rng.bytes(4)], 7, max_segments=3)), serial=7)
    out["ends_on_255k"] = stream(page(7, 0, [255, 255], rng.bytes(510), OX.BOS) + page(7, 1, [0, 9], rng.bytes(9), OX.CONTINUED, 2), serial=7)
    a, b = mux([rng.bytes(300), rng.bytes(20)], 7, max_segments=1), mux([rng.bytes(40), rng.bytes(600)], 9, max_segments=2)
    inter = [x for pair in zip(a, b) for x in pair] + a[len(b):] + b[len(a):]
    out["two_serials"] = stream(b"".join(inter), serial=7)
    out["two_serials_other"] = stream(b"".join(inter), serial=9)
    out["first_serial"] = stream(b"".join(inter[1:]), flags=OX.ANY_SERIAL)
    out["version_1"] = stream(page(7, 0, [3], b"abc", OX.BOS) + page(7, 1, [2], b"zz", version=1) + page(7, 1, [4], b"defg", OX.EOS, 5), serial=7)
    out["gap"] = stream(b"".join(mux([rng.bytes(30)], 7, eos=False)) + page(7, 1, [255], rng.bytes(255)) + page(7, 3, [5], rng.bytes(5), OX.CONTINUED), serial=7)
    good = mux([rng.bytes(100), rng.bytes(100), rng.bytes(100)], 7, max_segments=1)
    flipped = bytearray(good[1])
    flipped[40] ^= 0x10
    out["flipped_bit"] = stream(good[0] + bytes(flipped) + good[2], serial=7)
    out["junk"] = stream(good[0] + b"\x00\x01" + good[1] + good[2], serial=7)
    out["continued_first"] = stream(page(7, 4, [255, 255], rng.bytes(510), OX.CONTINUED) + page(7, 5, [255, 17, 6], rng.bytes(278), OX.CONTINUED, 9) +
                                    page(7, 6, [1], b"!", OX.EOS, 10), serial=7, expect_seq=4)
    out["any_seq"] = stream(page(7, 0xFFFFFFFF, [2], b"hi", 0, 1) + page(7, 0, [2], b"ho", 0, 2), serial=7, flags=OX.ANY_SEQ)
    whole = b"".join(good)
    out["truncated"] = stream(whole[:-11], serial=7)
    out["truncated_in_lacing"] = stream(whole[:len(good[0]) + 27], serial=7)
    out["truncated_in_header"] = stream(whole[:len(good[0]) + 26], serial=7)
    out["eos_open"] = stream(page(7, 0, [5], b"12345", OX.BOS, 1) + page(7, 1, [255], rng.bytes(255), OX.EOS, -1), serial=7)
    out["eos_open_then_closed"] = stream(page(7, 0, [255], rng.bytes(255), OX.EOS, -1) + page(7, 1, [0], b"", OX.CONTINUED, 4), serial=7)
    out["eos_no_segments"] = stream(page(7, 0, [255], rng.bytes(255), OX.BOS, -1) + page(7, 1, [], b"", OX.EOS, -1) + page(7, 2, [1], b"x", 0, 3), serial=7)
    inner = page(7, 1, [4], b"DATA", 0, 77)                               # a whole valid page image as payload
    out["page_in_body"] = stream(page(7, 0, lacing_of(len(inner) + 3), b"ab" + inner + b"c", OX.BOS, 1) + page(7, 1, [2], b"ok", OX.EOS, 2), serial=7)
    head = b"\x7fFLAC\x01\x00\x00\x02fLaC" + rng.bytes(38)
    out["mapping"] = stream(b"".join(mux([head, rng.bytes(40), rng.bytes(700)], 7, max_segments=2)), serial=7, flags=OX.FLAC_MAPPING)
    out["mapping_unasked"] = stream(b"".join(mux([head, rng.bytes(40)], 7)), serial=7)
    out["mapping_twice"] = stream(b"".join(mux([b"q", head, b"\x7fFLAC\x01abc", b"\x7fFLAC\x01abc" + rng.bytes(300), rng.bytes(7)], 7)), serial=7, flags=OX.FLAC_MAPPING)
    out["mapping_short"] = stream(b"".join(mux([rng.bytes(12), b"\x7fFLAC\x01\x00\x00", rng.bytes(5)], 7)), serial=7, flags=OX.FLAC_MAPPING)
    out["mapping_magic"] = stream(b"".join(mux([rng.bytes(12), b"\x7fFLAK\x01\x00\x00\x02fLaC", rng.bytes(5)], 7)), serial=7, flags=OX.FLAC_MAPPING)
    out["mapping_version"] = stream(b"".join(mux([rng.bytes(12), rng.bytes(600), b"\x7fFLAC\x02\x00\x00\x02fLaC" + rng.bytes(600), rng.bytes(5)], 7, max_segments=2)),
                                    serial=7, flags=OX.FLAC_MAPPING)
    out["mapping_open"] = stream(page(7, 0, [3, 255], b"abc" + head[:9] + rng.bytes(246), OX.BOS, 1), serial=7, flags=OX.FLAC_MAPPING)
    out["bad_resume"] = stream(good[0], serial=7, first_page_segment=2)
    out["resume_all"] = stream(good[0] + good[1], serial=7, first_page_segment=1)
    out["empty"] = stream(b"", serial=7)
    out["short"] = stream(b"OggS" + bytes(22), serial=7)
    out["not_ogg"] = stream(bytes(27), serial=7)
    return out


def fnv1a32(data):
    h = 2166136261
    for b in data:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def golden_expectation(events):
    """What the recorded events say the walk must give (tests/golden/ogg/README.md): the status, and (bytes, granule, b_o_s, e_o_s,
    hash) of the packets delivered."""
    status, delivered = OX.OK, []
    for e in events:
        if e[0] == "sync":
            status = OX.LOST_SYNC
            break
        if e[0] == "hole":
            status = OX.HOLE
            break
        if e[0] == "packet":
            delivered.append(tuple(e[1:]))
    return status, delivered


def load_golden():
    """The sessions recorded from the reference's page library (tests/golden/ogg/README.md): name -> (bytes, record)."""
    with open(os.path.join(GOLDEN, "sessions.json")) as f:
        index = json.load(f)
    out = {}
    for name, rec in index["sessions"].items():
        with gzip.open(os.path.join(GOLDEN, name + ".ogg.gz"), "rb") as f:
            out[name] = (f.read(), rec)
    return out


# ---- Ogg FLAC: the committed FLAC fixtures' frames wrapped in pages by the mapping's rules (a test-side muxer)
def flac_packets(fx):
    """The packets of an Ogg FLAC stream made of a native one: the mapping header with "fLaC" and STREAMINFO, a packet per further
    metadata block, a packet per frame; and the granule position (samples so far) behind every packet."""
    import flac_cases as FC
    data, at, blocks = fx.data, 4, []
    while True:
        last, size = data[at] & 0x80, int.from_bytes(data[at + 1:at + 4], "big")
        blocks.append(data[at:at + 4 + size])
        at += 4 + size
        if last:
            break
    assert at == fx.audio
    packets = [b"\x7fFLAC\x01\x00" + (len(blocks) - 1).to_bytes(2, "big") + b"fLaC" + blocks[0]] + blocks[1:]
    granules = [0] * len(packets)
    res, _ = FC.model(FC.whole(fx))
    done = 0
    for f, (a, b) in zip(res.frames, FC.frame_spans(fx.name)):
        packets.append(data[a:b])
        done += f.header.blocksize
        granules.append(done)
    return packets, granules, len(blocks)


def ogg_flac(fx, serial=0x464C, max_segments=255, first_audio_seq=None):
    """(bytes, offset of the page the first audio packet begins on, that page's number) of the fixture as Ogg FLAC: the header packet
    alone on the first page, the other metadata on the next, the audio from a fresh page on in pages of up to max_segments segments."""
    packets, granules, n_meta = flac_packets(fx)
    pages = mux(packets[:1], serial, 0, granules=granules[:1], eos=False)
    if n_meta > 1:
        pages += mux(packets[1:n_meta], serial, len(pages), granules=granules[1:n_meta], bos=False, eos=False)
    head = b"".join(pages)
    pages += mux(packets[n_meta:], serial, len(pages), max_segments=max_segments, granules=granules[n_meta:], bos=False)
    return b"".join(pages), len(head), len(pages) - len(mux(packets[n_meta:], serial, 0, max_segments=max_segments))
