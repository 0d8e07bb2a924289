"""Vorbis I streams for the tests, written two ways (no encoder library is involved):
(a) random-valid streams: a random setup (trees with unused entries, a one-entry book, an ordered book, lookups 1 and 2, floors with
    several classes and subclasses, residues 0 / 1 / 2 with multi-pass cascades, coupling, submaps) and audio packets whose bits are
    invented while tests/vorbis_textbook.py walks them -- every read takes a random value, every codeword a random used entry -- so each
    packet is exactly as long as its decode; the codebooks' common exponent is then set so that the model's PCM peaks near half scale
    (or, for the clipping stream, beyond full scale): the bits do not depend on it;
(b) a minimal encoder: one channel, a flat floor of 0 dB, one scalar codebook: the textbook forward MDCT of a signal, quantised."""
import numpy as np

import vorbis_textbook as TB


class Writer:
    def __init__(self):
        self.bits = []

    def write(self, v, n):
        self.bits.extend((v >> k) & 1 for k in range(n))

    def bytes(self):
        return np.packbits(np.array(self.bits + [0] * (-len(self.bits) % 8), dtype=np.uint8), bitorder="little").tobytes()


class Chooser:
    """The bit source that invents the bits: forced values first (the packet's head), then random ones."""
    def __init__(self, rng, forced, cap=1.0):
        self.rng, self.forced, self.w, self.eop, self.cap = rng, list(forced), Writer(), False, cap

    def read(self, n):
        if n == 0:
            return 0
        if self.forced:
            v = self.forced.pop(0)
        elif n == 1:
            v = int(self.rng.random() < 0.85)                        # (a floor's nonzero bit: mostly used)
        else:
            v = int(self.rng.integers(0, max(1, int((1 << n) * self.cap))))   # (a floor's two end amplitudes: cap < 1 keeps the curve low)
        self.w.write(v, n)
        return v

    def choose(self, book):
        used = sorted(book.codewords)
        e = used[int(self.rng.integers(0, len(used)))]
        n, cw = book.lengths[e], book.codewords[e]
        for k in reversed(range(n)):
            self.w.write((cw >> k) & 1, 1)
        return e


def pack_float(mant, exp, neg=False):
    """The specification's packed float of mant * 2^exp."""
    assert 0 <= mant < 1 << 21 and 0 <= exp + 788 < 1024
    return (int(neg) << 31) | ((exp + 788) << 21) | mant


def tree_lengths(rng, leaves, max_depth=14):
    """The leaf depths of a random full binary tree."""
    d = [1, 1]
    while len(d) < leaves:
        i = int(rng.integers(0, len(d)))
        if d[i] >= max_depth:
            continue
        d[i] += 1
        d.append(d[i])
    return d


def random_book(rng, entries, dim, lookup, kind="plain"):
    b = dict(dim=dim, entries=entries, lookup=lookup, ordered=kind == "ordered", sparse=kind == "sparse")
    if entries == 1:
        b["lengths"] = [1]
    elif kind == "ordered":
        b["lengths"] = sorted(tree_lengths(rng, entries))
    elif kind == "sparse":
        used = max(2, entries - int(rng.integers(1, max(2, entries // 3))))
        l = tree_lengths(rng, used) + [0] * (entries - used)
        b["lengths"] = [int(v) for v in rng.permutation(l)]
    else:
        b["lengths"] = [int(v) for v in rng.permutation(tree_lengths(rng, entries))]
    if lookup:
        b["vbits"] = int(rng.integers(2, 5))
        b["seq"] = int(rng.random() < 0.3)
        n = TB.lookup1_values(entries, dim) if lookup == 1 else entries * dim
        b["mult"] = [int(v) for v in rng.integers(0, 1 << b["vbits"], size=n)]
        b["min_mant"] = int(rng.integers(1, 1 << b["vbits"])) // 2 + 1
        b["delta_mant"] = int(rng.integers(1, 3))
    return b


def random_setup(rng, channels, e0, e1, coupling=0, submaps=1, one_entry=1, strict=False):
    """A random configuration: books 0-2 scalar (sparse, ordered, one entry), 3-4 class books, 5.. value books."""
    books = [random_book(rng, 24, 1, 0, "sparse"), random_book(rng, 32, 1, 0, "ordered"), random_book(rng, one_entry, 1, 0),
             random_book(rng, 9, 2, 0), random_book(rng, 5, 1, 0, "sparse"),
             random_book(rng, 25, 2, 1), random_book(rng, 16, 4, 2), random_book(rng, 16, 1, 1, "sparse"), random_book(rng, 64, 8, 1, "ordered"),
             random_book(rng, one_entry, 2, 2)]
    vq = [5, 6, 7, 8, 9]
    floors = []
    for k in range(2):
        classes = []
        for _ in range(int(rng.integers(2, 4))):
            sub = int(rng.integers(0, 3))
            classes.append(dict(dim=int(rng.integers(1, 4)), sub=sub, master=int(rng.choice([0, 1, 4])),
                                books=[int(rng.choice([-1, 0, 1, 2])) for _ in range(1 << sub)]))
        part = [int(rng.integers(0, len(classes))) for _ in range(int(rng.integers(3, 9)))]
        part[0] = len(classes) - 1                                   # (every class is read: the highest sets how many there are)
        rangebits = (e1 - 1, e0)[k] if k else e1 - 1
        nvals = sum(classes[c]["dim"] for c in part)
        x = [int(v) + 1 for v in rng.permutation((1 << rangebits) - 1)[:nvals]]
        floors.append(dict(classes=classes, part=part, mult=int(rng.integers(1, 5)), rangebits=rangebits, x=x))
    residues = []
    for t in (0, 1, 2):
        # strict: as many classes as the class book's entries decompose into (3^2 = 9 of book 3, 5^1 of book 4) -- an encoder writes no
        # other class word, and Tremor ends the residue at one that is out of range where the specification takes it modulo
        strict_book = int(rng.choice([3, 4])) if strict else None
        ncls = (3 if strict_book == 3 else 5) if strict else int(rng.integers(2, 4))
        cascade = [int(rng.integers(0, 8)) | (int(rng.random() < 0.3) << int(rng.integers(3, 8))) for _ in range(ncls)]
        cascade[0] |= 3                                              # (a class with two passes at least)
        psize = int(rng.choice([8, 16, 32]))
        half1 = 1 << (e1 - 1)
        residues.append(dict(type=t, begin=int(rng.integers(0, 3)) * psize, end=int(half1 * (channels if t == 2 else 1) + rng.integers(-1, 2) * psize), psize=psize,
                             classbook=strict_book if strict else int(rng.choice([3, 4])), cascade=cascade,
                             books=[[int(rng.choice(vq)) if (c >> j) & 1 else None for j in range(8)] for c in cascade]))
    mappings = []
    for k in range(2):
        steps = []
        while len(steps) < coupling:
            a, b = (int(v) for v in rng.permutation(channels)[:2])
            steps.append((a, b))
        mux = [int(rng.integers(0, submaps)) for _ in range(channels)]
        for sm in range(submaps):
            mux[sm % channels] = sm if channels >= submaps else mux[sm % channels]
        mappings.append(dict(submaps=submaps, coupling=steps, mux=mux,
                             sub=[(int(rng.integers(0, 2)), int(rng.integers(0, 3))) for _ in range(submaps)]))
    modes = [(0, 0), (1, 1), (1, 0)]
    return dict(channels=channels, rate=44100, e0=e0, e1=e1, books=books, floors=floors, residues=residues, mappings=mappings, modes=modes)


def write_headers(cfg, exponent):
    """(identification packet, setup packet) of a configuration; the value books' floats are their mantissas times 2^exponent.
    What a test overrides to write a header the random setups never are: cfg["floor_type"], cfg["framing"] (the last bit), and a book's
    "overrun" (an ordered book whose first count is one more than its entries)."""
    w = Writer()
    for c in b"\x01vorbis":
        w.write(c, 8)
    w.write(0, 32), w.write(cfg["channels"], 8), w.write(cfg["rate"], 32)
    w.write(0, 32), w.write(128000, 32), w.write(0, 32)
    w.write(cfg["e0"], 4), w.write(cfg["e1"], 4), w.write(1, 1)
    ident = w.bytes()
    w = Writer()
    for c in b"\x05vorbis":
        w.write(c, 8)
    w.write(len(cfg["books"]) - 1, 8)
    for b in cfg["books"]:
        w.write(0x564342, 24), w.write(b["dim"], 16), w.write(b["entries"], 24), w.write(int(b["ordered"]), 1)
        if b["ordered"]:
            l = b["lengths"]
            w.write(l[0] - 1, 5)
            cur, n = 0, l[0]
            while cur < len(l):
                number = len(l) + 1 if b.get("overrun") else sum(1 for v in l if v == n)
                w.write(number, TB.ilog(len(l) - cur))
                cur, n = cur + number, n + 1
        else:
            w.write(int(b["sparse"]), 1)
            for v in b["lengths"]:
                if b["sparse"]:
                    w.write(int(v != 0), 1)
                if v or not b["sparse"]:
                    w.write(v - 1, 5)
        w.write(b["lookup"], 4)
        if b["lookup"]:
            w.write(pack_float(b["min_mant"], exponent, True), 32), w.write(pack_float(b["delta_mant"], exponent), 32)
            w.write(b["vbits"] - 1, 4), w.write(b["seq"], 1)
            for m in b["mult"]:
                w.write(m, b["vbits"])
    w.write(0, 6), w.write(0, 16)
    w.write(len(cfg["floors"]) - 1, 6)
    for f in cfg["floors"]:
        w.write(cfg.get("floor_type", 1), 16), w.write(len(f["part"]), 5)
        for c in f["part"]:
            w.write(c, 4)
        for c in f["classes"][:max(f["part"], default=-1) + 1]:
            w.write(c["dim"] - 1, 3), w.write(c["sub"], 2)
            if c["sub"]:
                w.write(c["master"], 8)
            for k in c["books"]:
                w.write(k + 1, 8)
        w.write(f["mult"] - 1, 2), w.write(f["rangebits"], 4)
        for v in f["x"]:
            w.write(v, f["rangebits"])
    w.write(len(cfg["residues"]) - 1, 6)
    for r in cfg["residues"]:
        w.write(r["type"], 16), w.write(r["begin"], 24), w.write(r["end"], 24), w.write(r["psize"] - 1, 24)
        w.write(len(r["cascade"]) - 1, 6), w.write(r["classbook"], 8)
        for c in r["cascade"]:
            w.write(c & 7, 3), w.write(int(c >> 3 != 0), 1)
            if c >> 3:
                w.write(c >> 3, 5)
        for row in r["books"]:
            for k in row:
                if k is not None:
                    w.write(k, 8)
    w.write(len(cfg["mappings"]) - 1, 6)
    for m in cfg["mappings"]:
        w.write(0, 16), w.write(int(m["submaps"] > 1), 1)
        if m["submaps"] > 1:
            w.write(m["submaps"] - 1, 4)
        w.write(int(bool(m["coupling"])), 1)
        if m["coupling"]:
            w.write(len(m["coupling"]) - 1, 8)
            for a, b in m["coupling"]:
                w.write(a, TB.ilog(cfg["channels"] - 1)), w.write(b, TB.ilog(cfg["channels"] - 1))
        w.write(0, 2)
        if m["submaps"] > 1:
            for v in m["mux"]:
                w.write(v, 4)
        for fl, rs in m["sub"]:
            w.write(0, 8), w.write(fl, 8), w.write(rs, 8)
    w.write(len(cfg["modes"]) - 1, 6)
    for flag, mapping in cfg["modes"]:
        w.write(flag, 1), w.write(0, 16), w.write(0, 16), w.write(mapping, 8)
    w.write(cfg.get("framing", 1), 1)
    return ident, w.bytes()


class Stream:
    """ident, setup: the header packets; packets: the audio packets' bytes; model: tests/vorbis_textbook.py's parse of the headers."""
    def __init__(self, ident, setup, packets):
        self.ident, self.setup, self.packets = ident, setup, packets
        self.model = TB.parse_headers(ident, setup)


def random_stream(seed, channels, e0, e1, n_packets, coupling=0, submaps=1, peak=0.45, floor_cap=1.0, one_entry=1, strict=False, exponent=None):
    """exponent: the value books' common exponent as it is, in place of the one that brings the PCM's peak to `peak`."""
    rng = np.random.default_rng(seed)
    cfg = random_setup(rng, channels, e0, e1, coupling, submaps, one_entry, strict)
    ident, setup = write_headers(cfg, -12)
    model = TB.parse_headers(ident, setup)
    # the blocks: long and short in runs, so that all four neighbour pairs occur; a long packet's flags are its neighbours' blocks
    modes = [int(rng.choice([0, 1, 2], p=[0.5, 0.3, 0.2])) for _ in range(n_packets)]
    if n_packets >= 6:
        modes[:6] = [1, 0, 0, 1, 2, 0]
    packets = []
    for i, mode in enumerate(modes):
        flag = cfg["modes"][mode][0]
        forced = [0, mode] + ([cfg["modes"][modes[i - 1]][0] if i else 0, cfg["modes"][modes[i + 1]][0] if i + 1 < n_packets else 0] if flag else [])
        c = Chooser(rng, forced, floor_cap)
        status, got_mode, n, _, _ = TB.packet_head(model, c)
        assert status == TB.OK and got_mode == mode
        TB.packet_spectrum(model, c, mode, n)
        packets.append(c.w.bytes())
    if exponent is not None:
        return Stream(*write_headers(cfg, exponent), packets)
    _, _, x = TB.decode_stream(model, packets, want_float=True)
    top = float(np.abs(x).max())
    shift = int(np.round(np.log2(peak / top))) if top > 0 else 0
    ident, setup = write_headers(cfg, -12 + shift)
    return Stream(ident, setup, packets)


# ---------------------------------------------------------------- (b) the minimal encoder
ENC_BITS = 12                      # the scalar book: 2^12 entries, value k - 2^11
ENC_FLOOR = 145                    # the flat floor's table index: the quantiser's step is TB.DB[145], 9.82e-4


def encode(signal, e=8):
    """One channel, blocks of n = 2^e all alike: floor flat at table index ENC_FLOOR, residue type 1, partition 8, one class, one pass of
    the scalar book of whole numbers (the balance an encoder strikes: the floor carries the level).  Returns the Stream; its packets decode to signal[n/2 : ...] delayed by nothing (the first packet primes)."""
    n = 1 << e
    N = n // 2
    entries = 1 << ENC_BITS
    w = Writer()
    for c in b"\x01vorbis":
        w.write(c, 8)
    w.write(0, 32), w.write(1, 8), w.write(44100, 32), w.write(0, 32), w.write(0, 32), w.write(0, 32), w.write(e, 4), w.write(e, 4), w.write(1, 1)
    ident = w.bytes()
    w = Writer()
    for c in b"\x05vorbis":
        w.write(c, 8)
    w.write(1, 8)                                                    # two books
    w.write(0x564342, 24), w.write(1, 16), w.write(1, 24), w.write(0, 1), w.write(0, 1), w.write(0, 5), w.write(0, 4)   # 0: one entry, the class book
    w.write(0x564342, 24), w.write(1, 16), w.write(entries, 24), w.write(1, 1), w.write(ENC_BITS - 1, 5), w.write(entries, TB.ilog(entries))
    w.write(1, 4), w.write(TB_pack(1 << (ENC_BITS - 1), 0, True), 32), w.write(TB_pack(1, 0), 32)
    w.write(ENC_BITS - 1, 4), w.write(0, 1)
    for k in range(entries):
        w.write(k, ENC_BITS)
    w.write(0, 6), w.write(0, 16)
    w.write(0, 6), w.write(1, 16), w.write(0, 5), w.write(0, 2), w.write(e - 1, 4)          # the floor: no partitions, multiplier 1
    w.write(0, 6), w.write(1, 16), w.write(0, 24), w.write(N, 24), w.write(7, 24), w.write(0, 6), w.write(0, 8), w.write(1, 3), w.write(0, 1), w.write(1, 8)
    w.write(0, 6), w.write(0, 16), w.write(0, 1), w.write(0, 1), w.write(0, 2), w.write(0, 8), w.write(0, 8), w.write(0, 8)
    w.write(0, 6), w.write(0, 1), w.write(0, 16), w.write(0, 16), w.write(0, 8)
    w.write(1, 1)
    setup = w.bytes()
    win = np.concatenate([TB.slope(n), TB.slope(n)[::-1]])
    packets = []
    for b0 in range(0, len(signal) - n + 1, N):
        X = TB.mdct(signal[b0:b0 + n] * win)
        q = np.clip(np.round(X / float(TB.DB[ENC_FLOOR])).astype(np.int64) + (1 << (ENC_BITS - 1)), 0, entries - 1)
        w = Writer()
        w.write(0, 1)                                                # audio packet; one mode: no mode bits, a short block: no flags
        w.write(1, 1), w.write(ENC_FLOOR, 8), w.write(ENC_FLOOR, 8)  # the floor: used, both ends alike
        for k in range(N):
            if k % 8 == 0:
                w.write(0, 1)                                        # the partition's class: the one-entry book's codeword
            for bit in reversed(range(ENC_BITS)):
                w.write((int(q[k]) >> bit) & 1, 1)
        packets.append(w.bytes())
    return Stream(ident, setup, packets)


def TB_pack(mant, exp, neg=False):
    return pack_float(mant, exp, neg)


# ---------------------------------------------------------------- the arenas of a batch
def batch_tables(capi, streams, planar=False, max_samples=None, ranges=None, pad=0, fill=0, share_images=False):
    """The images' blob, descriptors, packet table, source arena and destination size for streams laid one after the other; ranges[i] =
    (first, count) takes a part of stream i's packets.  share_images: streams of the same headers name one image.  The packets lie back to back, a
    packet's last byte followed at once by the next one's first, behind `pad` bytes of `fill`, which also ends the arena."""
    images, descs, rows, src = {}, np.zeros(len(streams), dtype=capi.VORBIS_STREAM_DESC), [], bytearray([fill] * pad)
    infos = []
    dst = blob_bytes = 0
    for i, st in enumerate(streams):
        key = (st.ident, st.setup) if share_images else i
        if key not in images:
            image, info = capi.vorbis_setup_parse(st.ident, st.setup)
            images[key] = (blob_bytes, image, info)
            blob_bytes += image.size
        at, image, info = images[key]
        infos.append(info)
        first, count = ranges[i] if ranges else (0, len(st.packets))
        d = descs[i]
        d["image_offset"], d["image_bytes"] = at, image.size
        d["first_packet"], d["n_packets"] = len(rows), count
        for p in st.packets[first:first + count]:
            rows.append((len(src), len(p), 0))
            src += p
        ch, long_half = int(info["channels"]), int(info["blocksize_long"]) // 2
        cap = count * long_half if max_samples is None else max_samples[i]
        d["max_samples"], d["dst_offset"] = cap, dst
        if planar:
            d["flags"], d["dst_plane_stride"] = capi.VORBIS_OUT_PLANAR32, cap * 4
            dst += cap * 4 * ch
        else:
            dst += (cap * 2 * ch + 3) & ~3
    packets = np.array(rows, dtype=capi.ALAC_PACKET) if rows else np.zeros(0, dtype=capi.ALAC_PACKET)
    blob = np.concatenate([im for _, im, _ in images.values()]) if images else np.zeros(0, dtype=np.uint8)
    return blob, descs, packets, np.frombuffer(bytes(src) + bytes([fill] * 4), dtype=np.uint8).copy(), max(dst, 4), infos


# ---------------------------------------------------------------- Ogg around a stream
COMMENT = b"\x03vorbis" + (0).to_bytes(4, "little") + (0).to_bytes(4, "little") + b"\x01"      # no vendor, no comments, framing


def ogg_file(st, granules, serial=0x5642, max_segments=40):
    """The stream as an Ogg file: the identification header alone on the first page, comment and setup on the next, then the audio
    packets, max_segments segments a page; granules[k]: the samples delivered up to and with audio packet k."""
    import ogg_cases as OC
    pages = OC.mux([st.ident], serial, 0, bos=True, eos=False, granules=[0])
    pages += OC.mux([COMMENT, st.setup], serial, len(pages), bos=False, eos=False, granules=[0, 0])
    pages += OC.mux(list(st.packets), serial, len(pages), max_segments, granules=list(granules), bos=False, eos=True)
    return b"".join(pages)


def ogg_packets(data):
    """The packets of an Ogg file of one logical stream (no checks: the pages are this module's own): [bytes]"""
    packets, cur, at = [], b"", 0
    while at < len(data):
        assert data[at:at + 4] == b"OggS"
        nseg = data[at + 26]
        lacing = data[at + 27:at + 27 + nseg]
        body = at + 27 + nseg
        for v in lacing:
            cur += data[body:body + v]
            body += v
            if v < 255:
                packets.append(cur)
                cur = b""
        at = body
    return packets
