"""An independent model of the Vorbis I decoder (include/ohgpu_vorbis.h: V1-V6), in numpy, written from the specification: the header
packets parsed here, codewords assigned here, floor 1, residues 0 / 1 / 2, coupling -- in float32 where the product is, one operation at a
time, up to the spectrum -- and from there on float64: a direct-form DCT-IV unfolded into the IMDCT, the window from its closed form,
overlap-add, and V5's rounding with V6's rule for what is not a number.  Nothing of the product's text is used.

The bit source is an object with read(n), choose(book) and eop: Bits reads a packet; tests/vorbis_frames.py passes one that invents the
bits instead, which is how the random-valid streams are written."""
import math

import numpy as np

OK, HEADER, CORRUPT = 0, 1, 2
F32 = np.float32


def ilog(v):
    return int(v).bit_length()


class Bits:
    def __init__(self, data):
        self.data, self.pos, self.eop = bytes(data), 0, False

    def read(self, n):
        if n == 0:
            return 0
        if self.eop or self.pos + n > 8 * len(self.data):
            self.eop = True
            return 0
        v = 0
        for k in range(n):
            p = self.pos + k
            v |= ((self.data[p >> 3] >> (p & 7)) & 1) << k
        self.pos += n
        return v

    def choose(self, book):
        """One codeword, first bit first: the entry, or -1 (and the end of the packet) where the bits end or the tree holds nothing."""
        cw, length = 0, 0
        while length < 32:
            bit = self.read(1)
            if self.eop:
                return -1
            cw, length = (cw << 1) | bit, length + 1
            e = book.leaves.get((length, cw))
            if e is not None:
                return e
            if (length, cw) not in book.inner:
                break
        self.eop = True
        return -1


def assign_codewords(lengths):
    """Section 3.2.1: {entry: codeword} in entry order; ValueError for an over-specified tree."""
    avail = [0] * 33
    out = {}
    first = True
    for e, n in enumerate(lengths):
        if n == 0:
            continue
        if n > 32:
            raise ValueError("codeword length beyond 32")
        if first:
            first = False
            out[e] = 0
            for i in range(1, n + 1):
                avail[i] = 1 << (32 - i)
            continue
        z = n
        while z > 0 and not avail[z]:
            z -= 1
        if z == 0:
            raise ValueError("over-specified")
        res = avail[z]
        avail[z] = 0
        out[e] = res >> (32 - n)
        for y in range(n, z, -1):
            avail[y] = res + (1 << (32 - y))
    return out


def float32_unpack(x):
    mant, e = x & 0x1fffff, (x >> 21) & 0x3ff
    with np.errstate(over="ignore"):                                 # (the packed float reaches 2^256: V6 refuses what is not finite)
        return F32(math.ldexp(-mant if x & 0x80000000 else mant, e - 788))


def lookup1_values(entries, dim):
    r = 0
    while (r + 1) ** dim <= entries:
        r += 1
    return r


class Book:
    pass


class Setup:
    pass


class TooLarge(Exception):
    """parse_headers met a codebook of more entries than its caller wants to wait for."""


def parse_headers(id_packet, setup_packet, max_entries=None):
    """The identification and setup header packets -> Setup; ValueError("invalid ...") / ValueError("unsupported ...").  max_entries:
    TooLarge as soon as a codebook declares more (a damaged header can declare 2^24, and this is plain Python)."""
    b = Bits(id_packet)

    def magic(t):
        return [b.read(8) for _ in range(7)] == [t] + list(b"vorbis") and not b.eop
    if not magic(1) or b.read(32) != 0:
        raise ValueError("invalid identification header")
    s = Setup()
    s.channels, s.rate = b.read(8), b.read(32)
    b.read(32), b.read(32), b.read(32)
    e0, e1 = b.read(4), b.read(4)
    if b.read(1) != 1 or b.eop or s.channels == 0 or s.rate == 0 or e0 < 6 or e1 > 13 or e0 > e1:
        raise ValueError("invalid identification header")
    s.bs = (1 << e0, 1 << e1)
    ch = s.channels
    b = Bits(setup_packet)
    if not magic(5):
        raise ValueError("invalid setup header")
    s.books = []
    for _ in range(b.read(8) + 1):
        k = Book()
        if b.read(24) != 0x564342:
            raise ValueError("invalid codebook sync")
        k.dim, k.entries = b.read(16), b.read(24)
        if max_entries is not None and k.entries > max_entries:
            raise TooLarge(k.entries)
        lengths = [0] * k.entries
        if not b.read(1):
            sparse = b.read(1)
            for e in range(k.entries):
                if not sparse or b.read(1):
                    lengths[e] = b.read(5) + 1
        else:
            cur, n = 0, b.read(5) + 1
            while cur < k.entries and not b.eop:
                number = b.read(ilog(k.entries - cur))
                if number > k.entries - cur:
                    raise ValueError("invalid ordered lengths")
                lengths[cur:cur + number] = [n] * number
                cur, n = cur + number, n + 1
        if b.eop:
            raise ValueError("invalid: header ends")
        try:
            k.codewords = assign_codewords(lengths)
        except ValueError:
            raise ValueError("invalid: over-specified codebook")
        k.lengths = lengths
        k.leaves = {(lengths[e], cw): e for e, cw in k.codewords.items()}
        k.inner = {(n, cw >> (lengths[e] - n)) for e, cw in k.codewords.items() for n in range(1, lengths[e])}
        k.lookup = b.read(4)
        if k.lookup > 2:
            raise ValueError("invalid lookup type")
        k.values = None
        if k.lookup:
            vmin, delta = float32_unpack(b.read(32)), float32_unpack(b.read(32))
            vbits, seq = b.read(4) + 1, b.read(1)
            if k.dim == 0:
                raise ValueError("invalid: value vectors of dimension 0")
            if k.entries * k.dim * 4 > 16 << 20:
                raise ValueError("unsupported: value vectors beyond the image's cap")
            nmult = lookup1_values(k.entries, k.dim) if k.lookup == 1 else k.entries * k.dim
            if nmult * vbits > 8 * len(setup_packet):
                raise ValueError("invalid: header ends")
            mult = np.array([b.read(vbits) for _ in range(nmult)], dtype=F32)
            if b.eop:
                raise ValueError("invalid: header ends")
            # every entry's vector, one float32 operation at a time: (mult * delta + min) + last, a column of all entries per step
            k.values = np.zeros((k.entries, k.dim), dtype=F32)
            e = np.arange(k.entries, dtype=np.int64)
            last, div = np.zeros(k.entries, dtype=F32), 1
            with np.errstate(over="ignore", invalid="ignore"):
                for d in range(k.dim):
                    off = (e // div) % nmult if k.lookup == 1 else e * k.dim + d
                    v = (mult[off] * delta + vmin) + last          # (float32 arrays and scalars: each operation rounds to float32)
                    if seq:
                        last = v
                    k.values[:, d] = v
                    div = div * nmult if k.lookup == 1 else 1        # (nmult ^ dim <= entries: it stays small)
            if not np.isfinite(k.values).all():
                raise ValueError("invalid: a value vector entry is not finite (V6)")
        s.books.append(k)
    for _ in range(b.read(6) + 1):
        if b.read(16) != 0:
            raise ValueError("invalid time domain transform")
    s.floors = []
    for _ in range(b.read(6) + 1):
        t = b.read(16)
        if b.eop:
            raise ValueError("invalid: header ends")
        if t == 0:
            raise ValueError("unsupported floor 0")
        if t != 1:
            raise ValueError("invalid floor type")
        f = Setup()
        f.part_class = [b.read(4) for _ in range(b.read(5))]
        f.classes = []
        for _ in range(max(f.part_class) + 1 if f.part_class else 0):
            c = Setup()
            c.dim, c.sub = b.read(3) + 1, b.read(2)
            c.master = b.read(8) if c.sub else None
            c.books = [b.read(8) - 1 for _ in range(1 << c.sub)]
            if (c.sub and c.master >= len(s.books)) or max(c.books) >= len(s.books):
                raise ValueError("invalid floor book")
            f.classes.append(c)
        f.mult, f.rangebits = b.read(2) + 1, b.read(4)
        f.x = [0, 1 << f.rangebits]
        for c in f.part_class:
            f.x += [b.read(f.rangebits) for _ in range(f.classes[c].dim)]
        if len(f.x) > 65 or len(set(f.x)) != len(f.x):
            raise ValueError("invalid floor values")
        f.order = sorted(range(len(f.x)), key=lambda i: f.x[i])
        f.low = [max((k for k in range(i) if f.x[k] < f.x[i]), key=lambda k: f.x[k], default=None) for i in range(len(f.x))]
        f.high = [min((k for k in range(i) if f.x[k] > f.x[i]), key=lambda k: f.x[k], default=None) for i in range(len(f.x))]
        s.floors.append(f)
    s.residues = []
    for _ in range(b.read(6) + 1):
        r = Setup()
        r.type = b.read(16)
        if r.type > 2 or b.eop:
            raise ValueError("invalid residue type")
        r.begin, r.end, r.psize, r.classes, r.classbook = b.read(24), b.read(24), b.read(24) + 1, b.read(6) + 1, b.read(8)
        r.cascade = []
        for _ in range(r.classes):
            low = b.read(3)
            r.cascade.append((b.read(5) if b.read(1) else 0) * 8 + low)
        r.books = [[b.read(8) if (c >> j) & 1 else None for j in range(8)] for c in r.cascade]
        if r.classbook >= len(s.books) or s.books[r.classbook].dim == 0:
            raise ValueError("invalid residue class book")
        if any(k is not None and (k >= len(s.books) or s.books[k].values is None) for row in r.books for k in row):
            raise ValueError("invalid residue book: none, or one without value vectors")
        s.residues.append(r)
    s.mappings = []
    for _ in range(b.read(6) + 1):
        if b.read(16) != 0 or b.eop:
            raise ValueError("invalid mapping type")
        m = Setup()
        m.submaps = b.read(4) + 1 if b.read(1) else 1
        m.coupling = []
        if b.read(1):
            for _ in range(b.read(8) + 1):
                m.coupling.append((b.read(ilog(ch - 1)), b.read(ilog(ch - 1))))
            if len(m.coupling) > 32:
                raise ValueError("unsupported: more than 32 coupling steps")
            if any(mag == ang or mag >= ch or ang >= ch for mag, ang in m.coupling):
                raise ValueError("invalid coupling channels")
        if b.read(2) != 0:
            raise ValueError("invalid mapping")
        m.mux = [b.read(4) for _ in range(ch)] if m.submaps > 1 else [0] * ch
        m.sub = []
        for _ in range(m.submaps):
            b.read(8)
            m.sub.append((b.read(8), b.read(8)))
        if max(m.mux) >= m.submaps or any(fl >= len(s.floors) or rs >= len(s.residues) for fl, rs in m.sub):
            raise ValueError("invalid mapping: a mux, floor or residue number out of range")
        s.mappings.append(m)
    s.modes = []
    for _ in range(b.read(6) + 1):
        flag = b.read(1)
        if b.read(16) != 0 or b.read(16) != 0:
            raise ValueError("invalid mode")
        s.modes.append((flag, b.read(8)))
        if s.modes[-1][1] >= len(s.mappings):
            raise ValueError("invalid mode mapping")
    if b.read(1) != 1 or b.eop:
        raise ValueError("invalid framing")
    return s


# ---------------------------------------------------------------- a packet, up to the spectrum
def render_point(x0, y0, x1, y1, x):
    dy, adx = y1 - y0, x1 - x0
    off = abs(dy) * (x - x0) // adx
    return y0 - off if dy < 0 else y0 + off


def render_line(x0, y0, x1, y1, out):
    dy, adx = y1 - y0, x1 - x0
    base = abs(dy) // adx * (-1 if dy < 0 else 1)                   # (C's division truncates)
    sy = base - 1 if dy < 0 else base + 1
    ady = abs(dy) - abs(base) * adx
    y, err = y0, 0
    if x0 < len(out):
        out[x0] = y
    for x in range(x0 + 1, min(x1, len(out))):
        err += ady
        if err >= adx:
            err -= adx
            y += sy
        else:
            y += base
        out[x] = y


def floor_decode(s, f, b):
    """(final y, flags) or None for an unused floor -- also where the packet ends inside it (Tremor's reading)."""
    if not b.read(1):
        return None
    rng = (256, 128, 86, 64)[f.mult - 1]
    y = [b.read(ilog(rng - 1)), b.read(ilog(rng - 1))]
    for c in f.part_class:
        k = f.classes[c]
        cval = max(b.choose(s.books[k.master]), 0) if k.sub else 0
        for _ in range(k.dim):
            book = k.books[cval & ((1 << k.sub) - 1)]
            cval >>= k.sub
            y.append(max(b.choose(s.books[book]), 0) if book >= 0 else 0)
    if b.eop:
        return None
    fin, flag = y[:2] + [0] * (len(y) - 2), [True, True] + [False] * (len(y) - 2)
    for i in range(2, len(y)):
        lo, hi = f.low[i], f.high[i]
        pred = render_point(f.x[lo], fin[lo], f.x[hi], fin[hi], f.x[i])
        val, highroom, lowroom = y[i], rng - pred, pred
        room = min(highroom, lowroom) * 2
        if val:
            flag[lo] = flag[hi] = flag[i] = True
            if val >= room:
                fin[i] = val - lowroom + pred if highroom > lowroom else pred - val + highroom - 1
            else:
                fin[i] = pred - (val + 1) // 2 if val & 1 else pred + val // 2
        else:
            fin[i] = pred
    return fin, flag


def floor_curve(f, fin, flag, n):
    """The curve's n table indices."""
    out = [0] * n
    level = lambda j: min(max(fin[j] * f.mult, 0), 255)
    lx, ly = 0, level(f.order[0])
    for j in f.order[1:]:
        if flag[j]:
            hx, hy = f.x[j], level(j)
            render_line(lx, ly, hx, hy, out)
            lx, ly = hx, hy
    for x in range(lx, n):
        out[x] = ly
    return out


def residue_decode(s, r, b, half, dnd):
    """The vectors of one submap (float32 [len(dnd)][half]); stops where the packet ends."""
    nvec = len(dnd)
    two = r.type == 2
    out = np.zeros((nvec, half), dtype=F32)
    if two and all(dnd):
        return out
    vecs, actual = (1, half * nvec) if two else (nvec, half)
    work = np.zeros((vecs, actual), dtype=F32)

    def finish():
        return work.reshape(half, nvec).T.copy() if two else work
    lb, le = min(r.begin, actual), min(r.end, actual)
    cb = s.books[r.classbook]
    parts = max(le - lb, 0) // r.psize
    if parts == 0:
        return finish()
    cls = [[0] * (parts + cb.dim) for _ in range(vecs)]
    for p in range(8):
        pc = 0
        while pc < parts:
            if p == 0:
                for j in range(vecs):
                    if not two and dnd[j]:
                        continue
                    temp = b.choose(cb)
                    if temp < 0:
                        return finish()
                    for i in reversed(range(cb.dim)):
                        cls[j][pc + i] = temp % r.classes
                        temp //= r.classes
            for _ in range(cb.dim):
                if pc >= parts:
                    break
                for j in range(vecs):
                    if not two and dnd[j]:
                        continue
                    c = cls[j][pc]
                    if not (r.cascade[c] >> p) & 1:
                        continue
                    vb = s.books[r.books[c][p]]
                    off = lb + pc * r.psize
                    if r.type == 0:
                        step = r.psize // vb.dim
                        for k in range(step):
                            e = b.choose(vb)
                            if e < 0:
                                return finish()
                            work[j, off + k:off + k + vb.dim * step:step][:vb.dim] += vb.values[e]
                    else:
                        k = 0
                        while k < r.psize:
                            e = b.choose(vb)
                            if e < 0:
                                return finish()
                            m = min(vb.dim, r.psize - k)
                            work[j, off + k:off + k + m] += vb.values[e][:m]
                            k += m
                pc += 1
    return finish()


def packet_head(s, b):
    """(status, mode, block, prev flag, next flag)"""
    t = b.read(1)
    if b.eop:
        return CORRUPT, 0, 0, 0, 0
    if t:
        return HEADER, 0, 0, 0, 0
    mode = b.read(ilog(len(s.modes) - 1))
    if b.eop or mode >= len(s.modes):
        return CORRUPT, 0, 0, 0, 0
    flag = s.modes[mode][0]
    pf, nf = (b.read(1), b.read(1)) if flag else (0, 0)
    if b.eop:
        return CORRUPT, 0, 0, 0, 0
    return OK, mode, s.bs[flag], pf, nf


DB = np.array([F32(10.0 ** (7.0 * (i - 255) / 256.0)) for i in range(256)], dtype=F32)


def packet_spectrum(s, b, mode, n):
    """Behind packet_head: float32 [channels][n / 2], zero rows for unused floors."""
    half = n // 2
    m = s.mappings[s.modes[mode][1]]
    floors = [floor_decode(s, s.floors[m.sub[m.mux[c]][0]], b) for c in range(s.channels)]
    nonzero = [f is not None for f in floors]
    for mag, ang in m.coupling:
        if nonzero[mag] or nonzero[ang]:
            nonzero[mag] = nonzero[ang] = True
    rows = np.zeros((s.channels, half), dtype=F32)
    for sm in range(m.submaps):
        chans = [c for c in range(s.channels) if m.mux[c] == sm]
        if chans:
            rows[chans] = residue_decode(s, s.residues[m.sub[sm][1]], b, half, [not nonzero[c] for c in chans])
    for mag, ang in reversed(m.coupling):
        M, A = rows[mag].copy(), rows[ang].copy()
        newM = np.where(M > 0, np.where(A > 0, M, M + A), np.where(A > 0, M, M - A)).astype(F32)
        newA = np.where(M > 0, np.where(A > 0, M - A, M), np.where(A > 0, M + A, M)).astype(F32)
        rows[mag], rows[ang] = newM, newA
    for c in range(s.channels):
        if floors[c] is None:
            rows[c] = 0
        else:
            f = s.floors[m.sub[m.mux[c]][0]]
            rows[c] = rows[c] * DB[floor_curve(f, floors[c][0], floors[c][1], half)]
    return rows


# ---------------------------------------------------------------- from the spectrum on: float64
_DCT = {}


def dct4(x):
    """u[i] = sum_k x[k] cos(pi / N (i + 1/2)(k + 1/2)), by the definition."""
    N = len(x)
    x = x.astype(np.float64)
    if N <= 1024:
        if N not in _DCT:
            i = np.arange(N)
            _DCT[N] = np.cos(np.pi / N * np.outer(i + 0.5, i + 0.5))
        return _DCT[N] @ x
    out = np.zeros(N)
    k = np.arange(N) + 0.5
    for i0 in range(0, N, 256):
        out[i0:i0 + 256] = np.cos(np.pi / N * np.outer(np.arange(i0, i0 + 256) + 0.5, k)) @ x
    return out


def imdct(x):
    """y[i] = sum_k x[k] cos(pi / N (i + 1/2 + N/2)(k + 1/2)), i < 2N: the DCT-IV's N values, unfolded by the cosine's symmetries."""
    N = len(x)
    u = dct4(x)
    return np.concatenate([u[N // 2:], -u[::-1], -u[:N // 2]])


def slope(n):
    i = np.arange(n // 2)
    return np.sin(np.pi / 2 * np.sin((i + 0.5) / n * np.pi) ** 2)


def window(n, bs0, is_long, pf, nf):
    def half(full):
        if full:
            return slope(n)
        start = n // 4 - bs0 // 4
        return np.concatenate([np.zeros(start), slope(bs0), np.ones(n // 2 - start - bs0 // 2)])
    return np.concatenate([half(not is_long or pf), half(not is_long or nf)[::-1]])


def decode_packet(s, data):
    """One packet by itself (nothing of a packet depends on another before the overlap): (status, mode, block, spectrum, windowed block),
    the last two None unless OK."""
    b = Bits(data)
    status, mode, n, pf, nf = packet_head(s, b)
    if status != OK:
        return status, 0, 0, None, None
    with np.errstate(over="ignore", invalid="ignore"):               # (V6: huge finite value vectors may sum past float32)
        rows = packet_spectrum(s, b, mode, n)
        block = np.stack([imdct(rows[c]) for c in range(s.channels)]) * window(n, s.bs[0], n == s.bs[1] and s.modes[mode][0], pf, nf)[None, :]
    return status, mode, n, rows, block


def to_pcm16(x):
    """V5, and V6's second half: what is not a number is stored as 0."""
    with np.errstate(invalid="ignore"):
        v = np.clip(np.floor(x * 32768.0 + 0.5), -32768, 32767)
    return np.where(np.isnan(v), 0.0, v).astype(np.int32)


def decode_stream(s, packets, max_samples=None, want_float=False, cache=None):
    """A stream's packets (bytes each) -> (records, spectra, pcm): records as (status, mode, block, samples, position) per packet, spectra
    float32 [channels][block / 2] per OK packet (else None), pcm int32 [channels][samples] by V3-V6 (or the float64 before rounding).
    cache: a dict of this setup's decode_packet results by the packet's bytes, for sets of streams that share most packets."""
    recs, spectra, out = [], [], []
    prev, pos = None, 0
    for data in packets:
        data = bytes(data)
        if cache is None:
            status, mode, n, rows, block = decode_packet(s, data)
        else:
            if data not in cache:
                cache[data] = decode_packet(s, data)
            status, mode, n, rows, block = cache[data]
        if status != OK:
            recs.append((status, 0, 0, 0, pos))
            spectra.append(None)
            continue
        spectra.append(rows)
        d = 0
        if prev is not None:
            pn = prev.shape[1]
            d = pn // 4 + n // 4
            piece = np.zeros((s.channels, d))
            piece[:, :min(pn // 2, d)] += prev[:, pn // 2:pn // 2 + min(pn // 2, d)]
            shift = n // 4 - pn // 4
            j0 = max(0, -shift)
            with np.errstate(invalid="ignore"):
                piece[:, j0:] += block[:, j0 + shift:d + shift]
            out.append(piece)
        room = d if max_samples is None else max(0, min(d, max_samples - pos))
        recs.append((OK, mode, n, room, pos))
        pos += d
        prev = block
    x = np.concatenate(out, axis=1) if out else np.zeros((s.channels, 0))
    if max_samples is not None:
        x = x[:, :max_samples]
    if want_float:
        return recs, spectra, x
    return recs, spectra, to_pcm16(x)


def mdct(x):
    """The forward transform the minimal encoder uses: X[k] = sum_i x[i] cos(pi / N (i + 1/2 + N/2)(k + 1/2)) * 2 / N, so that windowed
    overlap-add of imdct(mdct(.)) gives the signal back."""
    n = len(x)
    N = n // 2
    i, k = np.arange(n), np.arange(N)
    return (np.cos(np.pi / N * np.outer(k + 0.5, i + 0.5 + N / 2)) @ x) * (2.0 / N)
