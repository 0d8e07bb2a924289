"""The tests' own Apple Lossless packet writer, for what no encoder emits: mode != 0, any predictor order, code factors other than 4,
rounding-shift extremes, the nine-ones escape, fill and data elements, LFE, an early end tag, a pair beyond the stream's channels,
shifted bytes together with escape, coefficients that wrap.  The residual coder is tests/alac_textbook.py's reader turned round; the
writer takes residuals, not samples (what they decode to is the model's to say, and tests/golden/alac_textbook.json pins it).
"""
import struct

SCE, CPE, LFE, DSE, FIL, END = 0, 1, 3, 4, 6, 7


def cookie(frame_length, bit_depth, channels, sample_rate=44100, pb=40, mb=10, kb=14, max_run=255, version=0):
    return struct.pack(">IBBBBBBHIII", frame_length, version, bit_depth, pb, mb, kb, channels, max_run, 0, 0, sample_rate)


def wrapped(config, frma=True, alac=True):
    """the configuration behind the atoms older files put in front of it"""
    out = b""
    if frma:
        out += struct.pack(">I4s4s", 12, b"frma", b"alac")
    if alac:
        out += struct.pack(">I4sI", 36, b"alac", 0)
    return out + config


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, k):
        for i in range(k - 1, -1, -1):
            self.bits.append((v >> i) & 1)

    def ones(self, n):
        self.bits.extend([1] * n)

    def align(self):
        while len(self.bits) & 7:
            self.bits.append(0)

    def short(self, value, k):
        """`value` (0 .. 2^k - 2) the way the reader's short_bits takes it"""
        if value == 0:
            self.put(0, k - 1)
        else:
            self.put(value + 1, k)

    def bytes(self):
        self.align()
        out = bytearray()
        for i in range(0, len(self.bits), 8):
            b = 0
            for bit in self.bits[i:i + 8]:
                b = (b << 1) | bit
            out.append(b)
        return bytes(out)


def ilog2(x):
    return x.bit_length() - 1


def write_residuals(w, res, pb, mb, kb, width, escape_at=(), run_escape_at=()):
    """`escape_at`: indices written with the nine-ones escape although a prefix would do; `run_escape_at`: the same for zero runs"""
    n = len(res)
    mean, after_run, c = mb, 0, 0
    while c < n:
        d = res[c]
        coded = 2 * d if d >= 0 else -2 * d - 1
        v = coded - after_run
        assert 0 <= v < (1 << width), "residual %d cannot follow a run / does not fit" % d
        k = min(ilog2((mean >> 9) + 3), kb)
        step = (1 << k) - 1
        if v // step >= 9 or c in escape_at:
            w.ones(9)
            w.put(v, width)
        else:
            w.ones(v // step)
            w.put(0, 1)
            if k > 1:
                w.short(v % step, k)
        c += 1
        mean = (pb * coded + mean - (((pb * mean) & 0xffffffff) >> 9)) & 0xffffffff
        if v > 0xffff:
            mean = 0xffff
        after_run = 0
        if ((mean << 2) & 0xffffffff) < 512 and c < n:
            after_run = 1
            run = 0
            while c + run < n and res[c + run] == 0 and run < 65535:
                run += 1
            kz = (32 - mean.bit_length()) - 24 + ((mean + 16) >> 6)
            stepz = ((1 << kz) - 1) & ((1 << kb) - 1)
            if run // stepz >= 9 or c in run_escape_at:
                w.ones(9)
                w.put(run, 16)
            else:
                w.ones(run // stepz)
                w.put(0, 1)
                w.short(run % stepz, kz)
            c += run
            if run >= 65535:
                after_run = 0
            mean = 0


def channel(res, order=0, coef=(), mode=0, den_shift=9, factor=4, escape_at=(), run_escape_at=()):
    assert len(coef) == order
    return dict(res=list(res), order=order, coef=list(coef), mode=mode, den_shift=den_shift, factor=factor, escape_at=set(escape_at),
                run_escape_at=set(run_escape_at))


def audio(w, cfg, tag, chans, instance=0, partial=None, shifted=0, mix_bits=0, mix_res=0, low=None, raw=None, unused=0):
    """One audio element.  chans: channel() records (compressed); raw: per-channel sample lists (escape).  low: per-channel lists of
    the shifted-off values.  partial: the sample count to write, or None for no partial flag."""
    frame_length, depth, pb, mb, kb = cfg
    nch = 2 if tag == CPE else 1
    w.put(tag, 3)
    w.put(instance, 4)
    w.put(unused, 12)
    w.put(1 if partial is not None else 0, 1)
    w.put(shifted, 2)
    w.put(1 if raw is not None else 0, 1)
    if partial is not None:
        w.put(partial, 32)
    if raw is not None:
        assert len(raw) == nch
        for i in range(len(raw[0])):
            for c in range(nch):
                w.put(raw[c][i] & ((1 << depth) - 1), depth)
        return
    assert len(chans) == nch
    width = depth - 8 * shifted + (1 if nch == 2 else 0)
    w.put(mix_bits, 8)
    w.put(mix_res & 0xff, 8)
    for ch in chans:
        w.put(ch["mode"], 4)
        w.put(ch["den_shift"], 4)
        w.put(ch["factor"], 3)
        w.put(ch["order"], 5)
        for a in ch["coef"]:
            w.put(a & 0xffff, 16)
    if shifted:
        for i in range(len(low[0])):
            for c in range(nch):
                w.put(low[c][i], 8 * shifted)
    for ch in chans:
        write_residuals(w, ch["res"], (pb * ch["factor"]) // 4, mb, kb, width, ch["escape_at"], ch["run_escape_at"])


def fil(w, count, payload=0xa5):
    w.put(FIL, 3)
    if count < 15:
        w.put(count, 4)
    else:
        w.put(15, 4)
        w.put(count - 15 + 1, 8)
    for _ in range(count):
        w.put(payload, 8)


def dse(w, count, align, payload=0x5a):
    w.put(DSE, 3)
    w.put(0, 4)
    w.put(1 if align else 0, 1)
    if count < 255:
        w.put(count, 8)
    else:
        w.put(255, 8)
        w.put(count - 255, 8)
    if align:
        w.align()
    for _ in range(count):
        w.put(payload, 8)


def end(w):
    w.put(END, 3)
