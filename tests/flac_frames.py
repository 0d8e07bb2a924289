"""A FLAC frame WRITER of the tests' own (bit writer, the two CRCs, Rice coder, residuals computed from the samples for a chosen
predictor): it exists to make streams the 1.2.1 encoder never emits -- every subframe type and order, escapes, wasted bits, odd header
forms, planted false candidates.  TEST INFRASTRUCTURE ONLY, written from the format's definition; the decoding model
(tests/flac_textbook.py) shares nothing with it but the CRC routine."""
import hashlib

from flac_textbook import crc8, crc16


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0, (v, n)
        self.acc = (self.acc << n) | v
        self.n += n

    def signed(self, v, n):
        if n == 0:
            assert v == 0
            return
        assert -(1 << (n - 1)) <= v < (1 << (n - 1)), (v, n)
        self.bits(v & ((1 << n) - 1), n)

    def unary(self, q):
        self.bits(1, q + 1)

    def align(self, fill=0):
        pad = -self.n % 8
        self.bits(fill & ((1 << pad) - 1), pad)

    def bytes(self):
        assert self.n % 8 == 0
        return self.acc.to_bytes(self.n // 8, "big")


def fold(e):
    return (e << 1) if e >= 0 else ((-e - 1) << 1) | 1


def rice_bits(residuals, k):
    return sum((fold(e) >> k) + 1 + k for e in residuals)


def best_k(residuals, limit):
    return min(range(limit), key=lambda k: rice_bits(residuals, k))


def write_residual(w, residuals, n, order, *, rice2=False, partition_order=0, escapes=(), params=None):
    """escapes: partitions written raw (at the least width that holds them: 0 bits for all zeros); params: {partition: k}."""
    width = 5 if rice2 else 4
    w.bits(1 if rice2 else 0, 2)
    w.bits(partition_order, 4)
    assert (n >> partition_order) << partition_order == n and (n >> partition_order) >= order
    at = 0
    for part in range(1 << partition_order):
        count = (n >> partition_order) - (order if part == 0 else 0)
        chunk = residuals[at:at + count]
        at += count
        if part in escapes:
            w.bits((1 << width) - 1, width)
            raw = 0 if not any(chunk) else max(max(e.bit_length() for e in chunk if e >= 0) if any(e >= 0 for e in chunk) else 0,
                                                 max((-e - 1).bit_length() for e in chunk if e < 0) if any(e < 0 for e in chunk) else 0) + 1
            w.bits(raw, 5)
            for e in chunk:
                w.signed(e, raw)
        else:
            k = (params or {}).get(part, best_k(chunk, (1 << width) - 1))
            w.bits(k, width)
            for e in chunk:
                u = fold(e)
                w.unary(u >> k)
                w.bits(u & ((1 << k) - 1), k)
    assert at == len(residuals)


FIXED_TAPS = ([], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1])


def write_subframe(w, samples, bps, spec):
    """spec: dict(type='constant'|'verbatim'|'fixed'|'lpc', order=, coefs=, precision=, shift=, wasted=, and write_residual's options)."""
    spec = dict(spec)
    kind, wasted = spec.pop("type"), spec.pop("wasted", 0)
    n = len(samples)
    if wasted:
        assert all(s % (1 << wasted) == 0 for s in samples)
        samples = [s >> wasted for s in samples]
        bps -= wasted
    w.bits(0, 1)
    order = spec.pop("order", 0)
    code = {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}[kind]
    w.bits(code, 6)
    w.bits(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
    if kind == "constant":
        assert len(set(samples)) == 1
        w.signed(samples[0], bps)
        return
    if kind == "verbatim":
        for s in samples:
            w.signed(s, bps)
        return
    for s in samples[:order]:
        w.signed(s, bps)
    if kind == "fixed":
        taps, shift = FIXED_TAPS[order], 0
    else:
        taps, shift, precision = spec.pop("coefs"), spec.pop("shift"), spec.pop("precision")
        assert len(taps) == order
        w.bits(precision - 1, 4)
        w.signed(shift, 5)
        for c in taps:
            w.signed(c, precision)
    residuals = [samples[i] - (sum(t * samples[i - 1 - j] for j, t in enumerate(taps)) >> shift) for i in range(order, n)]
    write_residual(w, residuals, n, order, **spec)


BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
SIZE_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


def coded_number(v):
    if v < 0x80:
        return bytes([v])
    for extra in range(1, 7):
        if v < 1 << (5 * extra + 6) or extra == 6:
            lead = (0xff << (7 - extra)) & 0xff
            out = [lead | (v >> (6 * extra))] if extra < 6 else [0xfe]
            return bytes(out + [0x80 | ((v >> (6 * k)) & 0x3f) for k in range(extra - 1, -1, -1)])


def header_bytes(blocksize, rate, number, *, variable, assignment, bits, rate_form="auto", size_from_streaminfo=False):
    """rate_form: 'auto' (a direct code where there is one), 'streaminfo' (code 0), 'khz', 'hz', 'tens' (the three trailers)."""
    bs_code = BS_CODES.get(blocksize, 6 if blocksize <= 256 else 7)
    if rate_form == "auto":
        rate_form = "direct" if rate in RATE_CODES else "hz"
    rate_code = {"direct": RATE_CODES.get(rate), "streaminfo": 0, "khz": 12, "hz": 13, "tens": 14}[rate_form]
    w = BitWriter()
    w.bits(0x3ffe, 14)
    w.bits(0, 1)
    w.bits(1 if variable else 0, 1)
    w.bits(bs_code, 4)
    w.bits(rate_code, 4)
    w.bits(assignment, 4)
    w.bits(0 if size_from_streaminfo else SIZE_CODES[bits], 3)
    w.bits(0, 1)
    for b in coded_number(number):
        w.bits(b, 8)
    if bs_code == 6:
        w.bits(blocksize - 1, 8)
    elif bs_code == 7:
        w.bits(blocksize - 1, 16)
    if rate_code == 12:
        assert rate % 1000 == 0
        w.bits(rate // 1000, 8)
    elif rate_code == 13:
        w.bits(rate, 16)
    elif rate_code == 14:
        assert rate % 10 == 0
        w.bits(rate // 10, 16)
    head = w.bytes()
    return head + bytes([crc8(head)])


def frame(channels, bits, rate, number, specs, *, variable=False, stereo=None, padding=0, **header_options):
    """channels: the FINAL samples, one list per channel.  stereo: None (independent) or 'left_side' / 'right_side' / 'mid_side'.
    specs: one subframe spec per channel.  padding: the bits in front of the CRC-16 (anything but 0 makes a frame decoders refuse)."""
    n = len(channels[0])
    if stereo is None:
        assignment, coded, depth = len(channels) - 1, channels, [bits] * len(channels)
    else:
        left, right = channels
        side = [a - b for a, b in zip(left, right)]
        assignment = {"left_side": 8, "right_side": 9, "mid_side": 10}[stereo]
        coded = {8: [left, side], 9: [side, right], 10: [[(a + b) >> 1 for a, b in zip(left, right)], side]}[assignment]
        depth = {8: [bits, bits + 1], 9: [bits + 1, bits], 10: [bits, bits + 1]}[assignment]
    w = BitWriter()
    for b in header_bytes(n, rate, number, variable=variable, assignment=assignment, bits=bits, **header_options):
        w.bits(b, 8)
    for samples, bps, spec in zip(coded, depth, specs):
        write_subframe(w, samples, bps, spec)
    w.align(padding)
    body = w.bytes()
    return body + crc16(body).to_bytes(2, "big")


def stream(frames, pcm, bits, rate, channels, *, min_blocksize, max_blocksize, total_samples=None):
    """'fLaC' + STREAMINFO (MD5 of pcm: the samples that went in, [frames][channels]) + the frames."""
    nb = (bits + 7) // 8
    m = hashlib.md5()
    m.update(b"".join((v & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little") for row in pcm for v in row))
    total = len(pcm) if total_samples is None else total_samples
    sizes = [len(f) for f in frames]
    v = (rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total
    info = min_blocksize.to_bytes(2, "big") + max_blocksize.to_bytes(2, "big") + min(sizes).to_bytes(3, "big") + max(sizes).to_bytes(3, "big") \
        + v.to_bytes(8, "big") + m.digest()
    assert len(info) == 34
    return b"fLaC" + bytes([0x80]) + (34).to_bytes(3, "big") + info + b"".join(frames)
