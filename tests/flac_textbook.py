"""A plain-Python FLAC frame decoder written from the format's definition, one bit at a time, Python integers only: the
independent model the device decoder (csrc/flac_frame_kernel.hip) and its CPU build are held against.  TEST INFRASTRUCTURE ONLY;
it imports neither the product, nor ctypes, nor the oracle.

What it models is the contract of include/ohgpu.h's FLAC section:

  candidate   a byte position of the range whose header has the sync code, only legal codes, a well-formed coded number and a
              matching CRC-8
  probe       the candidate parsed to its end: every field legal, the channel count the stream's, the block size within the
              stream's maximum, zero padding bits, a matching CRC-16; running out of range first is "need more", not an error
  chain       the lowest candidate that passes (at_frame: the one at the range's start), then each time the candidate that starts
              where the last frame ended; it must have the stream's channels, depth and rate, the first frame's blocking strategy, a
              block no larger than the stream's under fixed blocking, and the next number.  The chain ends OK at the range's end or at
              "need more", CORRUPT at anything else, UNSUPPORTED at a 12- or 20-bit frame, OVERFLOW at a frame outside
              [first_sample, first_sample + max_samples)

Padding bits: a frame whose padding in front of the CRC-16 is not zero FAILS.  This is what the reference's libFLAC 1.2.1 does with
a handmade stream (tests/golden/make_flac_decode_fixtures.py checks it where oracle/_ref exists: the decoder reports a lost sync at
such a frame and delivers nothing of it), so the model, and the product, refuse it.

Sample arithmetic is exact (Python integers) and a stored sample is the low 32 bits of the result, two's complement: on a
well-formed stream nothing is ever cut off; on a malformed one this is what a 64-bit sum kept in 32 bits gives."""
import collections
import hashlib

OK, CORRUPT, UNSUPPORTED, OVERFLOW = 0, 1, 2, 3
MAX_BYTES_AHEAD = 16          # the longest header: 2 + 2 + 7 + 2 + 2 + 1


class NeedMore(Exception):
    pass


class Illegal(Exception):
    pass


class Bits:
    """Bits of data[start:end], most significant first, one at a time."""

    def __init__(self, data, start, end):
        self.data, self.at, self.end = data, start * 8, end * 8

    def bit(self):
        if self.at >= self.end:
            raise NeedMore()
        b = (self.data[self.at >> 3] >> (7 - (self.at & 7))) & 1
        self.at += 1
        return b

    def unsigned(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def signed(self, n):
        if n == 0:
            return 0
        v = self.unsigned(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        q = 0
        while self.bit() == 0:
            q += 1
        return q

    def aligned(self):
        return self.at % 8 == 0

    def byte_pos(self):
        assert self.at % 8 == 0
        return self.at // 8


def crc(data, width, poly):
    """Remainder of data * X^width by the polynomial, bit by bit."""
    r, top, mask = 0, 1 << (width - 1), (1 << width) - 1
    for byte in data:
        for k in range(7, -1, -1):
            fed = ((byte >> k) & 1) ^ (1 if r & top else 0)
            r = (r << 1) & mask
            if fed:
                r ^= poly
    return r


def crc8(data):
    return crc(data, 8, 0x07)


def crc16(data):
    return crc(data, 16, 0x8005)


def wrap32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def streaminfo(data):
    """(dict, offset of the first frame): 'fLaC', the metadata blocks, STREAMINFO first.  ValueError on anything else."""
    if len(data) < 4 or bytes(data[:4]) != b"fLaC":
        raise ValueError("no fLaC marker")
    at, info = 4, None
    while True:
        if len(data) - at < 4:
            raise ValueError("ends inside the metadata")
        last, kind = data[at] >> 7, data[at] & 0x7f
        length = int.from_bytes(data[at + 1:at + 4], "big")
        at += 4
        if len(data) - at < length:
            raise ValueError("ends inside the metadata")
        if info is None:
            if kind != 0 or length != 34:
                raise ValueError("the first block is not STREAMINFO")
            b = data[at:at + 34]
            v = int.from_bytes(b[10:18], "big")
            info = dict(min_blocksize=int.from_bytes(b[0:2], "big"), max_blocksize=int.from_bytes(b[2:4], "big"),
                        min_framesize=int.from_bytes(b[4:7], "big"), max_framesize=int.from_bytes(b[7:10], "big"),
                        sample_rate=v >> 44, channels=((v >> 41) & 7) + 1, bits=((v >> 36) & 31) + 1,
                        total_samples=v & ((1 << 36) - 1), md5=bytes(b[18:34]))
        at += length
        if last:
            return info, at


BLOCK_SIZES = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
DEPTHS = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}
ASSIGNMENTS = {8: "left_side", 9: "right_side", 10: "mid_side"}

Header = collections.namedtuple("Header", "variable blocksize rate channels assignment bits number length bs_code rate_code size_code number_bytes")


def read_header(data, pos, end, cfg):
    """The frame header at data[pos:end]: Header, or Illegal / NeedMore."""
    rd = Bits(data, pos, end)
    if rd.unsigned(14) != 0x3ffe:
        raise Illegal("sync")
    if rd.bit():
        raise Illegal("reserved bit")
    variable = rd.bit()
    bs_code, rate_code, asg, size_code = rd.unsigned(4), rd.unsigned(4), rd.unsigned(4), rd.unsigned(3)
    if rd.bit():
        raise Illegal("reserved bit")
    if bs_code == 0 or rate_code == 15 or asg > 10 or size_code in (3, 7):
        raise Illegal("reserved code")
    lead = rd.unsigned(8)
    ones = 0
    while ones < 8 and (lead >> (7 - ones)) & 1:
        ones += 1
    if ones == 1 or ones == 8:
        raise Illegal("coded number")
    number = lead & (0xff >> (ones + 1)) if ones else lead
    for _ in range(max(ones - 1, 0)):
        c = rd.unsigned(8)
        if c >> 6 != 2:
            raise Illegal("coded number")
        number = (number << 6) | (c & 0x3f)
    if bs_code == 6:
        blocksize = rd.unsigned(8) + 1
    elif bs_code == 7:
        blocksize = rd.unsigned(16) + 1
    else:
        blocksize = BLOCK_SIZES[bs_code]
    if rate_code == 0:
        rate = cfg["sample_rate"]
    elif rate_code == 12:
        rate = rd.unsigned(8) * 1000
    elif rate_code == 13:
        rate = rd.unsigned(16)
    elif rate_code == 14:
        rate = rd.unsigned(16) * 10
    else:
        rate = RATES[rate_code]
    here = rd.byte_pos()
    if rd.unsigned(8) != crc8(data[pos:here]):
        raise Illegal("CRC-8")
    return Header(variable, blocksize, rate, asg + 1 if asg < 8 else 2, asg, cfg["bits"] if size_code == 0 else DEPTHS[size_code],
                  number, here + 1 - pos, bs_code, rate_code, size_code, max(ones, 1))


def candidate(data, pos, end, cfg):
    """'yes', 'no', or 'open' (the range ends before the header does and nothing so far speaks against it)."""
    try:
        read_header(data, pos, min(end, pos + MAX_BYTES_AHEAD), cfg)
        return "yes"
    except Illegal:
        return "no"
    except NeedMore:
        return "open"


def read_residual(rd, n, order, census):
    method = rd.unsigned(2)
    if method > 1:
        raise Illegal("residual method")
    width = 4 + method
    po = rd.unsigned(4)
    if order > n or (po and ((n >> po) << po != n or (n >> po) < order)):
        raise Illegal("partition")
    census["method:" + ("RICE", "RICE2")[method]] += 1
    census["partition_order:%d" % po] += 1
    out = []
    for part in range(1 << po):
        count = (n >> po) - (order if part == 0 else 0)
        k = rd.unsigned(width)
        if k == (1 << width) - 1:
            raw = rd.unsigned(5)
            census["escape:0" if raw == 0 else "escape:>0"] += 1
            out.extend(rd.signed(raw) for _ in range(count))
        else:
            census[("rice:%d", "rice2:%d")[method] % k] += 1
            for _ in range(count):
                u = (rd.unary() << k) | rd.unsigned(k)
                if u >> 32:
                    raise Illegal("residual out of range")
                out.append(-(u >> 1) - 1 if u & 1 else u >> 1)
    return out


def read_subframe(rd, n, bps, census):
    """One channel's samples (before decorrelation), low 32 bits each."""
    pad, kind, has_wasted = rd.bit(), rd.unsigned(6), rd.bit()      # (the header's eight bits are read, then judged)
    if pad:
        raise Illegal("subframe padding")
    wasted = 0
    if has_wasted:
        wasted = rd.unary() + 1
        if wasted >= bps:
            raise Illegal("wasted bits")
        bps -= wasted
    if kind == 0:
        census["sub:CONSTANT"] += 1
        s = [rd.signed(bps)] * n
    elif kind == 1:
        census["sub:VERBATIM"] += 1
        s = [rd.signed(bps) for _ in range(n)]
    elif 8 <= kind <= 12:
        order = kind - 8
        if order > n:
            raise Illegal("order")
        census["sub:FIXED:%d" % order] += 1
        s = [rd.signed(bps) for _ in range(order)]
        taps = ([], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1])[order]
        for e in read_residual(rd, n, order, census):
            s.append(wrap32(e + sum(t * s[-1 - j] for j, t in enumerate(taps))))
    elif kind >= 32:
        order = kind - 31
        if order > n:
            raise Illegal("order")
        s = [rd.signed(bps) for _ in range(order)]
        precision = rd.unsigned(4) + 1
        shift = rd.signed(5)
        if precision == 16 or shift < 0:
            raise Illegal("LPC parameters")
        census["sub:LPC:%d" % order] += 1
        census["sub:LPC:%d:precision:%d" % (order, precision)] += 1
        coef = [rd.signed(precision) for _ in range(order)]
        for e in read_residual(rd, n, order, census):
            s.append(wrap32(e + (sum(c * s[-1 - j] for j, c in enumerate(coef)) >> shift)))
    else:
        raise Illegal("reserved subframe type")
    if wasted:
        s = [wrap32(v << wasted) for v in s]
    return s, wasted


Frame = collections.namedtuple("Frame", "pos end header planes census")


def read_frame(data, pos, end, cfg, census=None):
    """The whole frame at data[pos:end] -> Frame (planes: the decoded channels), or Illegal / NeedMore."""
    census = collections.Counter() if census is None else census
    mine = collections.Counter()
    h = read_header(data, pos, end, cfg)
    if h.blocksize > cfg["max_blocksize"] or h.channels != cfg["channels"]:
        raise Illegal("not a frame of this stream")
    rd = Bits(data, pos + h.length, end)
    coded, wasted = [], []
    for c in range(h.channels):
        side = (h.assignment, c) in ((8, 1), (9, 0), (10, 1))
        s, w = read_subframe(rd, h.blocksize, h.bits + (1 if side else 0), mine)
        coded.append(s)
        wasted.append(w)
    while not rd.aligned():
        if rd.bit():
            raise Illegal("padding")
    here = rd.byte_pos()
    if rd.unsigned(16) != crc16(data[pos:here]):
        raise Illegal("CRC-16")
    if h.assignment == 8:
        planes = [coded[0], [wrap32(a - b) for a, b in zip(*coded)]]
    elif h.assignment == 9:
        planes = [[wrap32(a + b) for a, b in zip(*coded)], coded[1]]
    elif h.assignment == 10:
        planes = [[], []]
        for m, s in zip(*coded):
            m = (m << 1) | (s & 1)
            planes[0].append(wrap32((m + s) >> 1))
            planes[1].append(wrap32((m - s) >> 1))
    else:
        planes = coded
    mine["assignment:" + ASSIGNMENTS.get(h.assignment, "independent")] += 1
    mine["channels:%d" % h.channels] += 1
    mine["bits:%d" % h.bits] += 1
    mine["blocksize:%d" % h.blocksize] += 1
    mine["blocksize_code:%d" % h.bs_code] += 1
    mine["rate_code:%d" % h.rate_code] += 1
    mine["blocking:" + ("variable" if h.variable else "fixed")] += 1
    mine["number_bytes:%d" % h.number_bytes] += 1
    if h.channels == 2 and (wasted[0] == 0) != (wasted[1] == 0):
        mine["wasted:one_of_a_pair"] += 1
    if any(wasted):
        mine["wasted:any"] += 1
    census.update(mine)
    return Frame(pos, rd.byte_pos(), h, planes, mine)


Result = collections.namedtuple("Result", "status frames samples first_sample_decoded bytes_consumed candidates candidates_rejected census places")


def decode_range(data, offset, nbytes, *, channels, bits, sample_rate, max_blocksize, max_samples, blocksize=0, first_sample=0, at_frame=False):
    """The chain over data[offset:offset + nbytes].  Result.frames: the accepted Frames (pos / end relative to offset);
    Result.places: each one's first sample's index in the output."""
    cfg = dict(channels=channels, bits=bits, sample_rate=sample_rate, max_blocksize=max_blocksize)
    end = offset + nbytes
    probes, n_candidates = {}, 0
    for pos in range(offset, end):
        if data[pos] != 0xff:
            continue
        kind = candidate(data, pos, end, cfg)
        if kind == "no":
            continue
        n_candidates += kind == "yes"
        try:
            probes[pos] = read_frame(data, pos, end, cfg, collections.Counter())
        except NeedMore:
            probes[pos] = "open"
        except Illegal:
            probes[pos] = "bad"
    order = sorted(probes)
    opens = [p for p in order if probes[p] == "open"]
    passing = [p for p in order if isinstance(probes[p], Frame)]
    status, consumed, start = OK, nbytes, None
    if at_frame:
        here = probes.get(offset, "bad")
        if here == "open":
            consumed = 0
        elif here == "bad":
            status, consumed = (CORRUPT if nbytes else OK), 0
        else:
            start = offset
    elif passing:
        start = passing[0]
    elif opens:
        consumed = opens[0] - offset
    frames, places, census, samples, first_decoded = [], [], collections.Counter(), 0, 0
    if start is not None:
        first = probes[start]
        stream_bs = blocksize or first.header.blocksize
        at, expect = start, None
        while True:
            f = probes[at]
            h = f.header
            if h.bits not in (8, 16, 24):
                status, consumed = UNSUPPORTED, at - offset
                break
            fits = (h.channels, h.bits, h.rate, h.variable) == (channels, bits, sample_rate, first.header.variable)
            fits = fits and (h.variable or h.blocksize <= stream_bs) and (expect is None or h.number == expect)
            if not fits:
                status, consumed = CORRUPT, at - offset
                break
            s0 = h.number if h.variable else h.number * stream_bs
            if s0 < first_sample or s0 - first_sample + h.blocksize > max_samples:
                status, consumed = OVERFLOW, at - offset
                break
            if not frames:
                first_decoded = s0
            frames.append(f._replace(pos=f.pos - offset, end=f.end - offset))
            places.append(s0 - first_sample)
            samples += h.blocksize
            census.update(f.census)
            consumed = f.end - offset
            expect = h.number + (h.blocksize if h.variable else 1)
            if f.end >= end:
                break
            nxt = probes.get(f.end, "bad")
            if nxt == "open":
                break
            if nxt == "bad":
                status = CORRUPT
                break
            at = f.end
    return Result(status, frames, samples, first_decoded, consumed, n_candidates, n_candidates - len(frames), census, places)


def render(result, arena, *, dst_offset, channels, bits, packed, dst_plane_stride=0):
    """Writes the accepted frames into arena (a bytearray / uint8 buffer) the way the device does: planes of host-endian (little)
    int32, or interleaved big-endian at bits / 8 bytes."""
    nb = bits // 8
    for f, place in zip(result.frames, result.places):
        for c, plane in enumerate(f.planes):
            for i, v in enumerate(plane):
                if packed:
                    at = dst_offset + ((place + i) * channels + c) * nb
                    arena[at:at + nb] = (v & ((1 << bits) - 1)).to_bytes(nb, "big")
                else:
                    at = dst_offset + c * dst_plane_stride + (place + i) * 4
                    arena[at:at + 4] = (v & 0xffffffff).to_bytes(4, "little")


def md5_of(frames, bits):
    """The MD5 STREAMINFO carries: of the samples, interleaved, little-endian, at the depth rounded up to whole bytes."""
    nb = (bits + 7) // 8
    m = hashlib.md5()
    for f in frames:
        buf = bytearray()
        for i in range(f.header.blocksize):
            for plane in f.planes:
                buf += (plane[i] & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
        m.update(bytes(buf))
    return m.digest()


def decode_file(data):
    """A whole file: (info, Result) with the descriptor its STREAMINFO gives."""
    info, audio = streaminfo(data)
    res = decode_range(data, audio, len(data) - audio, channels=info["channels"], bits=info["bits"], sample_rate=info["sample_rate"],
                       max_blocksize=info["max_blocksize"], max_samples=max(info["total_samples"], 1), at_frame=True)
    return info, res
