"""A plain-Python Apple Lossless packet decoder: the tests' independent model of csrc/alac_packet_core.h.

It reads one bit at a time, keeps every number a Python int and narrows it only where the format does, through wrap16 / wrap32;
the predictor works from one list into another.  It imports nothing from the library or the oracle.

Statuses: OK, CORRUPT, UNSUPPORTED.  Where the model (and the library) is stricter than the reference decoder:
  * bits past the packet's end read as zero, and an element that needed one is CORRUPT (the reference reads up to four bytes on);
  * a compressed element's sample width (depth - 8 * shifted bytes, plus one for a pair) outside 1..32 is CORRUPT;
  * a sample count above the stream's frame length, or audio elements of one packet that disagree about it, is CORRUPT;
  * depth 20 is UNSUPPORTED (the reference's caller counts two bytes a sample where its decoder writes three), so is any depth
    but 16 / 24 / 32, and a kb outside 1..31;
  * a rounding shift (denShift) of zero rounds with nothing; a matrix shift (mixBits) above 31 shifts by 31;
  * an escaped element carries `depth` bits a sample whatever its shift field says;
  * a failed packet yields no samples at all.
"""
import struct

OK, CORRUPT, UNSUPPORTED = 0, 1, 2
PLANAR, PACKED_LE, PACKED_BE = 0, 1, 2
MAX_FRAME_LENGTH = 16384


def wrap32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x & 0x80000000 else x


def wrap16(x):
    x &= 0xffff
    return x - (1 << 16) if x & 0x8000 else x


def u32(x):
    return x & 0xffffffff


def narrow(x, width):
    """x's low `width` bits, read as a signed number"""
    x &= (1 << width) - 1
    return x - (1 << width) if x >> (width - 1) else x


class Corrupt(Exception):
    pass


def parse_config(cookie):
    """The 24-byte configuration, behind an optional 'frma' atom and / or 'alac' atom header of 12 bytes each."""
    c = bytes(cookie)
    for name in (b"frma", b"alac"):
        if len(c) >= 12 and c[4:8] == name:
            c = c[12:]
    if len(c) < 24:
        raise ValueError("configuration shorter than 24 bytes")
    frame_length, version, depth, pb, mb, kb, channels, max_run, max_frame_bytes, avg_bit_rate, sample_rate = struct.unpack(">IBBBBBBHIII", c[:24])
    if version != 0:
        raise ValueError("compatible version %d" % version)
    return dict(frame_length=frame_length, bit_depth=depth, pb=pb, mb=mb, kb=kb, channels=channels, max_run=max_run,
                max_frame_bytes=max_frame_bytes, avg_bit_rate=avg_bit_rate, sample_rate=sample_rate)


class Reader:
    def __init__(self, data):
        self.data = bytes(data)
        self.nbits = 8 * len(self.data)
        self.pos = 0

    def bit(self):
        at = self.pos
        self.pos += 1
        if at >= self.nbits:
            return 0
        return (self.data[at >> 3] >> (7 - (at & 7))) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = (v << 1) | self.bit()
        return v

    def ones(self, most):
        """ones in front, at most `most` of them; the zero that ends fewer is consumed"""
        n = 0
        while n < most:
            if self.bit() == 0:
                return n
            n += 1
        return n

    def short_bits(self, k):
        """k bits whose values 0 and 1 are written one bit shorter; 0 for those, value - 1 otherwise"""
        high = self.bits(k - 1)
        if high == 0:
            return 0
        return high * 2 + self.bit() - 1

    @property
    def dry(self):
        return self.pos > self.nbits


def ilog2(x):
    return x.bit_length() - 1


def read_residuals(r, cfg, pb, width, n, seen):
    kb = cfg["kb"]
    mean, after_run, out = cfg["mb"], 0, []
    while len(out) < n:
        k = min(ilog2((mean >> 9) + 3), kb)
        step = (1 << k) - 1
        prefix = r.ones(9)
        if prefix == 9:
            v = r.bits(width)
            seen.add("long_escape")
        else:
            v = prefix * step
            if k > 1:
                v += r.short_bits(k)
        coded = u32(v + after_run)
        half = u32(coded + 1) >> 1
        out.append(wrap32(-half if coded & 1 else half))
        mean = u32(pb * coded + mean - (u32(pb * mean) >> 9))
        if v > 0xffff:
            mean = 0xffff
        after_run = 0
        if u32(mean << 2) < 512 and len(out) < n:
            after_run = 1
            kz = (32 - mean.bit_length()) - 24 + ((mean + 16) >> 6)
            stepz = ((1 << kz) - 1) & ((1 << kb) - 1)
            prefix = r.ones(9)
            if prefix == 9:
                run = r.bits(16)
                seen.add("run_escape")
            else:
                run = prefix * stepz + r.short_bits(kz)
            if run > n - len(out):
                raise Corrupt("a run of %d zeros with %d samples to go" % (run, n - len(out)))
            if run:
                seen.add("zero_run")
            out.extend([0] * run)
            if run >= 65535:
                after_run = 0
            mean = 0
        if r.dry:
            raise Corrupt("the residuals run past the packet")
    return out


def sign_of(v):
    return (v > 0) - (v < 0)


def predict(res, coef, order, width, den_shift):
    """one pass of the predictor over the residuals `res`; coef is adapted in place"""
    n = len(res)
    if order == 0 or n == 0:
        return list(res)
    out = [res[0]]
    if order == 31:
        for j in range(1, n):
            out.append(narrow(wrap32(res[j] + out[j - 1]), width))
        return out
    for j in range(1, min(order + 1, n)):
        out.append(narrow(wrap32(res[j] + out[j - 1]), width))
    lim = order + 1
    half = (1 << (den_shift - 1)) if den_shift else 0
    for j in range(lim, n):
        top = out[j - lim]
        total = 0
        for k in range(order):
            total = wrap32(total + wrap32(coef[k] * wrap32(out[j - 1 - k] - top)))
        out.append(narrow(wrap32(res[j] + top + (wrap32(total + half) >> den_shift)), width))
        left = res[j]
        sg = sign_of(left)
        if sg == 0:
            continue
        for k in range(order - 1, -1, -1):
            dd = wrap32(top - out[j - 1 - k])
            sgn = sign_of(dd)
            if sg > 0:
                coef[k] = wrap16(coef[k] - sgn)
                left = wrap32(left - wrap32((order - k) * (wrap32(sgn * dd) >> den_shift)))
                if left <= 0:
                    break
            else:
                coef[k] = wrap16(coef[k] + sgn)
                left = wrap32(left - wrap32((order - k) * (wrap32(-sgn * dd) >> den_shift)))
                if left >= 0:
                    break
    return out


def order_class(order):
    return {0: "order_0", 4: "order_4", 8: "order_8", 31: "order_31"}.get(order, "order_other")


def decode_packet(cfg, data, seen=None):
    """-> (status, samples, channels): channels[c][i], each sample a signed number of cfg's depth; [] unless status is OK"""
    seen = set() if seen is None else seen
    try:
        n, chans = _decode(cfg, data, seen)
    except Corrupt:
        return CORRUPT, 0, []
    except NotImplementedError:
        return UNSUPPORTED, 0, []
    return OK, n, chans


def _decode(cfg, data, seen):
    depth, channels = cfg["bit_depth"], cfg["channels"]
    if depth not in (16, 24, 32) or not 1 <= cfg["kb"] <= 31:
        raise NotImplementedError
    r = Reader(data)
    out = []
    n, count = cfg["frame_length"], None
    while len(out) < channels:
        if r.pos >= r.nbits:
            raise Corrupt("the packet ends with channels missing")
        tag = r.bits(3)
        if tag == 7:
            if r.dry:
                raise Corrupt("end tag cut")
            seen.add("early_END")
            break
        if tag in (2, 5):
            raise Corrupt("element %d" % tag)
        if tag == 4:
            r.bits(4)
            align = r.bit()
            size = r.bits(8)
            if size == 255:
                size += r.bits(8)
            if align:
                while r.pos & 7:
                    r.pos += 1
            r.pos += 8 * size
            if r.dry:
                raise Corrupt("data element cut")
            seen.add("DSE_aligned" if align else "DSE")
            continue
        if tag == 6:
            size = r.bits(4)
            if size == 15:
                size += r.bits(8) - 1
            r.pos += 8 * size
            if r.dry:
                raise Corrupt("fill element cut")
            seen.add("FIL")
            continue
        pair = tag == 1
        nch = 2 if pair else 1
        if len(out) + nch > channels:
            seen.add("CPE_beyond_channels")
            break
        seen.add({0: "SCE", 1: "CPE", 3: "LFE"}[tag])
        r.bits(4)
        if r.bits(12) != 0:
            raise Corrupt("header bits set")
        partial, shifted, escape = r.bit(), r.bits(2), r.bit()
        if shifted == 3:
            raise Corrupt("three bytes shifted")
        if partial:
            n = r.bits(32)
            seen.add("partial")
        if r.dry:
            raise Corrupt("element header cut")
        if n > cfg["frame_length"] or (count is not None and n != count):
            raise Corrupt("sample count %d" % n)
        count = n
        width = depth - 8 * shifted + (1 if pair else 0)
        if not escape and not 1 <= width <= 32:
            raise Corrupt("sample width %d" % width)
        if escape:
            seen.add("escape")
            if shifted:
                seen.add("escape_with_shift")
            if r.pos + n * nch * depth > r.nbits:
                raise Corrupt("escaped samples cut")
            got = [[] for _ in range(nch)]
            for _ in range(n):
                for c in range(nch):
                    got[c].append(narrow(r.bits(depth), depth))
            out.extend(got)
            continue
        seen.add("shift_%d" % shifted)
        mix_bits = r.bits(8)
        mix_res = narrow(r.bits(8), 8)
        params = []
        for _ in range(nch):
            mode, den_shift, factor, order = r.bits(4), r.bits(4), r.bits(3), r.bits(5)
            coef = [wrap16(r.bits(16)) for _ in range(order)]
            params.append((mode, den_shift, factor, order, coef))
            seen.add(order_class(order))
            if mode:
                seen.add("mode")
            if factor != 4:
                seen.add("factor_not_4")
        if r.dry:
            raise Corrupt("element parameters cut")
        low = [[] for _ in range(nch)]
        if shifted:
            if r.pos + n * nch * 8 * shifted > r.nbits:
                raise Corrupt("shifted-off bytes cut")
            for _ in range(n):
                for c in range(nch):
                    low[c].append(r.bits(8 * shifted))
        rows = []
        for mode, den_shift, factor, order, coef in params:
            res = read_residuals(r, cfg, (cfg["pb"] * factor) // 4, width, n, seen)
            if mode:
                res = predict(res, None, 31, width, 0)
            rows.append(predict(res, coef, order, width, den_shift))
        if pair:
            seen.add("mix" if mix_res else "mix_0")
            if mix_res:
                u, v = rows
                left = [wrap32(u[i] + v[i] - (wrap32(mix_res * v[i]) >> min(mix_bits, 31))) for i in range(n)]
                rows = [left, [wrap32(left[i] - v[i]) for i in range(n)]]
        for c in range(nch):
            if shifted:
                rows[c] = [wrap32(rows[c][i] << (8 * shifted)) | low[c][i] for i in range(n)]
            out.append([narrow(x, depth) for x in rows[c]])
    while len(out) < channels:
        out.append([0] * n)
    return n, out


def pack(cfg, chans, n, form):
    """one packet's samples in an output form: PLANAR -> a list of per-channel host-endian int32 byte strings; packed -> bytes"""
    depth = cfg["bit_depth"]
    if form == PLANAR:
        return [struct.pack("<%di" % n, *chans[c][:n]) for c in range(len(chans))]
    size = depth // 8
    order = "little" if form == PACKED_LE else "big"
    out = bytearray()
    for i in range(n):
        for c in range(len(chans)):
            out += (chans[c][i] & ((1 << depth) - 1)).to_bytes(size, order)
    return bytes(out)


def render(cfg, packets, form, dst, dst_offset, plane_stride, decode_packet=decode_packet):
    """Decode a stream's packets into the bytearray `dst` the way a descriptor of the library does: packet p at sample p * frame_length.
    -> [(status, samples)] per packet.  A packet that fails leaves its part of dst alone."""
    results = []
    depth, channels, fl = cfg["bit_depth"], cfg["channels"], cfg["frame_length"]
    for p, data in enumerate(packets):
        status, n, chans = decode_packet(cfg, data)
        results.append((status, n))
        if status != OK:
            continue
        if form == PLANAR:
            for c, plane in enumerate(pack(cfg, chans, n, form)):
                at = dst_offset + c * plane_stride + p * fl * 4
                dst[at:at + len(plane)] = plane
        else:
            at = dst_offset + p * fl * channels * (depth // 8)
            body = pack(cfg, chans, n, form)
            dst[at:at + len(body)] = body
    return results
