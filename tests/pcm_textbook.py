"""The PCM message path of one descriptor (oracle_lib.MSG_DESC), one subsample at a time, on plain Python integers.

Written from the operation's definition in SURVEY.md 8a (rows a1, a6, a7, a9, a11, a12) and DESIGN.md, NOT from oracle/*.c or
the kernels: no ctypes, no import of oracle_lib, no batching, no chunking, no magic division, no byte shuffles.  It is slow on
purpose.  tests/test_pcm_textbook.py holds it equal to the oracle byte for byte; tests/test_gpu_pcm_textbook.py holds the device
equal to it.

The operation, per subsample q of a message of `n_frames` frames of `channels` subsamples (frame i = q // channels, channel
c = q % channels):

  1. READ     `src_bits` / 8 bytes at src_offset + q * bytes, in the source byte order, as a signed integer, left-justified in
              32 bits (a1 then a11: the reference keeps audio big-endian and FlywheelInput pads the low bytes with zeros).
  2. ATTENUATE (a6, 16-bit audio only, attenuation != 256): the reference multiplies a TInt16 promoted to TInt by a TUint, so the
              product is taken modulo 2^32 and the division by 256 is an UNSIGNED division that truncates; the quotient's low 16
              bits are the new sample.  (For attenuations up to 256 that equals floor(s * att / 256) -- SURVEY.md 8a row a6.)
  3. RAMP     (a7) frame i of N uses ramp = start when N == 1, else the low 16 bits of start - trunc(i * (start - end) / (N - 1))
              with C's truncation toward zero; index = min(511, (16384 - ramp + 16) >> 5); the subsample's TOP 16 bits, as a
              signed 16-bit number, times the Q15 table entry, shifted right by 15 arithmetically; the low 16 bits of that go back
              as the top two bytes (8-bit audio keeps only the upper of them), every lower byte becomes zero -- except that
              32-bit audio of exactly six channels carries channel << 4 in its fourth byte.
  1'. SILENCE (a9) instead of 1-3: the message is zeros in the SOURCE depth, emitted in cells of at most 9216 bytes rounded down
              to whole frames; with exactly six channels every cell starts with the 32 bytes 0,0,0,0x00, 0,0,0,0x10, ... 0,0,0,0x70
              -- whatever the depth (Msg.cpp's constant is a byte array; at 16 bits the id bytes land in odd subsamples' low bytes).
              A silent message is neither attenuated nor ramped.
  4. WRITE    (a12) the first `dst_bits` / 8 of the four big-endian bytes, reversed for a little-endian destination; with
              ZERO_LSB32 a 32-bit destination's fourth byte is zero.

Ambiguities of the written definition, settled by reading the reference (recorded in tests/test_pcm_textbook.py's docstring):
the attenuation's "/256" (unsigned, see 2) and the silence id bytes at depths other than 32 (see 1').
"""
import json
import os

ENDIAN_LITTLE, ENDIAN_BIG = 1, 2
FLAG_RAMP, FLAG_SILENCE, FLAG_ZERO_LSB32 = 1, 2, 4
RAMP_MAX = 1 << 14
UNITY_ATTENUATION = 256
CELL_BYTES = 9216                       # DecodedAudio::kMaxBytes

_TABLE = None


def ramp_table():
    """RampArray.h's 512 Q15 multipliers, from the committed fixture."""
    global _TABLE
    if _TABLE is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ramp_table_q15.json")
        with open(path) as f:
            _TABLE = [int(v) for v in json.load(f)["values"]]
        assert len(_TABLE) == 512
    return _TABLE


def wrap16(v):
    """The value a C int16_t holds after an assignment of v (two's complement)."""
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def wrap32(v):
    v &= 0xFFFFFFFF
    return v - 0x100000000 if v & 0x80000000 else v


def trunc_div(a, b):
    """C's integer division: the quotient rounded toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def read_subsample(src, offset, bits, endian):
    nbytes = bits // 8
    raw = bytes(src[offset:offset + nbytes])
    assert len(raw) == nbytes, "the message reads beyond its arena"
    value = int.from_bytes(raw, "little" if endian == ENDIAN_LITTLE else "big", signed=True)
    return value << (32 - bits)


def attenuate(v32, attenuation):
    """16-bit audio: (TInt16 promoted to TInt) * TUint is unsigned arithmetic modulo 2^32, divided by 256 as unsigned."""
    s16 = v32 >> 16
    product = (s16 * attenuation) % (1 << 32)
    quotient = product // UNITY_ATTENUATION
    return wrap16(quotient) << 16


def ramp_value(frame, n_frames, start, end):
    if n_frames == 1:
        return start & 0xFFFF
    total = start - end
    return (start - trunc_div(frame * total, n_frames - 1)) & 0xFFFF


def ramp_index(ramp16):
    return min(511, ((RAMP_MAX - ramp16 + 16) % (1 << 32)) >> 5)


def ramp_subsample(v32, bits, channels, channel, multiplier):
    s16 = v32 >> 16                                  # the top 16 bits as a signed number
    product = (s16 * multiplier) >> 15               # Python's >> is arithmetic
    if bits == 8:
        return wrap32(((product >> 8) & 0xFF) << 24)
    out = (product & 0xFFFF) << 16
    if bits == 32 and channels == 6:
        out |= (channel << 4) & 0xFF
    return wrap32(out)


def silence_byte(position, channels, src_bits):
    """Byte `position` of a silent message in its source depth."""
    frame_bytes = channels * (src_bits // 8)
    cell = CELL_BYTES - CELL_BYTES % frame_bytes
    p = position % cell
    if channels == 6 and p < 32 and p % 4 == 3:
        return (p // 4) << 4
    return 0


def write_subsample(v32, dst_bits, dst_endian, zero_lsb32):
    be = list((v32 & 0xFFFFFFFF).to_bytes(4, "big"))
    if dst_bits == 32 and zero_lsb32:
        be[3] = 0
    out = be[:dst_bits // 8]
    if dst_endian == ENDIAN_LITTLE:
        out.reverse()
    return bytes(out)


def process_message(d, src):
    """The destination bytes of one message.  d: a mapping or numpy record with MSG_DESC's fields; src: the source arena."""
    n_frames, channels = int(d["n_frames"]), int(d["channels"])
    src_bits, dst_bits = int(d["src_bits"]), int(d["dst_bits"])
    src_endian, dst_endian = int(d["src_endian"]), int(d["dst_endian"])
    flags, attenuation = int(d["flags"]), int(d["attenuation"])
    start, end, src_offset = int(d["ramp_start"]), int(d["ramp_end"]), int(d["src_offset"])
    assert src_bits in (8, 16, 24, 32) and dst_bits in (8, 16, 24, 32) and channels >= 1
    assert attenuation == UNITY_ATTENUATION or src_bits == 16 or (flags & FLAG_SILENCE)
    sbytes = src_bits // 8
    table = ramp_table()
    out = bytearray()
    for q in range(n_frames * channels):
        frame, channel = q // channels, q % channels
        if flags & FLAG_SILENCE:
            raw = bytes(silence_byte(q * sbytes + k, channels, src_bits) for k in range(sbytes))
            v = int.from_bytes(raw, "big", signed=True) << (32 - src_bits)
        else:
            v = read_subsample(src, src_offset + q * sbytes, src_bits, src_endian)
            if attenuation != UNITY_ATTENUATION:
                v = attenuate(v, attenuation)
            if flags & FLAG_RAMP:
                multiplier = table[ramp_index(ramp_value(frame, n_frames, start, end))]
                v = ramp_subsample(v, src_bits, channels, channel, multiplier)
        out += write_subsample(v, dst_bits, dst_endian, bool(flags & FLAG_ZERO_LSB32))
    return bytes(out)


def process_batch(descs, src, dst):
    """Every message of `descs` in order into the bytearray / uint8 array `dst` (later messages overwrite earlier ones)."""
    for d in descs:
        out = process_message(d, src)
        off = int(d["dst_offset"])
        assert off + len(out) <= len(dst), "the message writes beyond its arena"
        for k, byte in enumerate(out):
            dst[off + k] = byte
    return dst
