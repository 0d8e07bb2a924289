"""numpy int64 model of the pulled resampler: the checker for the pulled path's tests.

It restates the specification, not the library: positions, phase and weight from the Q32.32 position, the interpolated Q28
coefficients, the exact integer dot product, the S24 rounding, then RampApplicator's 24-bit case and the pack of a resampled
message (pcm_device.h ramp_index / ramp_word / store_word).  The table itself is the library's (ohgpu_src_pull_design);
tests/test_src_pull_design.py holds it to its own properties.
"""
import numpy as np

ENDIAN_LITTLE, ENDIAN_BIG = 1, 2
FLAG_RAMP, FLAG_ZERO_LSB32 = 1, 4
RAMP_MAX = 16384
NOMINAL = 1 << 31
MASK32 = (1 << 32) - 1


def step_of(rate_in, rate_out, multiplier=NOMINAL):
    """Q32.32 input frames per output frame: floor(2 * rate_in * multiplier / rate_out)."""
    return (2 * rate_in * multiplier) // rate_out


def multiplier_of(ppm):
    """The fix-1.31 multiplier of a pull of `ppm` parts per million (positive: the input is consumed faster)."""
    return int(round(NOMINAL * (1.0 + ppm * 1e-6)))


def window(pos_frame, pos_frac, step, n_frames, taps):
    """(first, frames): the input frames outputs 0 .. n_frames - 1 of a message read."""
    last = pos_frame + ((pos_frac + (n_frames - 1) * step) >> 32)
    first = max(pos_frame - (taps - 1), 0)
    return first, last - first + 1


def advance(pos_frame, pos_frac, step, k):
    """The position of output k: the position of the remainder of a message split after k outputs."""
    u = pos_frac + k * step
    return pos_frame + (u >> 32), u & MASK32


def decode_s24(data, channels, bits, endian):
    """Packed interleaved PCM -> int64 [frames, channels] in the S24 domain (left-justified to 24 bits, arithmetic shift)."""
    sb = bits // 8
    b = np.frombuffer(np.ascontiguousarray(data, dtype=np.uint8).tobytes(), dtype=np.uint8).reshape(-1, sb).astype(np.int64)
    if endian == ENDIAN_LITTLE and sb > 1:
        b = b[:, ::-1]
    w = np.zeros(b.shape[0], dtype=np.int64)
    for i in range(sb):
        w |= b[:, i] << (24 - 8 * i)
    w = np.where(w >= 1 << 31, w - (1 << 32), w)          # the 32-bit word as signed
    return (w >> 8).reshape(-1, channels)


def resample(table, phases_log2, x, x_first, pos_frame, pos_frac, step, n_frames):
    """S24 outputs [n_frames, channels] of one message.  x: int64 [frames, channels] holding input frames x_first .. ;
    frames before the stream start (negative indices) are zeros; every other frame read must be in x."""
    C = np.asarray(table, dtype=np.int64)
    P, T = (1 << phases_log2), C.shape[1]
    assert C.shape[0] == P + 1
    s = phases_log2
    assert pos_frac + max(n_frames - 1, 0) * step < 1 << 64     # (the library refuses a message whose positions overflow)
    u = np.uint64(pos_frac) + np.arange(n_frames, dtype=np.uint64) * np.uint64(step)
    n = (np.uint64(pos_frame) + (u >> np.uint64(32))).astype(np.int64)
    f = (u & np.uint64(MASK32)).astype(np.int64)
    p = f >> (32 - s)
    w = (f >> (16 - s)) & 0xFFFF
    c = C[p] + (((C[p + 1] - C[p]) * w[:, None]) >> 16)     # [n_frames, T]
    idx = n[:, None] - np.arange(T)[None, :]                   # input frame of tap k
    rel = idx - x_first
    inside = idx >= 0
    assert np.all(rel[inside] >= 0) and np.all(rel[inside] < x.shape[0]), "window does not hold the frames the message reads"
    xs = np.where(inside[:, :, None], x[np.clip(rel, 0, x.shape[0] - 1)], 0)    # [n_frames, T, channels]
    acc = np.einsum("jk,jkc->jc", c, xs)                       # exact: |acc| < 2^53 < 2^63
    y = (acc + (1 << 27)) >> 28
    return np.clip(y, -(1 << 23), (1 << 23) - 1)


def ramp_multipliers(ramp_table, ramp_start, ramp_end, n_frames):
    """RampApplicator::GetNextSample's per-frame Q15 multiplier (Msg.cpp:835-837; pcm_device.h ramp_index)."""
    total = ramp_start - ramp_end
    i = np.arange(n_frames, dtype=np.int64)
    if n_frames == 1:
        ramp = np.full(1, ramp_start, dtype=np.int64)
    else:
        prod = i * total
        q = np.sign(prod) * (np.abs(prod) // (n_frames - 1))    # C division: toward zero
        ramp = ramp_start - q
    ramp &= 0xFFFF
    idx = ((RAMP_MAX - ramp + 16) & MASK32) >> 5
    return np.asarray(ramp_table, dtype=np.int64)[np.minimum(idx, 511)]


def pack(y, dst_bits, dst_endian, flags=0, ramp=None, ramp_table=None):
    """S24 [frames, channels] -> the message's bytes: the 24-bit ramp case, depth, byte order, ZERO_LSB32."""
    frames, ch = y.shape
    w = (y.astype(np.int64) << 8) & MASK32                          # left-justified word
    if flags & FLAG_RAMP:
        mult = ramp_multipliers(ramp_table, ramp[0], ramp[1], frames)[:, None]
        s16 = ((w >> 16) & 0xFFFF).astype(np.int64)
        s16 = np.where(s16 >= 1 << 15, s16 - (1 << 16), s16)
        w = (((s16 * mult) >> 15) & 0xFFFF) << 16
    db = dst_bits // 8
    if (flags & FLAG_ZERO_LSB32) and db == 4:
        w &= 0xFFFFFF00
    out = np.zeros((frames, ch, db), dtype=np.uint8)
    for b in range(db):
        out[:, :, b] = (w >> (24 - 8 * b)) & 0xFF
    if dst_endian == ENDIAN_LITTLE:
        out = out[:, :, ::-1]
    return out.reshape(-1)


def message_bytes(table, phases_log2, desc, src_arena, ramp_table=None):
    """What ohgpu_src_pull_batch_run writes for one ohgpu_src_pull_msg_desc (numpy record) reading `src_arena`."""
    d = {k: int(desc[k]) for k in ("src_offset", "src_frame0", "src_frames", "pos_frame", "step", "pos_frac", "n_frames",
                                   "ramp_start", "ramp_end", "channels", "src_bits", "src_endian", "dst_bits", "dst_endian", "flags")}
    ch, sb = d["channels"], d["src_bits"] // 8
    raw = src_arena[d["src_offset"]:d["src_offset"] + d["src_frames"] * ch * sb]
    x = decode_s24(raw, ch, d["src_bits"], d["src_endian"]) if d["src_frames"] else np.zeros((0, ch), dtype=np.int64)
    y = resample(table, phases_log2, x, d["src_frame0"], d["pos_frame"], d["pos_frac"], d["step"], d["n_frames"])
    return pack(y, d["dst_bits"], d["dst_endian"], d["flags"], (d["ramp_start"], d["ramp_end"]), ramp_table)
