"""The fixed-ratio resampler as the textbook states it, in numpy alone: the checker the resampler's kernels are held to.

    u[i] = x[i / L] where L divides i, else 0            (zero-stuff by L; input frames before frame 0 are zeros)
    y[m] = sum_j h[j] * u[m*M - j]                       (the prototype h at the upsampled rate, every M-th output kept)
    out[m] = clamp((y[m] + 2^27) >> 28, -2^23, 2^23 - 1) (Q28 -> S24: round half up, then clamp)

with the prototype h[p + k*L] = coef_q28[p*T + k].  The stuffed zeros contribute nothing, so the sum is evaluated over the
samples that are not: y[m] = sum_n h[m*M - n*L] * x[n] for the input frames n with 0 <= m*M - n*L < L*T -- one row of a banded
matrix per output, indexed by the prototype position m*M - n*L (no phase, no tap order, no n0).  The coefficient table is an
input; nothing here comes from the library or the oracle.  Decode, the 24-bit ramp and the pack are src_pull_model's
restatements; tests/test_src_textbook.py holds all of it to the oracle byte for byte, and to scipy's upfirdn where that exists.

The second half builds the inputs the tests feed it: rounding ties, the golden fixture's inputs, the source layouts' bytes.
"""
import numpy as np

import src_pull_model as PM

S24_MIN, S24_MAX = -(1 << 23), (1 << 23) - 1
FLAG_RAMP, FLAG_ZERO_LSB32, FLAG_SRC_PLANAR32 = 1, 4, 8
ENDIAN_LITTLE, ENDIAN_BIG = PM.ENDIAN_LITTLE, PM.ENDIAN_BIG
UNITY_ATTENUATION = 256
_EXACT = 1 << 53


def prototype(coef_q28, L, T):
    """The polyphase table back into one FIR at the upsampled rate: h[p + k*L] = coef_q28[p*T + k] (length L*T)."""
    c = np.asarray(coef_q28, dtype=np.int64).reshape(L, T)
    return np.ascontiguousarray(c.T).reshape(-1)


def out_frames(L, M, in_frames):
    """Outputs whose newest input frame has arrived once in_frames have: m with floor(m*M / L) <= in_frames - 1."""
    return (in_frames * L + M - 1) // M


def round_s24(acc):
    """Q28 sums -> S24: floor(acc / 2^28 + 1/2), clamped to [-2^23, 2^23 - 1]."""
    return np.clip((np.asarray(acc, dtype=np.int64) + (1 << 27)) >> 28, S24_MIN, S24_MAX)


def frames_read(h_len, up, t):
    """(oldest, newest) input frame that the sums at upsampled positions t reach (the oldest clipped at frame 0)."""
    t = np.asarray(t, dtype=np.int64)
    return max(-((h_len - 1 - int(t.min())) // up), 0), int(t.max()) // up


def filter_at(h, up, x, x_first, t):
    """Exact sums y(t) = sum_n h[t - n*up] * x[n] at upsampled positions t (int64 [K]) -> int64 [K, channels].  x: int64
    [frames, channels] holding input frames x_first ..; frames before 0 are zeros; every other frame a sum reaches must be in x."""
    h = np.asarray(h, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    ch = x.shape[1]
    if t.size == 0:
        return np.zeros((0, ch), dtype=np.int64)
    n_lo, n_hi = frames_read(h.size, up, t)
    n = np.arange(n_lo, n_hi + 1, dtype=np.int64)
    j = t[:, None] - n[None, :] * up                                      # the prototype position of (output, frame)
    inside = (j >= 0) & (j < h.size)
    H = np.where(inside, h[np.clip(j, 0, h.size - 1)], 0)                 # [K, frames]
    rel = n - x_first
    have = (rel >= 0) & (rel < x.shape[0])
    assert np.all(have[inside.any(axis=0)]), "the buffer does not hold every frame the outputs read"
    xs = np.zeros((n.size, ch), dtype=np.int64)
    xs[have] = x[rel[have]]
    bound = int(np.abs(H).sum(axis=1).max()) * int(np.abs(xs).max(initial=0))
    if bound < _EXACT:                                                    # every partial sum an integer below 2^53: fp64 is exact
        return (H.astype(np.float64) @ xs.astype(np.float64)).astype(np.int64)
    return H @ xs


def resample(coef_q28, L, M, T, x, x_first, m0, n_out):
    """S24 outputs m0 .. m0 + n_out - 1 ([n_out, channels]) of the L/M resampler whose table is coef_q28."""
    t = (np.int64(m0) + np.arange(n_out, dtype=np.int64)) * M
    return round_s24(filter_at(prototype(coef_q28, L, T), L, x, x_first, t))


def pulled_prototype(table, phases_log2):
    """The pulled path's table as one FIR at 2^s times the input rate: h[p + k * 2^s] = table[p][k] for p < 2^s."""
    C = np.asarray(table, dtype=np.int64)
    return np.ascontiguousarray(C[:1 << phases_log2].T).reshape(-1)


def resample_pulled(table, phases_log2, x, x_first, pos_frame, pos_frac, step, n_out):
    """The pulled path's phase-aligned case (step = a * 2^(32 - s), pos_frac a multiple of 2^(32 - s), so that the interpolation
    weight is 0) as the same operation: up = 2^s, down = a, outputs at the upsampled positions
    pos_frame * 2^s + pos_frac / 2^(32 - s) + j * a."""
    s = phases_log2
    unit = 1 << (32 - s)
    assert step % unit == 0 and pos_frac % unit == 0, "not phase-aligned"
    t = (pos_frame << s) + pos_frac // unit + np.arange(n_out, dtype=np.int64) * (step // unit)
    return round_s24(filter_at(pulled_prototype(table, s), 1 << s, x, x_first, t))


def decode(src_arena, d):
    """The message's buffer (frames src_frame0 .. + src_frames) as int64 [frames, channels] S24."""
    ch, bits, frames = int(d["channels"]), int(d["src_bits"]), int(d["src_frames"])
    off = int(d["src_offset"])
    arena = np.asarray(src_arena, dtype=np.uint8)
    if frames == 0:
        return np.zeros((0, ch), dtype=np.int64)
    if int(d["flags"]) & FLAG_SRC_PLANAR32:                               # one plane of LE int32 per channel, values at `bits` depth
        assert bits <= 24
        stride = int(d["src_plane_stride"])
        planes = [arena[off + c * stride:off + c * stride + 4 * frames].view("<i4").astype(np.int64) for c in range(ch)]
        return np.stack(planes, axis=1) << (24 - bits)
    return PM.decode_s24(arena[off:off + frames * ch * bits // 8], ch, bits, int(d["src_endian"]))


def message_s24(coef_q28, L, M, T, d, src_arena):
    """S24 [n_frames, channels] of one ohgpu_src_msg_desc (numpy record), before ramp and pack."""
    assert int(d["attenuation"]) == UNITY_ATTENUATION
    return resample(coef_q28, L, M, T, decode(src_arena, d), int(d["src_frame0"]), int(d["out_frame0"]), int(d["n_frames"]))


def pack(y, d, ramp_table):
    """S24 [n_frames, channels] -> the bytes of the message d (its ramp, depth, byte order and ZERO_LSB32)."""
    return PM.pack(y, int(d["dst_bits"]), int(d["dst_endian"]), int(d["flags"]) & (FLAG_RAMP | FLAG_ZERO_LSB32),
                   (int(d["ramp_start"]), int(d["ramp_end"])), ramp_table)


def message_bytes(coef_q28, L, M, T, d, src_arena, ramp_table):
    """The bytes one ohgpu_src_msg_desc asks for: resample, RampApplicator's 24-bit case, depth, byte order, ZERO_LSB32."""
    return pack(message_s24(coef_q28, L, M, T, d, src_arena), d, ramp_table)


def batch_bytes(coef_q28, L, M, T, descs, src_arena, dst_bytes, ramp_table, fill=0xA5):
    """A batch's whole destination arena: every message's bytes, `fill` wherever no message writes."""
    out = np.full(dst_bytes, fill, dtype=np.uint8)
    for d in descs:
        b = message_bytes(coef_q28, L, M, T, d, src_arena, ramp_table)
        out[int(d["dst_offset"]):int(d["dst_offset"]) + b.size] = b
    return out


def impulse_response(coef_q28, L, M, T, amplitude, n, m):
    """What a lone impulse `amplitude` at input frame n gives at outputs m: round(amplitude * h[m*M - n*L] / 2^28) where that
    position is inside the prototype, 0 elsewhere -- read straight from the table."""
    h = prototype(coef_q28, L, T)
    j = np.asarray(m, dtype=np.int64) * M - n * L
    inside = (j >= 0) & (j < h.size)
    return np.where(inside, round_s24(amplitude * h[np.clip(j, 0, h.size - 1)]), 0)


# ------------------------------------------------------------------------------------------ inputs
def source_shift(bits):
    """A source sample of `bits` bits sits this many bits left in its S24 value (a 32-bit one: its top 24 bits are the value)."""
    return 24 - min(bits, 24)


def tie_gap(L, M, T):
    """Outputs between planted ties so that their windows (T input frames each) share no frame."""
    return -(-(T + 1) * L // M) + 1


def plant_tie(rng, h, up, down, m, y, col, bits, offset=0, big=False):
    """Make output m of channel `col` a rounding tie: its window's exact sum == 2^27 + offset (mod 2^28) -- offset 0 for a tie,
    +/- 2^source_shift(bits) (one source step) beside one.  y: int64 [frames, channels] of source-unit samples (S24 = y <<
    source_shift(bits)) whose frames in the window are rewritten; big: the other samples at full scale with their coefficients'
    signs, so that the sum lies far past the clamp.  Returns the exact sum, or None for a window without an odd coefficient."""
    sh = source_shift(bits)
    mod = 1 << (28 - sh)
    lim = 1 << (min(bits, 24) - 1)
    assert offset % (1 << sh) == 0
    t = m * down
    n_lo, n_hi = frames_read(len(h), up, [t])
    assert n_hi < y.shape[0]
    n = np.arange(n_lo, n_hi + 1)
    c = np.asarray(h, dtype=np.int64)[t - n * up]
    odd = np.nonzero(c & 1)[0]
    if odd.size == 0:
        return None
    target = ((1 << 27) + offset) >> sh
    for _ in range(2000):
        k = int(rng.choice(odd))
        if big:
            sign = 1 if rng.random() < 0.5 else -1
            v = np.where(c * sign >= 0, lim - 1, -lim) - np.sign(c * sign) * rng.integers(0, 16, size=n.size)
        else:
            v = rng.integers(-lim, lim, size=n.size)
        v = v.astype(np.int64)
        v[k] = 0
        rest = int(np.dot(c, v))
        vk = ((target - rest) * pow(int(c[k]) % mod, -1, mod)) % mod
        if vk >= mod // 2:
            vk -= mod
        if -lim <= vk < lim:
            v[k] = vk
            y[n, col] = v
            acc = int(np.dot(c, v)) << sh
            assert (acc - (1 << 27) - offset) % (1 << 28) == 0
            return acc
    raise AssertionError("no tie within reach")


def plant_ties(rng, coef_q28, L, M, T, y, bits, first_frame=0):
    """Ties in every channel at every tie_gap-th output whose window starts at or after first_frame and ends inside y: most exact,
    one in three one source step above or below; every fifth far past the clamp.  Returns {(output, channel): (exact sum, offset)}."""
    h = prototype(coef_q28, L, T)
    step = 1 << source_shift(bits)
    m = -(-(first_frame * L + h.size - 1) // M)
    ties, i = {}, 0
    while (m * M) // L < y.shape[0]:
        for col in range(y.shape[1]):
            offset = (0, 0, step, 0, 0, -step)[i % 6]
            acc = plant_tie(rng, h, L, M, m, y, col, bits, offset, big=(i % 5 == 4))
            if acc is not None:
                ties[(m, col)] = (acc, offset)
            i += 1
        m += tie_gap(L, M, T)
    return ties


FIXTURE_INPUTS = ("noise", "impulses_and_ties")
FIXTURE_FRAMES = 6144                 # (48 -> 44.1 kHz: more than one of round 1's 4704-output blocks)


def fixture_input(kind, coef_q28, L, M, T, frames=FIXTURE_FRAMES):
    """The golden fixture's two stereo S24 inputs (tests/golden/src_textbook.json), from their seeds: full-scale noise; or
    full-scale impulses of both signs at a different frame in each channel, then rounding ties planted up to the end."""
    if kind == "noise":
        return np.random.default_rng(20261016).integers(S24_MIN, S24_MAX + 1, size=(frames, 2))
    assert kind == "impulses_and_ties"
    y = np.zeros((frames, 2), dtype=np.int64)
    y[0, 0], y[3, 1] = S24_MAX, S24_MIN
    y[T // 2, 0], y[T // 2 + 5, 1] = S24_MIN, S24_MAX
    plant_ties(np.random.default_rng(1016), coef_q28, L, M, T, y, 24, first_frame=2 * T)
    return y


def encode(y, bits, endian, rng=None, planar_stride=None):
    """Source-unit samples y (int64 [frames, channels]) as a layout's bytes: packed interleaved at `bits` and `endian` (32-bit: the
    value in the top 24 bits, a random low byte), or -- planar_stride given -- one LE int32 plane per channel, planes
    planar_stride bytes apart."""
    frames, ch = y.shape
    if planar_stride is not None:
        out = np.zeros(ch * planar_stride, dtype=np.uint8)
        for c in range(ch):
            out[c * planar_stride:c * planar_stride + 4 * frames] = y[:, c].astype("<i4").view(np.uint8)
        return out
    w = (y.astype(np.int64) << 8) if bits == 32 else (y.astype(np.int64) << (32 - bits))
    if bits == 32 and rng is not None:
        w |= rng.integers(0, 256, size=w.shape)
    w &= 0xFFFFFFFF
    sb = bits // 8
    out = np.zeros((frames, ch, sb), dtype=np.uint8)
    for b in range(sb):
        out[:, :, b] = (w >> (24 - 8 * b)) & 0xFF
    if endian == ENDIAN_LITTLE:
        out = out[:, :, ::-1]
    return out.reshape(-1)
