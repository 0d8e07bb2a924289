"""DSD -> PCM (include/ohgpu.h) as a textbook would do it, on numpy: a whole-signal convolution, then every D-th value.

Written from the specification, NOT from ohpipeline_amd/csrc/dsd_pcm_core.h (which walks one output's taps bit by bit) or
dsd_pcm_kernel.hip (byte-indexed partial sums): no per-output loop, no tables, no window arithmetic beyond which bits to take.

  1. UNPACK   the chunks [P/2 x 00] L L [P/2 x 00] R R into one bit row per channel, most significant bit of the first byte first.
  2. MAP      bit -> 2 * bit - 1.
  3. PREPEND  bit n < 0 is [0,1,1,0,1,0,0,1][n mod 8] (non-negative modulo): the silence byte 0x69 repeating, aligned at n = 0.
  4. CONVOLVE np.convolve in int64 with coef[0 .. N): full[p] = sum_k coef[k] * s[p - k].
  5. DECIMATE output frame m is the value whose newest sample is bit (m + 1) * D - 1.
  6. ROUND    y = clamp(-2^23, 2^23 - 1, (acc + 16) >> 5).
  7. RAMP     through tests/pcm_textbook.py's functions at 24 bits, frame i of the message's n_frames.
  8. PACK     three bytes, interleaved L R, big-endian unless dst_endian says little.

The design (ohgpu_dsd_pcm_design) is restated in `design`: plain Python floats, the formula as DESIGN.md 4c gives it."""
import math

import numpy as np

import pcm_textbook as PT

IDLE = (0, 1, 1, 0, 1, 0, 0, 1)
DECIMATIONS = (8, 16, 32, 64)
ENDIAN_LITTLE, ENDIAN_BIG = 1, 2
FLAG_RAMP = 1


# ---------------------------------------------------------------- the design
def _i0(x):
    total, term, q = 1.0, 1.0, x * x * 0.25
    for k in range(1, 500):
        term *= q / (float(k) * float(k))
        total += term
        if term < total * 1e-20:
            break
    return total


def design(dsd_rate, pcm_rate, T, beta, f_pass, gain):
    """coef_q28[D * T]: a Kaiser-windowed sinc of odd length D * T - 1 centred on a tap, cutoff midway between f_pass and
    pcm_rate - f_pass, scaled to sum = gain, times 2^28 rounded half up; the last stored coefficient is zero."""
    assert dsd_rate % pcm_rate == 0
    D = dsd_rate // pcm_rate
    assert D in DECIMATIONS and T % 8 == 0 and 8 <= T <= 64
    n_taps = D * T - 1
    fc = 0.5 * (f_pass + (float(pcm_rate) - f_pass))
    wc = 2.0 * fc / float(dsd_rate)
    centre = 0.5 * float(n_taps - 1)
    i0b = _i0(beta)
    h, total = [], 0.0
    for n in range(n_taps):
        d = float(n) - centre
        x = wc * d
        sinc = 1.0 if abs(x) < 1e-12 else math.sin(math.pi * x) / (math.pi * x)
        r = d / centre
        arg = 1.0 - r * r
        w = _i0(beta * math.sqrt(arg if arg > 0.0 else 0.0)) / i0b
        h.append(wc * sinc * w)
        total += h[-1]
    scale = gain / total
    coef = [int(math.floor(v * scale * 268435456.0 + 0.5)) for v in h] + [0]
    return D, np.array(coef, dtype=np.int64)


def bound_ok(coef):
    return int(np.abs(np.asarray(coef, dtype=np.int64)).sum()) < (1 << 30)


# ---------------------------------------------------------------- the signal
def window(out_frame0, n_frames, D, T):
    """[chunk_lo, chunk_hi): the chunks whose bits of index >= 0 output frames [out_frame0, + n_frames) meet."""
    oldest, newest = (out_frame0 + 1) * D - D * T, (out_frame0 + n_frames) * D - 1
    return max(oldest, 0) // 16, newest // 16 + 1


def unpack(chunk_bytes, P):
    """(2, 16 * chunks) bits of a run of chunks in the pipeline's DSD format."""
    a = np.frombuffer(bytes(chunk_bytes), dtype=np.uint8).reshape(-1, 4 + P)
    left, right = a[:, P // 2:P // 2 + 2], a[:, P + 2:P + 4]
    return np.stack([np.unpackbits(left.reshape(-1)), np.unpackbits(right.reshape(-1))])


def pack_chunks(bits, P):
    """The inverse: (2, 16 * chunks) bits -> the format's bytes."""
    chunks = bits.shape[1] // 16
    out = np.zeros((chunks, 4 + P), dtype=np.uint8)
    out[:, P // 2:P // 2 + 2] = np.packbits(bits[0]).reshape(chunks, 2)
    out[:, P + 2:P + 4] = np.packbits(bits[1]).reshape(chunks, 2)
    return out.tobytes()


def frames(coef, D, bits, bit0, out_frame0, n_frames):
    """S24 values (n_frames, 2) of output frames [out_frame0, + n_frames); bits[:, i] is the stream's bit bit0 + i."""
    coef = np.asarray(coef, dtype=np.int64)
    N = coef.size
    index = np.arange((out_frame0 + 1) * D - N, (out_frame0 + n_frames) * D, dtype=np.int64)
    idle = np.array(IDLE, dtype=np.int64)[index % 8]
    held = np.clip(index - bit0, 0, bits.shape[1] - 1)
    assert ((index < 0) | ((index >= bit0) & (index - bit0 < bits.shape[1]))).all(), "the message reads a bit its window does not hold"
    out = np.zeros((n_frames, 2), dtype=np.int64)
    for c in range(2):
        samples = 2 * np.where(index < 0, idle, bits[c][held].astype(np.int64)) - 1
        acc = np.convolve(samples, coef)[N - 1:N - 1 + n_frames * D:D]
        out[:, c] = np.clip((acc + 16) >> 5, -(1 << 23), (1 << 23) - 1)
    return out


def message_bytes(d, coef, D, src):
    """The destination bytes of one message (a record of capi.DSD_PCM_MSG_DESC's fields); src: the source arena."""
    n, P = int(d["n_frames"]), int(d["pad_bytes_per_chunk"])
    if n == 0:
        return b""
    so, c0, held = int(d["src_offset"]), int(d["src_chunk0"]), int(d["src_chunks"])
    raw = bytes(src[so:so + held * (4 + P)])
    assert len(raw) == held * (4 + P), "the window leaves the arena"
    y = frames(coef, D, unpack(raw, P), 16 * c0, int(d["out_frame0"]), n)
    ramped, table = bool(int(d["flags"]) & FLAG_RAMP), PT.ramp_table()
    out = bytearray()
    for i in range(n):
        if ramped:
            mult = table[PT.ramp_index(PT.ramp_value(i, n, int(d["ramp_start"]), int(d["ramp_end"])))]
        for c in range(2):
            v = int(y[i, c]) << 8
            if ramped:
                v = PT.ramp_subsample(v, 24, 2, c, mult)
            out += PT.write_subsample(v, 24, int(d["dst_endian"]), False)
    return bytes(out)


def batch_bytes(descs, coef, D, src, dst_bytes, fill):
    dst = np.full(dst_bytes, fill, dtype=np.uint8)
    for d in descs:
        out = np.frombuffer(message_bytes(d, coef, D, src), dtype=np.uint8)
        off = int(d["dst_offset"])
        assert off + out.size <= dst_bytes or out.size == 0, "the message writes beyond its arena"
        dst[off:off + out.size] = out
    return dst


def totals(descs, D, T):
    """ohgpu_batch_info of a batch: messages, chunks read, frames out, source bytes read, destination bytes written."""
    chunks = src = frames_out = 0
    for d in descs:
        if int(d["n_frames"]):
            lo, hi = window(int(d["out_frame0"]), int(d["n_frames"]), D, T)
            chunks += hi - lo
            src += (hi - lo) * (4 + int(d["pad_bytes_per_chunk"]))
            frames_out += int(d["n_frames"])
    return {"n_msgs": len(descs), "in_frames": chunks, "out_frames": frames_out, "src_bytes_touched": src, "dst_bytes_written": 6 * frames_out}
