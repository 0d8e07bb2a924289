"""FlywheelRamper on plain Python integers: decimation by sample-and-hold, Burg's method of degree 3 on 16-bit
data, the coefficient-overflow correction, and the 3-state feedback filter that generates the ramp.

Written from the operation's definition, NOT from oracle/ohp_flywheel.c or flywheel_kernel.hip: no ctypes, no import of oracle_lib.
Every place where the reference's C types narrow a value is an explicit wrap16 / wrap32 here, and Python's unbounded integers
carry everything in between, so a forgotten or misplaced wrap shows as a different number instead of hiding in a C type.

One request = `channels` planes of big-endian 32-bit training samples (oldest first; only the newest `in_samples` of each plane are
used), a sample rate (which fixes the decimation factor), and `out_frames` frames to generate in blocks of at most `block_frames`.

The one undefined spot: Burg's reflection coefficient is (sn << 13) / sd in 64 bits.  sd is a sum of squares kept in 32 bits, so
it can wrap to exactly 0 while sn != 0; the reference then divides by zero.  The model raises UndefinedDivision there and no test
input may reach it (tests/test_flywheel_textbook.py asserts that for every input the GPU tests use).
"""

DEGREE = 3
MAX_CHANNELS = 10
BURG_DATA_DESCALE_BITS = 1            # the training data are halved before Burg's method
BURG_OUTPUT_FORMAT = 3                # coefficients are 3.13 fixed point
BURG_SCALE_SHIFT = 16 - BURG_OUTPUT_FORMAT
FEEDBACK_DATA_DESCALE_BITS = 0
FEEDBACK_DATA_FORMAT = 1
FEEDBACK_OUTPUT_FORMAT = 1


class UndefinedDivision(ArithmeticError):
    pass


def wrap16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def wrap32(v):
    v &= 0xFFFFFFFF
    return v - 0x100000000 if v & 0x80000000 else v


def wrap64(v):
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v & (1 << 63) else v


def trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def decimation_factor(sample_rate):
    if sample_rate in (176400, 192000):
        return 4
    if sample_rate in (88200, 96000):
        return 2
    return 1


def burgs_method(samples, degree=DEGREE):
    """samples: signed 16-bit values.  Returns the `degree` prediction coefficients (3.13, signed 16-bit)."""
    count = len(samples)
    per = [0] * count                       # backward prediction error, 16-bit
    pef = [0] * count                       # forward prediction error, 16-bit
    out = [0] * degree
    h = [0] * degree
    limit1 = count - 1
    limit2 = limit1
    for n in range(degree):
        sn = 0
        sd = 0
        for j in range(limit1):
            t1 = wrap16(samples[j + n + 1] + pef[j])
            t2 = wrap16(samples[j] + per[j])
            sn = wrap32(sn - wrap32(2 * wrap32(t1 * t2)))
            sd = wrap32(sd + wrap32(wrap32(t1 * t1) + wrap32(t2 * t2)))
        limit1 -= 1
        t3 = 0
        if sn != 0:
            if sd == 0:
                raise UndefinedDivision("Burg's method: sn = %d over sd = 0 at order %d" % (sn, n))
            t3 = wrap16(trunc_div(wrap64(sn << BURG_SCALE_SHIFT), sd))
        out[n] = t3
        if n > 0:
            for j in range(n):
                product = wrap32(t3 * out[n - j - 1])
                h[j] = wrap16(product >> BURG_SCALE_SHIFT)
                h[j] = wrap16(h[j] + out[j])
            for j in range(n):
                out[j] = h[j]
            limit2 -= 1
        if n == degree - 1:
            break
        for j in range(limit2):
            i = j + 1
            p = wrap32(wrap32(pef[j] + samples[i + n]) * t3)
            per[j] = wrap16(per[j] + wrap16(p >> BURG_SCALE_SHIFT))
            f = wrap32(wrap32(per[i] + samples[i]) * t3)
            pef[j] = wrap16(f >> BURG_SCALE_SHIFT)
            pef[j] = wrap16(pef[j] + pef[i])
    return out


def coeff_overflow(coeffs, fmt=BURG_OUTPUT_FORMAT):
    """How far the coefficients' 16-bit sum lies outside [-1.0, +1.0] in `fmt`.(16 - fmt) fixed point (0: inside)."""
    one = wrap16(1 << (16 - fmt))
    total = 0
    for c in coeffs:
        total = wrap16(total + c)
    if -one <= total <= one:
        return 0
    if total & 0x8000:
        return wrap16(total + one)
    return wrap16(total - one)


class FeedbackModel:
    """y[n] = sum_j high32(state[j] * coeff[j]) << coeff_format, the newest output first in `state`."""

    def __init__(self, state_count, data_descale_bits, coeff_format, data_format, output_format, coeffs, samples):
        assert len(coeffs) == state_count and len(samples) == state_count
        self.coeffs = [wrap32(c) for c in coeffs]
        self.samples = [wrap32(s) >> data_descale_bits for s in samples]
        self.coeff_format = coeff_format
        self.scale_shift_for_output = data_format + data_descale_bits - output_format

    def next_sample(self):
        total = 0
        for s, c in zip(self.samples, self.coeffs):
            total = wrap32(total + wrap32((s * c) >> 32))
        for j in range(len(self.samples) - 1, 0, -1):
            self.samples[j] = self.samples[j - 1]
        total = wrap32(total << self.coeff_format)
        self.samples[0] = total
        if self.scale_shift_for_output < 0:
            total >>= -self.scale_shift_for_output
        else:
            total = wrap32(total << self.scale_shift_for_output)
        return total


def channel_model(plane, in_samples, sample_rate):
    """The feedback filter of one channel after training.  plane: the channel's training bytes (4 per sample, big-endian)."""
    assert in_samples * 4 <= len(plane)
    dec = decimation_factor(sample_rate)
    count = in_samples // dec
    assert count >= DEGREE + 1
    newest = plane[len(plane) - in_samples * 4:]           # the oldest audio is skipped
    training, states = [], [0] * DEGREE
    for i in range(count):
        at = 4 * dec * i
        s32 = int.from_bytes(bytes(newest[at:at + 4]), "big", signed=True)
        s16 = s32 >> 16
        if i >= count - DEGREE:
            states[count - i - 1] = s32                      # the filter starts from the last samples, newest first
        training.append(s16 >> BURG_DATA_DESCALE_BITS)
    burg = burgs_method(training, DEGREE)
    excess = coeff_overflow(burg, BURG_OUTPUT_FORMAT)
    if excess != 0:
        burg[0] = wrap16(burg[0] - wrap32(excess * 2))
    coeffs = [wrap32(-wrap32(c << 16)) for c in burg]
    return FeedbackModel(DEGREE, FEEDBACK_DATA_DESCALE_BITS, BURG_OUTPUT_FORMAT, FEEDBACK_DATA_FORMAT, FEEDBACK_OUTPUT_FORMAT,
                         coeffs, states)


def flywheel_ramp(training, channel_bytes, in_samples, sample_rate, channels, out_frames, block_frames):
    """The generated ramp: out_frames frames of `channels` big-endian 32-bit subsamples, interleaved.  training: `channels` planes of
    channel_bytes bytes each."""
    assert 1 <= channels <= MAX_CHANNELS and block_frames > 0
    dec = decimation_factor(sample_rate)
    models = [channel_model(training[c * channel_bytes:(c + 1) * channel_bytes], in_samples, sample_rate) for c in range(channels)]
    out = bytearray()
    remaining = out_frames
    held = [0] * channels
    while remaining > 0:
        n = min(remaining, block_frames)
        remaining -= n
        hold = 0                                             # the hold counter restarts with every block
        for _ in range(n):
            for c in range(channels):
                if hold == 0:
                    held[c] = models[c].next_sample()
                out += (held[c] & 0xFFFFFFFF).to_bytes(4, "big")
            hold += 1
            if hold == dec:
                hold = 0
    return bytes(out)
