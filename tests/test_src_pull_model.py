"""CPU checks of the pulled resampler's specification through its numpy model: the split identity, windows against
the whole stream, the interpolation's end points, and an independent float64 evaluation of the continuous windowed sinc."""
import numpy as np
import pytest

import src_pull_model as PM
from ohpipeline_amd import capi

S = 8
RATE_IN, RATE_OUT, F_PASS, BETA, MAX_PULL = 44100, 48000, 20000.0, 8.0, 0.001


@pytest.fixture(scope="module")
def table():
    return capi.src_pull_design(RATE_IN, RATE_OUT, 32, S, BETA, F_PASS, MAX_PULL)


def noise(seed, frames, ch=2):
    return np.random.default_rng(seed).integers(-(1 << 23), 1 << 23, size=(frames, ch), dtype=np.int64)


def test_split_identity_at_every_point(table):
    x = noise(1, 4000)
    step = PM.step_of(RATE_IN, RATE_OUT, PM.multiplier_of(317))
    pos, frac, n = 1234, (1 << 32) - 5, 97
    whole = PM.resample(table, S, x, 0, pos, frac, step, n)
    for k in range(1, n):
        p2, f2 = PM.advance(pos, frac, step, k)
        head = PM.resample(table, S, x, 0, pos, frac, step, k)
        tail = PM.resample(table, S, x, 0, p2, f2, step, n - k)
        assert np.array_equal(np.vstack([head, tail]), whole), k
        # ... and so are the bytes: the pack is per frame
        assert np.array_equal(np.concatenate([PM.pack(head, 24, PM.ENDIAN_BIG), PM.pack(tail, 24, PM.ENDIAN_BIG)]),
                              PM.pack(whole, 24, PM.ENDIAN_BIG))


def test_chunked_windows_equal_the_whole_stream(table):
    rng = np.random.default_rng(2)
    x = noise(3, 20000)
    pos, frac = 0, 0
    for _ in range(60):
        step = PM.step_of(RATE_IN, RATE_OUT, PM.multiplier_of(int(rng.integers(-1000, 1001))))
        n = int(rng.integers(1, 400))
        first, frames = PM.window(pos, frac, step, n, 32)
        got = PM.resample(table, S, x[first:first + frames], first, pos, frac, step, n)      # the message's window alone
        assert np.array_equal(got, PM.resample(table, S, x, 0, pos, frac, step, n))
        pos, frac = PM.advance(pos, frac, step, n)
    assert pos > 10000


def test_zero_weight_is_a_dot_product_with_row_p(table):
    C = table.astype(np.int64)
    x = noise(4, 3000)
    step = 233 << 24                                  # multiples of 2^(32 - s): every output lands on a phase, w = 0
    frac = 77 << 24
    y = PM.resample(table, S, x, 0, 100, frac, step, 200)
    for j in range(200):
        u = frac + j * step
        n, p = 100 + (u >> 32), (u & PM.MASK32) >> 24
        acc = C[p] @ x[n - np.arange(32)]
        assert np.array_equal(y[j], np.clip((acc + (1 << 27)) >> 28, -(1 << 23), (1 << 23) - 1))


def continuous_reference(x, pos_frame, pos_frac, step, n_frames, T=32, P=256):
    """Direct float64 evaluation of the design's continuous Kaiser-windowed sinc at each output's exact fractional position,
    normalised to DC gain 1 at that position -- independent of the table, the interpolation and the integer arithmetic."""
    f_stop = RATE_OUT - F_PASS
    fc = 0.5 * (F_PASS / (RATE_IN * (1 - MAX_PULL)) + f_stop / (RATE_IN * (1 + MAX_PULL)))
    wc, centre = 2.0 * fc / P, 0.5 * (T * P - 1)
    out = np.zeros((n_frames, x.shape[1]))
    k = np.arange(T)
    for j in range(n_frames):
        u = pos_frac + j * step
        n, phi = pos_frame + (u >> 32), (u & PM.MASK32) / 2.0 ** 32
        d = (k + phi) * P - centre
        r = np.clip(d / centre, -1.0, 1.0)
        h = wc * np.sinc(wc * d) * np.i0(BETA * np.sqrt(1.0 - r * r)) / np.i0(BETA)
        out[j] = (h / h.sum()) @ x[n - k].astype(np.float64)
    return np.clip(out, -(1 << 23), (1 << 23) - 1)                 # (full-scale noise overshoots: both saturate)


# |model - continuous| in S24 LSB: Q28 coefficients, the linear interpolation between 256 phases and the final rounding.  Measured
# (DESIGN.md 4b): noise 371 peak / 31 rms, the tone 330 / 11.5 -- at most -86 dB of full scale
REFERENCE_ERROR_LSB, REFERENCE_RMS_LSB = 400.0, 40.0


@pytest.mark.parametrize("signal", ["noise", "tone997"])
def test_independent_float64_evaluation(table, signal):
    frames = 6000
    if signal == "noise":
        x = noise(5, frames)
    else:
        t = np.arange(frames)
        x = np.round(0.891 * ((1 << 23) - 1) * np.sin(2 * np.pi * 997.0 * t / RATE_IN))[:, None].repeat(2, axis=1).astype(np.int64)
    step = PM.step_of(RATE_IN, RATE_OUT, PM.multiplier_of(-427))
    pos, frac, n = 40, 123456789, 5000
    got = PM.resample(table, S, x, 0, pos, frac, step, n)
    want = continuous_reference(x, pos, frac, step, n)
    err = np.abs(got - want)
    assert err.max() <= REFERENCE_ERROR_LSB, err.max()
    assert np.sqrt((err ** 2).mean()) <= REFERENCE_RMS_LSB
