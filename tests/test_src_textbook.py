"""The resampler's textbook model (tests/src_textbook.py) on the CPU: byte for byte the oracle's ohp_src_msg_process over designs,
formats, input classes and message shapes; scipy's upfirdn, a third party's implementation of the same operation; the impulse
identity read off the table; rounding ties on both signs and past the clamp; and the golden fixture that pins the numbers.

Every other bit-exactness test of the resampler compares with the oracle or src_pull_model, both written here, and the oracle
shares the kernels' polyphase indexing (n0 = m*M div L, the phase, the tap order, zeros before the stream).  The model indexes
the prototype directly, so a mistake made the same way in the oracle and the kernels shows up here."""
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import src_pull_model as PM
import src_textbook as TB
from ohpipeline_amd import capi

LE, BE = TB.ENDIAN_LITTLE, TB.ENDIAN_BIG
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "src_textbook.json")
GENERATOR = os.path.join(HERE, "golden", "make_src_textbook_fixtures.py")
RAMPS = [(16384, 0), (0, 16384), (16384, 8192), (8191, 8190), (5, 5), (16384, 16384), (0, 0), (12345, 54), (17, 16001)]
FORMATS = list(itertools.product([(b, e) for b in (8, 16, 24, 32) for e in (LE, BE)], [(b, e) for b in (8, 16, 24, 32) for e in (BE, LE)]))
CLASSES = ("noise", "rails", "impulses", "ties")
BETA, F_PASS = 9.0, 20000.0


def _accepted_designs():
    out = []
    for rin, rout, T in itertools.product([44100, 48000, 88200, 96000, 176400, 192000, 32000, 8000], [48000, 44100], [16, 24, 32, 64]):
        try:
            O.Src(rin, rout, T, BETA, F_PASS)
        except ValueError:
            continue
        out.append((rin, rout, T))
    return out


DESIGNS = _accepted_designs()


def full_scale(bits):
    return -(1 << (min(bits, 24) - 1)), (1 << (min(bits, 24) - 1)) - 1


def class_input(kind, rng, coef, L, M, T, n_in, ch, bits):
    """Source-unit samples [n_in, ch] of one input class (tests/test_gpu_src_textbook.py has the GPU's forms of them)."""
    lo, hi = full_scale(bits)
    if kind == "noise":
        return rng.integers(lo, hi + 1, size=(n_in, ch))
    if kind == "rails":                                           # DC at each rail, then a full-scale square wave in the pass band
        y = np.empty((n_in, ch), dtype=np.int64)
        third = n_in // 3
        up = np.arange(ch) % 2 == 0
        y[:third] = np.where(up, hi, lo)
        y[third:2 * third] = np.where(up, lo, hi)
        y[2 * third:] = np.where((np.arange(n_in - 2 * third) // 24) % 2 == 0, hi, lo)[:, None]
        return y
    if kind == "impulses":
        y = np.zeros((n_in, ch), dtype=np.int64)
        for i, n in enumerate(range(0, n_in, 3 * T + 7)):
            for c in range(ch):
                if n + 2 * c < n_in:
                    y[n + 2 * c, c] = hi if (i + c) % 2 == 0 else lo
        return y
    y = rng.integers(lo, hi + 1, size=(n_in, ch))
    ties = TB.plant_ties(rng, coef, L, M, T, y, bits)
    assert ties or not (TB.prototype(coef, L, T) & 1).any()     # (the identity's one coefficient, 2^28, makes no tie)
    return y


@pytest.mark.parametrize("rin,rout,T", DESIGNS, ids=[f"{a}to{b}_T{t}" for a, b, t in DESIGNS])
def test_model_equals_the_oracle(rin, rout, T):
    """Four streams per design -- one per input class, each in its own source and destination format and channel count, the
    formats rotating over the designs so that every pair of the 64 is met -- cut twice into messages of 1, 2, L-1, L, L+1, 239
    and 240 frames: the first pass from the stream's start with the whole stream as the buffer, the second with the tightest
    buffer each message allows (src_frame0 > 0); ramped / unramped, ZERO_LSB32 on some."""
    ref = O.Src(rin, rout, T, BETA, F_PASS)
    L, M, coef = ref.L, ref.M, ref.coef_q28
    k = DESIGNS.index((rin, rout, T))
    rng = np.random.default_rng(100 + k)
    sizes = [n for n in (1, 2, L - 1, L, L + 1, 239, 240) if n > 0] * 2
    n_in = (sum(sizes) - 1) * M // L + 1
    rows, parts, sp, dp = [], [], 0, 0
    for s, kind in enumerate(CLASSES):
        (sbits, se), (dbits, de) = FORMATS[(len(CLASSES) * k + s) % len(FORMATS)]
        ch = (k + s) % 8 + 1
        data = TB.encode(class_input(kind, rng, coef, L, M, T, n_in, ch, sbits), sbits, se, rng)
        fb = ch * sbits // 8
        m = 0
        for i, n in enumerate(sizes):
            f0, nf = 0, n_in
            if i >= len(sizes) // 2:
                f0 = max((m * M) // L - (T - 1), 0)
                nf = min(((m + n - 1) * M) // L - f0 + 1 + i % 3, n_in - f0)
            ramp = RAMPS[(k + i) % len(RAMPS)]
            flags = (O.FLAG_RAMP if (k + i) % 3 else 0) | (O.FLAG_ZERO_LSB32 if (k + i) % 4 == 0 else 0)
            rows.append((sp + f0 * fb, f0, nf, m, dp, n, ramp[0], ramp[1], 256, ch, sbits, se, dbits, de, flags, 0))
            dp += n * ch * dbits // 8
            m += n
        parts.append(data)
        sp += data.size
        dp += 3
    descs = np.array(rows, dtype=O.SRC_MSG_DESC)
    src = np.concatenate(parts)
    want = np.full(dp, 0xA5, dtype=np.uint8)
    assert ref.process_batch(descs, src, want) == 0
    got = TB.batch_bytes(coef, L, M, T, descs, src, dp, O.ramp_table())
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} of {dp} bytes differ, first at {bad[:8]}"


def test_the_oracle_matrix_meets_every_format():
    assert len(DESIGNS) * len(CLASSES) >= len(FORMATS) and len(DESIGNS) >= 40


def upfirdn_s24(signal, h, x, up, down, n_out):
    """scipy's upfirdn of every channel, then the stated output rule; its fp64 sums are exact where the caller asserted the bound."""
    y = np.stack([signal.upfirdn(np.asarray(h, dtype=np.float64), x[:, c].astype(np.float64), up=up, down=down) for c in range(x.shape[1])], axis=1)
    assert np.array_equal(y, np.rint(y))
    return TB.round_s24(y.astype(np.int64))[:n_out] if n_out is not None else TB.round_s24(y.astype(np.int64))


def noise_and_rails(seed, n_in):
    x = np.random.default_rng(seed).integers(TB.S24_MIN, TB.S24_MAX + 1, size=(n_in, 2))
    x[n_in // 5:2 * n_in // 5, 0] = TB.S24_MAX
    x[2 * n_in // 5:3 * n_in // 5, 0] = TB.S24_MIN
    x[n_in // 4:n_in // 2, 1] = np.where((np.arange(n_in // 2 - n_in // 4) // 20) % 2 == 0, TB.S24_MAX, TB.S24_MIN)
    return x


@pytest.mark.parametrize("rin,rout,T", [(44100, 48000, 32), (96000, 48000, 64), (48000, 44100, 32), (32000, 48000, 16),
                                        (88200, 48000, 24), (8000, 48000, 32), (192000, 48000, 64)])
def test_model_equals_upfirdn(rin, rout, T):
    signal = pytest.importorskip("scipy.signal")
    L, M, coef = capi.src_design(rin, rout, T, BETA, F_PASS)
    assert (int(np.abs(coef.astype(np.int64)).reshape(L, T).sum(axis=1).max()) << 23) < 1 << 53       # upfirdn's sums are exact
    x = noise_and_rails(rin + rout + T, 3000)
    n_out = TB.out_frames(L, M, x.shape[0])
    got = TB.resample(coef, L, M, T, x, 0, 0, n_out)
    assert np.array_equal(got, upfirdn_s24(signal, TB.prototype(coef, L, T), x, L, M, n_out))
    assert (got == TB.S24_MAX).sum() > 50 and (got == TB.S24_MIN).sum() > 50


PULLED = [(8, 32, 256), (8, 32, 235), (8, 64, 279), (8, 64, 512), (6, 32, 64), (6, 64, 59), (6, 32, 128)]


def pulled_case(s, T, a, n_in=3000, n=700):
    table = capi.src_pull_design(44100, 48000, T, s, 8.0 if T == 32 else 9.0, F_PASS, 0.001)
    P = 1 << s
    assert (int(np.abs(table.astype(np.int64)).sum(axis=1).max()) << 23) < 1 << 53
    x = noise_and_rails(s * 1000 + T + a, n_in)
    m0 = 2 * T * P // a + 3                                     # (positions past T frames in: the first windows are whole)
    t0 = m0 * a
    return table, x, m0, t0 // P, (t0 % P) << (32 - s), a << (32 - s), n


@pytest.mark.parametrize("s,T,a", PULLED)
def test_pulled_model_at_phase_aligned_steps_is_the_same_operation(s, T, a):
    """The pulled path's model (src_pull_model) at steps and positions on the phase grid equals the fixed-ratio model's operation
    with up = 2^s, down = a on the pulled table's prototype."""
    table, x, m0, pos, frac, step, n = pulled_case(s, T, a)
    got = PM.resample(table, s, x, 0, pos, frac, step, n)
    assert np.array_equal(got, TB.resample_pulled(table, s, x, 0, pos, frac, step, n))
    assert (got == TB.S24_MAX).any() and (got == TB.S24_MIN).any()


@pytest.mark.parametrize("s,T,a", PULLED)
def test_pulled_model_equals_upfirdn(s, T, a):
    signal = pytest.importorskip("scipy.signal")
    table, x, m0, pos, frac, step, n = pulled_case(s, T, a)
    want = upfirdn_s24(signal, TB.pulled_prototype(table, s), x, 1 << s, a, None)[m0:m0 + n]
    assert want.shape[0] == n
    assert np.array_equal(TB.resample_pulled(table, s, x, 0, pos, frac, step, n), want)


@pytest.mark.parametrize("rin,rout,T", [(44100, 48000, 32), (96000, 48000, 64), (48000, 44100, 32), (32000, 48000, 16), (8000, 48000, 32)])
def test_impulse_identity(rin, rout, T):
    """A full-scale impulse A at input frame n: y[m] = clamp(round_half_up(A * h[m*M - n*L] / 2^28)) where 0 <= m*M - n*L < L*T,
    0 elsewhere -- in the model and in the oracle (one mono S24 message of the whole stream)."""
    ref = O.Src(rin, rout, T, BETA, F_PASS)
    L, M, coef = ref.L, ref.M, ref.coef_q28
    n_in = 6 * T + 40
    n_out = TB.out_frames(L, M, n_in)
    m = np.arange(n_out)
    for A, n in itertools.product((TB.S24_MAX, TB.S24_MIN), (0, 1, T - 1, T, 3 * T + 5)):
        x = np.zeros((n_in, 1), dtype=np.int64)
        x[n, 0] = A
        want = TB.impulse_response(coef, L, M, T, A, n, m)
        assert np.array_equal(TB.resample(coef, L, M, T, x, 0, 0, n_out)[:, 0], want), (A, n)
        d = np.array([(0, 0, n_in, 0, 0, n_out, 16384, 16384, 256, 1, 24, BE, 24, BE, 0, 0)], dtype=O.SRC_MSG_DESC)
        dst = np.zeros(n_out * 3, dtype=np.uint8)
        assert ref.process_batch(d, TB.encode(x, 24, BE), dst) == 0
        assert np.array_equal(PM.decode_s24(dst, 1, 24, BE)[:, 0], want), (A, n)
        assert np.abs(want).max() > (1 << 21)


@pytest.mark.parametrize("rin,rout,T", [(44100, 48000, 32), (48000, 44100, 32), (96000, 48000, 64)])
def test_ties_round_up_on_both_signs(rin, rout, T):
    """Windows whose exact sum lies half an LSB between two outputs, built for every phase (solved modulo 2^28 through an odd
    coefficient), on both signs and past the clamp, and windows one unit either side of a tie: the model and the oracle round
    every tie up and the neighbours to the nearer output."""
    ref = O.Src(rin, rout, T, BETA, F_PASS)
    L, M, coef = ref.L, ref.M, ref.coef_q28
    h = TB.prototype(coef, L, T)
    rng = np.random.default_rng(rin + T)
    gap = TB.tie_gap(L, M, T)
    inv_M = pow(M, -1, L) if L > 1 else 0
    phases = list(range(L)) * max(1, 96 // L)
    outs, m = [], -(-(h.size - 1) // M) + 1
    for p in phases:                                            # the next output of phase p whose window is clear of the last one
        m += (p * inv_M - m) % L if L > 1 else 0
        outs.append(m)
        m += gap
    n_in = (outs[-1] * M) // L + 1
    x = rng.integers(TB.S24_MIN, TB.S24_MAX + 1, size=(n_in, 1))
    want, sums, offsets = [], [], []
    for i, m in enumerate(outs):
        offset = (0, 0, 1, 0, 0, -1)[i % 6]
        acc = TB.plant_tie(rng, h, L, M, m, x, 0, 24, offset, big=(i % 5 == 4))
        assert acc is not None, f"phase {(m * M) % L} has no odd coefficient"
        q = (acc >> 28) + (1 if offset >= 0 else 0)             # ties and one above round up, one below rounds down
        want.append(min(max(q, TB.S24_MIN), TB.S24_MAX))
        sums.append(acc)
        offsets.append(offset)
    assert {(m * M) % L for m in outs} == set(range(L))
    sums, offsets, want = np.array(sums, dtype=object), np.array(offsets), np.array(want)
    ties = offsets == 0
    assert (sums[ties] < 0).sum() > 5 and (sums[ties] > 0).sum() > 5
    past = np.array([(s >> 28) + 1 for s in sums])
    assert (ties & (past > TB.S24_MAX)).any() and (ties & (past < TB.S24_MIN)).any()
    got = TB.round_s24(TB.filter_at(h, L, x, 0, np.array(outs) * M))[:, 0]
    assert np.array_equal(got, want)
    d = np.zeros(len(outs), dtype=O.SRC_MSG_DESC)
    d["src_frames"], d["out_frame0"], d["dst_offset"], d["n_frames"] = n_in, outs, np.arange(len(outs)) * 3, 1
    d["ramp_start"], d["ramp_end"], d["attenuation"], d["channels"] = 16384, 16384, 256, 1
    d["src_bits"], d["src_endian"], d["dst_bits"], d["dst_endian"] = 24, BE, 24, BE
    dst = np.zeros(len(outs) * 3, dtype=np.uint8)
    assert ref.process_batch(d, TB.encode(x, 24, BE), dst) == 0
    assert np.array_equal(PM.decode_s24(dst, 1, 24, BE)[:, 0], want)


def test_planar_source_decodes_as_the_packed_one():
    rng = np.random.default_rng(5)
    for bits in (8, 16, 24):
        lo, hi = full_scale(bits)
        y = rng.integers(lo, hi + 1, size=(100, 3))
        d = np.zeros(1, dtype=capi.SRC_MSG_DESC)[0]
        d["src_frames"], d["channels"], d["src_bits"], d["src_endian"] = 100, 3, bits, BE
        packed = TB.decode(TB.encode(y, bits, BE), d)
        d["flags"], d["src_plane_stride"] = TB.FLAG_SRC_PLANAR32, 100 * 4 + 12
        assert np.array_equal(TB.decode(TB.encode(y, bits, BE, planar_stride=100 * 4 + 12), d), packed)
        assert np.array_equal(packed, y << TB.source_shift(bits))


# ------------------------------------------------------------------------------------------ the golden fixture
def sha256_i32(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_library_designs_reproduce_the_fixture_tables():
    fx = fixture()
    assert [(f["rate_in"], f["rate_out"], f["T"]) for f in fx["filters"]] == [(44100, 48000, 32), (96000, 48000, 64), (48000, 44100, 32), (32000, 48000, 32)]
    for f in fx["filters"]:
        L, M, coef = capi.src_design(f["rate_in"], f["rate_out"], f["T"], f["beta"], f["f_pass"])
        assert (L, M) == (f["L"], f["M"]) and sha256_i32(coef) == f["coef_sha256"], f["rate_in"]


def test_model_reproduces_the_fixture():
    for f in fixture()["filters"]:
        L, M, coef = capi.src_design(f["rate_in"], f["rate_out"], f["T"], f["beta"], f["f_pass"])
        assert [i["kind"] for i in f["inputs"]] == list(TB.FIXTURE_INPUTS)
        for inp in f["inputs"]:
            x = TB.fixture_input(inp["kind"], coef, L, M, f["T"])
            y = TB.resample(coef, L, M, f["T"], x, 0, 0, TB.out_frames(L, M, x.shape[0]))
            assert (x.shape[0], y.shape[0]) == (inp["in_frames"], inp["out_frames"])
            assert y[:64].tolist() == inp["first_64"], (f["rate_in"], inp["kind"])
            assert sha256_i32(y) == inp["s24_sha256"], (f["rate_in"], inp["kind"])


def test_fixture_generator_check_mode():
    r = subprocess.run([sys.executable, GENERATOR, "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
