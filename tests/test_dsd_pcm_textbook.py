"""DSD -> PCM on the CPU: the library's host-side half (ohgpu_dsd_pcm_design, ohgpu_dsd_pcm_window, ohgpu_dsd_pcm_batch_check) against
tests/dsd_pcm_textbook.py and tests/golden/dsd_pcm_textbook.json, and one audio-domain property of the model itself.  No device."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import dsd_pcm_cases as DC
import dsd_pcm_textbook as DP
from ohpipeline_amd import capi

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dsd_pcm_textbook.json")


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


# ---------------------------------------------------------------- the design
@pytest.mark.parametrize("key", list(DC.DESIGNS), ids=[f"D{D}T{T}" for D, T in DC.DESIGNS])
@pytest.mark.parametrize("gain", [1.0, 2.0])
def test_design_equals_the_restatement_and_the_fixture(key, gain):
    dsd_rate, pcm_rate, T = DC.DESIGNS[key]
    D, coef = capi.dsd_pcm_design(dsd_rate, pcm_rate, T, DC.BETA, DC.F_PASS, gain)
    D_model, model = DP.design(dsd_rate, pcm_rate, T, DC.BETA, DC.F_PASS, gain)
    assert (D, T) == key and D_model == D and np.array_equal(coef, model)
    assert coef[-1] == 0 and np.array_equal(coef[:-1], coef[-2::-1])                    # odd length, symmetric: a whole-sample delay
    assert abs(int(coef.sum()) - round(gain * (1 << 28))) <= D * T // 2                 # sum ~ gain * 2^28 within the rounding
    assert DP.bound_ok(coef) and int(np.abs(coef).max()).bit_length() <= 27
    if gain == 1.0:
        f = fixture()["designs"][f"{D}x{T}"]
        assert hashlib.sha256(coef.astype("<i4").tobytes()).hexdigest() == f["coef_sha256"]
        assert (f["dsd_rate"], f["pcm_rate"], f["T"], f["beta"], f["f_pass"]) == (dsd_rate, pcm_rate, T, DC.BETA, DC.F_PASS)


def test_design_refusals():
    """A ratio that is not 8, 16, 32 or 64, a T outside the rule, a short capacity and a gain that breaks sum|coef| < 2^30."""
    for dsd_rate, pcm_rate, T, gain in ((2822400, 44100 * 3, 16, 1.0), (2822400, 705600, 16, 1.0), (2822400, 22050, 16, 1.0), (2822400, 96000, 16, 1.0),
                                        (2822400, 88200, 12, 1.0), (2822400, 88200, 72, 1.0), (2822400, 88200, 0, 1.0), (2822400, 88200, 16, 0.0),
                                        (2822400, 88200, 16, 3.0)):
        with pytest.raises(capi.OhGpuError) as e:
            capi.dsd_pcm_design(dsd_rate, pcm_rate, T, DC.BETA, DC.F_PASS, gain)
        assert e.value.code == capi.ERR_INVALID, (dsd_rate, pcm_rate, T, gain)
    assert not DP.bound_ok(DP.design(2822400, 88200, 16, DC.BETA, DC.F_PASS, 3.0)[1])       # (the model agrees about the bound)
    assert DP.bound_ok(DP.design(2822400, 88200, 16, DC.BETA, DC.F_PASS, 2.0)[1])
    import ctypes as C
    D, small = C.c_uint32(0), np.zeros(511, dtype=np.int32)
    assert capi.lib().ohgpu_dsd_pcm_design(2822400, 88200, 16, DC.BETA, DC.F_PASS, 1.0, small.ctypes.data_as(C.c_void_p), small.size, C.byref(D)) == capi.ERR_INVALID


# ---------------------------------------------------------------- the window
def test_window_equals_the_model():
    for D in DP.DECIMATIONS:
        for T in (8, 16, 24, 64):
            for out0 in (0, 1, 7, T - 1, T, T + 1, 1001, (1 << 40)):
                for n in (1, 2, 15, 16, 17, 512, 4096):
                    assert capi.dsd_pcm_window(out0, n, D, T) == DP.window(out0, n, D, T), (D, T, out0, n)
    for args in ((0, 0, 32, 16), ((1 << 40) + 1, 1, 32, 16), (0, 1, 12, 16), (0, 1, 32, 4), (0, 1, 32, 20)):
        with pytest.raises(capi.OhGpuError) as e:
            capi.dsd_pcm_window(*args)
        assert e.value.code == capi.ERR_INVALID


# ---------------------------------------------------------------- descriptors
def _refused(key, descs, src_bytes, dst_bytes, code):
    with pytest.raises(capi.OhGpuError) as e:
        capi.dsd_pcm_batch_check(key[0], key[1], descs, src_bytes, dst_bytes)
    assert e.value.code == code, (code, str(e.value))


def test_descriptor_validation_by_case():
    key = (32, 16)
    good = DC.Batch(key, 9700, src_lead=1, dst_lead=2).add(1001, 17, (6, 2), before=1, after=1).finish("good")
    S, Dst = good.src.size, good.dst_bytes
    capi.dsd_pcm_batch_check(key[0], key[1], good.descs, S, Dst)
    lo, hi = DP.window(1001, 17, *key)
    tight = good.descs.copy()                                              # exactly the window: accepted
    tight["src_offset"][0] += 8 * (lo - int(tight["src_chunk0"][0]))
    tight["src_chunk0"][0], tight["src_chunks"][0] = lo, hi - lo
    capi.dsd_pcm_batch_check(key[0], key[1], tight, S, Dst)
    for field, value in (("src_chunk0", lo + 1), ("src_chunks", hi - lo - 1)):             # a short window, at either end
        bad = tight.copy()
        bad[field][0] = value
        _refused(key, bad, S, Dst, capi.ERR_INVALID)
    for k in range(12):                                                    # reserved bytes
        bad = good.descs.copy()
        bad["reserved"][0][k] = 1
        _refused(key, bad, S, Dst, capi.ERR_INVALID)
    for W, P in ((0, 0), (6, 1), (7, 3), (6, 4), (8, 2), (4, 2), (2, 2), (12, 6)):          # a bad (W, P): ohgpu_dsd_desc's rule
        bad = good.descs.copy()
        bad["sample_block_words"][0], bad["pad_bytes_per_chunk"][0] = W, P
        _refused(key, bad, 1 << 20, Dst, capi.ERR_INVALID)
    for field, value in (("dst_endian", 0), ("flags", 2), ("ramp_start", capi.RAMP_MAX + 1), ("ramp_end", 65535)):
        bad = good.descs.copy()
        bad[field][0] = value
        _refused(key, bad, S, Dst, capi.ERR_INVALID)
    _refused(key, good.descs, S - 1, Dst, capi.ERR_BOUNDS)                 # bounds: each arena one byte short
    _refused(key, good.descs, S, Dst - 1, capi.ERR_BOUNDS)
    far = good.descs.copy()
    far["dst_offset"][0] = (1 << 64) - 3
    _refused(key, far, S, Dst, capi.ERR_BOUNDS)
    # a stream start needs no chunk before chunk 0; the same window claimed one chunk late is short
    start = DC.Batch(key, 9701).add(0, 16).finish("start")
    capi.dsd_pcm_batch_check(key[0], key[1], start.descs, start.src.size, start.dst_bytes)
    assert int(start.descs["src_chunk0"][0]) == 0 and int(start.descs["src_chunks"][0]) == 16 * 32 // 16
    _refused((12, 16), good.descs, S, Dst, capi.ERR_INVALID)


def test_fixture_cases_are_the_models():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    try:
        import make_dsd_pcm_fixtures as G
    finally:
        sys.path.pop(0)
    fx = fixture()
    assert len(fx["cases"]) == len(G.CASES) == 8
    for entry, (key, out0, fmt, ramp, endian) in zip(fx["cases"], G.CASES):
        case = DC.Batch(key, entry["seed"]).add(out0, 64, fmt, "noise", ramp, endian).finish("fixture")
        assert case.want().tolist() == entry["first_64_frames"] and len(entry["first_64_frames"]) == 384


# ---------------------------------------------------------------- one property in the audio domain
def modulate(x):
    """A second-order delta-sigma modulator: two integrators, the one-bit output fed back into both."""
    bits = np.zeros(x.size, dtype=np.uint8)
    i1 = i2 = 0.0
    for n, v in enumerate(x):
        y = 1.0 if i2 >= 0.0 else -1.0
        bits[n] = y > 0
        i1 += v - y
        i2 += i1 - y
    return bits


def sine_through_the_model():
    """(amplitude / 2^23 of the fitted 1 kHz component, residual after the fit in dBFS): 2^17 bits of a 1 kHz sine at half
    modulation, D = 32, T = 16, the first 2 T output frames (idle history and the filter filling) left out."""
    key = (32, 16)
    D, T = key
    n_bits, rate = 1 << 17, 2822400.0
    x = 0.5 * np.sin(2.0 * math.pi * 1000.0 * np.arange(n_bits) / rate)
    bits = modulate(x)
    y = DP.frames(DC.coef(key), D, np.stack([bits, bits]), 0, 0, n_bits // D)[2 * T:, 0].astype(np.float64)
    t = (np.arange(y.size) + 2 * T) * (D / rate)
    basis = np.stack([np.sin(2.0 * math.pi * 1000.0 * t), np.cos(2.0 * math.pi * 1000.0 * t), np.ones_like(t)], axis=1)
    fit, *_ = np.linalg.lstsq(basis, y, rcond=None)
    residual = y - basis @ fit
    return float(math.hypot(fit[0], fit[1]) / (1 << 23)), float(20.0 * math.log10(np.sqrt(np.mean(residual ** 2)) / (1 << 23)))


def test_a_sine_comes_back_at_its_amplitude():
    """The bounds are the committed model's own values with a margin, written beside the fixture: the amplitude within a thousandth
    of the modulation (the pass band's ripple is far below that), the residual -- the modulator's shaped noise that the filter lets
    through, and the rounding -- no more than 1 dB above what the model gave when the fixture was written."""
    s = fixture()["sine"]
    amplitude, residual_db = sine_through_the_model()
    print(f"amplitude {amplitude:.6f} x 2^23, residual {residual_db:.2f} dBFS")
    assert s["bounds"]["amplitude_low"] < amplitude < s["bounds"]["amplitude_high"]
    assert residual_db < s["bounds"]["residual_dbfs_max"]
    assert abs(amplitude - s["amplitude_over_2_23"]) < 1e-9 and abs(residual_db - s["residual_dbfs"]) < 1e-6
