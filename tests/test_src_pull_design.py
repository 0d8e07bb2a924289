"""CPU checks of the pulled resampler's host side: the descriptor's layout, the Q28 table's shape and bounds, what
the design refuses, the prototype's frequency response at both extreme pulls, and ohgpu_src_pull_step / ohgpu_src_pull_window
against their formulas.  No device is needed."""
import os
import subprocess

import numpy as np
import pytest

import src_pull_model as PM
from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (rate_in, rate_out, taps, max_pull, beta): the conversions the adapter uses most, at the default pull range and at 2 %.  T = 32 needs
# beta = 8 to keep -80 dB where the transition band is narrowest (48 -> 48 kHz, 0.166 cycles per input frame); 96 -> 48 kHz needs T = 64
DESIGNS = [(44100, 48000, 32, 0.001, 8.0), (48000, 48000, 32, 0.001, 8.0), (44100, 48000, 64, 0.001, 9.0), (48000, 48000, 64, 0.001, 9.0),
           (96000, 48000, 64, 0.001, 8.0), (44100, 48000, 64, 0.02, 9.0), (48000, 48000, 64, 0.02, 9.0)]
F_PASS = 20000.0
PASS_DB, STOP_DB = 0.01, -80.0


def test_pull_desc_layout_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    fields = ["src_offset", "src_frame0", "src_frames", "pos_frame", "step", "dst_offset", "pos_frac", "n_frames", "ramp_start",
              "ramp_end", "attenuation", "channels", "src_bits", "src_endian", "dst_bits", "dst_endian", "flags", "reserved",
              "src_plane_stride"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\nint main(){printf("%zu", sizeof(ohgpu_src_pull_msg_desc));' +
                   "".join(f'printf(" %zu", offsetof(ohgpu_src_pull_msg_desc, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == capi.SRC_PULL_MSG_DESC.itemsize == 80
    assert out[1:] == [capi.SRC_PULL_MSG_DESC.fields[f][1] for f in fields]


@pytest.mark.parametrize("rate_in,rate_out,T,max_pull,beta", DESIGNS)
def test_table_shape_rows_and_bound(rate_in, rate_out, T, max_pull, beta):
    C = capi.src_pull_design(rate_in, rate_out, T, 8, beta, F_PASS, max_pull).astype(np.int64)
    assert C.shape == (257, T)
    assert np.array_equal(C[256, :-1], C[0, 1:]) and C[256, -1] == 0          # row P is row 0 moved on one tap (h[T*P] = 0)
    sums = C.sum(axis=1)
    assert np.all(np.abs(sums[:256] - (1 << 28)) <= T // 2)                    # rows 0 .. P-1: DC gain 1 within the rounding
    assert sums[256] == sums[0] - C[0, 0]                                      # ... and row P short by the prototype's first tap
    assert abs(C[0, 0]) < (1 << 28) >> 14
    bound = np.maximum(np.abs(C[:-1]), np.abs(C[1:])).sum(axis=1)
    assert bound.max() < (1 << 30)                                             # exact fp64 accumulation
    assert np.abs(np.diff(C, axis=0)).max() < (1 << 30)


def test_design_refusals():
    with pytest.raises(capi.OhGpuError) as e:
        capi.src_pull_design(44100, 48000, 32, 17)
    assert e.value.code == capi.ERR_INVALID
    for T in (16, 48, 128):
        with pytest.raises(capi.OhGpuError) as e:
            capi.src_pull_design(44100, 48000, T, 8)
        assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.OhGpuError) as e:                                  # f_stop = 48000 - 24500 < f_pass
        capi.src_pull_design(44100, 48000, 32, 8, f_pass=24500.0)
    assert e.value.code == capi.ERR_INVALID and "stop edge" in capi.last_error()
    with pytest.raises(capi.OhGpuError) as e:                                  # a pull so wide the edges cross
        capi.src_pull_design(48000, 48000, 32, 8, max_pull=0.2)
    assert e.value.code == capi.ERR_INVALID
    coef = np.zeros(10, dtype=np.int32)                                        # capacity below (P + 1) * T
    assert capi.lib().ohgpu_src_pull_design(44100, 48000, 32, 8, 8.0, F_PASS, 0.001, coef.ctypes.data, coef.size) == capi.ERR_INVALID


def _response_db(C, P):
    """(f, |H(f)| in dB relative to DC) of the prototype the table samples, h[p + k*P] = C[p][k] for rows 0 .. P-1, on a grid of
    P / 2^21 cycles per input frame from 0 to P / 2."""
    h = C[:P].astype(np.float64).T.reshape(-1)
    H = np.abs(np.fft.rfft(h, 1 << 21))
    with np.errstate(divide="ignore"):
        return np.arange(H.size) * P / (1 << 21), 20 * np.log10(H / abs(h.sum()))


def band_figures(rate_in, rate_out, T, max_pull, beta, P=256):
    """(worst pass-band deviation in dB up to f_pass, worst stop-band level in dB from f_stop) over both extreme pulls."""
    f, db = _response_db(capi.src_pull_design(rate_in, rate_out, T, 8, beta, F_PASS, max_pull), P)
    worst_pass, worst_stop = 0.0, -1e9
    for pull in (-max_pull, max_pull):
        r = rate_in * (1.0 + pull)                                             # the input rate the stream actually runs at
        worst_pass = max(worst_pass, np.abs(db[f <= F_PASS / r]).max())
        worst_stop = max(worst_stop, db[f >= (rate_out - F_PASS) / r].max())
    return worst_pass, worst_stop


@pytest.mark.parametrize("rate_in,rate_out,T,max_pull,beta", DESIGNS)
def test_prototype_bands_hold_at_both_extreme_pulls(rate_in, rate_out, T, max_pull, beta):
    worst_pass, worst_stop = band_figures(rate_in, rate_out, T, max_pull, beta)
    assert worst_pass <= PASS_DB, worst_pass
    assert worst_stop <= STOP_DB, worst_stop


def test_step_matches_formula():
    rng = np.random.default_rng(7)
    cases = [(44100, 48000, PM.NOMINAL), (48000, 48000, PM.NOMINAL), (48000, 48000, PM.multiplier_of(1000)),
             (48000, 48000, PM.multiplier_of(-1000)), (44100, 48000, PM.multiplier_of(1000)), (44100, 48000, PM.multiplier_of(-1000)),
             (192000, 48000, PM.NOMINAL), (8000, 384000, PM.NOMINAL), (48000, 44100, (1 << 32) - 1)]
    cases += [(int(a), int(b), int(m)) for a, b, m in zip(rng.choice([8000, 22050, 44100, 48000, 88200, 96000, 176400, 192000], 50),
                                                       rng.choice([44100, 48000, 96000], 50), rng.integers(1 << 30, 1 << 32, 50))]
    for ri, ro, m in cases:
        want = PM.step_of(ri, ro, m)
        if 0 < want <= capi.SRC_PULL_MAX_STEP:
            assert capi.src_pull_step(ri, ro, m) == want, (ri, ro, m)
        else:
            with pytest.raises(capi.OhGpuError):
                capi.src_pull_step(ri, ro, m)
    with pytest.raises(capi.OhGpuError):
        capi.src_pull_step(48000, 48000, 0)                                    # zero step
    with pytest.raises(capi.OhGpuError):
        capi.src_pull_step(384000, 8000, PM.NOMINAL)                           # 48 input frames per output: beyond the maximum
    with pytest.raises(capi.OhGpuError):
        capi.src_pull_step(0, 48000, PM.NOMINAL)


def test_window_matches_formula():
    rng = np.random.default_rng(11)
    steps = [PM.step_of(44100, 48000), PM.step_of(48000, 48000), PM.step_of(48000, 48000, PM.multiplier_of(1000)),
             PM.step_of(48000, 48000, PM.multiplier_of(-1000)), PM.step_of(44100, 48000, PM.multiplier_of(20000)), 1, capi.SRC_PULL_MAX_STEP]
    fracs = [0, 1, (1 << 31), (1 << 32) - 1, (1 << 32) - 7]
    for T in (32, 64):
        for st in steps:
            for frac in fracs:
                for pos in (0, 5, T - 1, T, 10 ** 9, 1 << 47):
                    for n in (1, 2, 240, 9216):
                        assert capi.src_pull_window(pos, frac, st, n, T) == PM.window(pos, frac, st, n, T), (pos, frac, st, n, T)
        for _ in range(200):
            pos, frac = int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 32))
            st, n = int(rng.integers(1, capi.SRC_PULL_MAX_STEP)), int(rng.integers(1, 9217))
            assert capi.src_pull_window(pos, frac, st, n, T) == PM.window(pos, frac, st, n, T)
    for bad in [(0, 0, 0, 10, 32), (0, 0, capi.SRC_PULL_MAX_STEP + 1, 10, 32), (0, 0, 1 << 33, 0, 32), (0, (1 << 32) - 1, 1 << 34, (1 << 32) - 1, 32)]:
        with pytest.raises(capi.OhGpuError) as e:
            capi.src_pull_window(*bad)
        assert e.value.code == capi.ERR_INVALID


def stream_design(rate_in, rate_out, f_pass=20000.0, max_pull=0.001):
    """PullableSampleRateConverter::StreamDesign restated (DESIGN.md 4b "Per stream"): (T, pass edge in Hz)."""
    a = rate_in if rate_out >= 2 * rate_in else rate_out
    widest = lambda tr: (a / (1 + max_pull) - tr * rate_in) / (1 / (1 + max_pull) + 1 / (1 - max_pull))
    cap = min(f_pass, f_pass * min(rate_in, rate_out) / 44100.0)
    T = 32 if widest(0.1655) >= cap else 64
    return T, min(cap, widest(0.1655 if T == 32 else 0.09))


@pytest.mark.parametrize("rate_out", [48000, 44100])
@pytest.mark.parametrize("rate_in", [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 352800, 384000])
def test_every_source_rate_gets_a_design_that_holds_80_db(rate_in, rate_out):
    T, fp = stream_design(rate_in, rate_out)
    if (rate_in, rate_out) in ((44100, 48000), (48000, 48000)):
        assert (T, fp) == (32, 20000.0)                                        # the common cases keep the whole 20 kHz
    f, db = _response_db(capi.src_pull_design(rate_in, rate_out, T, 8, 8.0, fp, 0.001), 256)
    f_stop = rate_in - fp if rate_out >= 2 * rate_in else rate_out - fp
    for pull in (-0.001, 0.001):
        r = rate_in * (1.0 + pull)
        assert np.abs(db[f <= fp / r]).max() <= PASS_DB
        assert db[f >= f_stop / r].max() <= STOP_DB
