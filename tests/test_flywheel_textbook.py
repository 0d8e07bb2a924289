"""tests/flywheel_textbook.py (FlywheelRamper from its definition, every 16/32-bit narrowing an explicit wrap on Python integers)
held to the reference's own known answers DIRECTLY (TestFlywheelRamper.cpp Test1-Test6, the numbers of
tests/test_oracle_flywheel_kats.py -- here without the oracle in between), then to the oracle byte for byte on every input class
and shape edge of tests/flywheel_cases.py, and to the fixture tests/golden/pcm_textbook.json.

Readings of the reference recorded here:
  * FlywheelRamper.cpp:273 `(((TInt64)sn) << 13) / (TInt64)sd` is undefined for sd == 0 with sn != 0 (sd is a 32-bit sum of
    squares: it can wrap to 0).  The model raises; test_no_shared_input_reaches_the_undefined_division shows that none of the inputs
    the CPU and GPU tests share gets there (share of inputs excluded: 0).
  * FlywheelRamper.cpp:191 takes sampleCount from the WHOLE buffer's size although :184-189 skips the oldest bytes when the buffer
    is longer than expected -- with surplus bytes the reference would read past the buffer's end.  The C ABI (include/ohgpu.h) and
    the oracle define the count as in_samples / decimation, and so does the model; the StarvationRamper's surplus is at most
    a rounding's worth of samples and below one decimated sample, where the two agree.
  * FlywheelRamper.cpp:86, 118-121: the sample-and-hold counter restarts with every block of at most block_frames, so a block
    length that the decimation factor does not divide shortens the last hold of the block.  Model and oracle agree.
No disagreement between model and oracle was met.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import flywheel_cases as FC
import flywheel_textbook as FT
import oracle_lib as O
from test_oracle_flywheel_kats import BURG_IN_1, BURG_IN_2

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pcm_textbook.json")


def feedback(degree, descale, coeff_fmt, data_fmt, out_fmt, coeffs, samples, n):
    m = FT.FeedbackModel(degree, descale, coeff_fmt, data_fmt, out_fmt, coeffs, samples)
    return [m.next_sample() & 0xffffffff for _ in range(n)]


def test_feedback_model_known_answers():
    """TestFlywheelRamper.cpp Test1 (:111-157), Test2 (:160-271), Test3 (:274-320), Test4 (:323-400), Test5 (:403-520)."""
    assert feedback(4, 8, 1, 1, 1, [0x01000000, 0x02000000, 0x04000000, 0x08000000],
                    [0x01000000, 0x02000000, 0x04000000, 0x08000000], 4) == [0x00aa0000, 0x00555400, 0x002b5200, 0x0016fa00]
    cases = {(1, 1, 1): (0x20000, 0x400), (2, 1, 1): (0x40000, 0x1000), (3, 1, 1): (0x80000, 0x4000),
             (4, 1, 1): (0x100000, 0x10000), (1, 2, 1): (0x40000, 0x800), (1, 3, 1): (0x80000, 0x1000),
             (1, 4, 1): (0x100000, 0x2000), (1, 1, 2): (0x10000, 0x200), (1, 1, 3): (0x8000, 0x100),
             (1, 1, 4): (0x4000, 0x80), (2, 2, 2): (0x40000, 0x1000)}
    for (cf, df, of), want in cases.items():
        assert tuple(feedback(2, 8, cf, df, of, [0x01000000, 0], [0x01000000, 0], 2)) == want, (cf, df, of)
    one, neg = 0x40000000, 0xc0000000
    assert feedback(6, 8, 2, 2, 2, [one, 0, 0, 0, 0, 0], [one, 0, 0, 0, 0, 0], 10) == [one] * 10
    assert feedback(6, 8, 2, 2, 2, [0, one, 0, 0, 0, 0], [one, 0, 0, 0, 0, 0], 8) == [0, one] * 4
    assert feedback(6, 8, 2, 2, 2, [0, 0, one, 0, 0, 0], [one, 0, 0, 0, 0, 0], 6) == [0, 0, one] * 2
    assert feedback(6, 8, 2, 2, 2, [neg, 0, 0, 0, 0, 0], [one, 0, 0, 0, 0, 0], 6) == [neg, one] * 3
    assert feedback(6, 8, 2, 2, 2, [0, neg, 0, 0, 0, 0], [one, 0, 0, 0, 0, 0], 6) == [0, neg, 0, one, 0, neg]
    assert feedback(6, 8, 2, 2, 2, [0, 0, neg, 0, 0, 0], [one, 0, 0, 0, 0, 0], 12) == [0, 0, neg, 0, 0, one] * 2


def test_burgs_method_known_answers():
    """Test6 (:549-612): *(samples + i) = (TInt16)(input >> 16), degree 3."""
    assert FT.burgs_method([v >> 16 for v in BURG_IN_1]) == [-16619, 8835, -374]
    assert FT.burgs_method([v >> 16 for v in BURG_IN_2]) == [-14748, 5235, 1360]


def test_decimation_and_coefficient_overflow():
    assert [FT.decimation_factor(r) for r in (44100, 48000, 88200, 96000, 176400, 192000, 352800, 384000)] == [1, 1, 2, 2, 4, 4, 1, 1]
    assert [FC.decimation(r) for r in FC.RATES] == [FT.decimation_factor(r) for r in FC.RATES]
    assert FT.coeff_overflow([-16619, 8835, -374]) == 0
    assert FT.coeff_overflow([-16619, 300, 0]) == -16619 + 300 + 8192
    assert FT.coeff_overflow([100, 200, 300]) == 0
    assert FT.coeff_overflow([8000, 300, 0]) == 108
    rng = np.random.default_rng(5)
    for _ in range(2000):                                       # ... and the oracle's, on sums that wrap in 16 bits
        c = rng.integers(-32768, 32768, size=3).astype(np.int16)
        assert FT.coeff_overflow(c.tolist()) == O.lib().ohp_flywheel_coeff_overflow(c.ctypes.data, 3, 3), c


def test_burgs_method_equals_the_oracle_on_sixteen_bit_extremes():
    """Burg's method alone, on data that are NOT halved first (the kernel's and the reference's function takes any 16-bit data):
    the 16-bit sums t1 / t2 and the 32-bit sums sn / sd wrap for real."""
    rng = np.random.default_rng(11)
    done = 0
    for k in range(300):
        n = int(rng.integers(4, 60))
        kind = k % 4
        x = (rng.integers(-32768, 32768, size=n) if kind == 0 else
             np.where(np.arange(n) % 2 == 0, 32767, -32768) if kind == 1 else
             rng.choice([-32768, 32767, 0, 1, -1], size=n) if kind == 2 else
             np.round(30000 * np.sin(np.arange(n) * (0.05 + 0.01 * k)))).astype(np.int16)
        try:
            want = FT.burgs_method(x.tolist())
        except FT.UndefinedDivision:
            continue                                            # (the oracle would divide by zero: nothing to compare)
        out, h = np.zeros(3, dtype=np.int16), np.zeros(3, dtype=np.int16)
        per, pef = np.zeros(n, dtype=np.int16), np.zeros(n, dtype=np.int16)
        O.lib().ohp_burgs_method(x.ctypes.data, n, 3, out.ctypes.data, h.ctypes.data, per.ctypes.data, pef.ctypes.data)
        assert out.tolist() == want, (k, x.tolist())
        done += 1
    assert done >= 290


def oracle_ramp(r):
    out = np.zeros(r["out_frames"] * r["channels"] * 4, dtype=np.uint8)
    rc = O.lib().ohp_flywheel_ramp(r["blob"].ctypes.data, r["channel_bytes"], r["in_samples"], r["sample_rate"], r["channels"],
                                   r["out_frames"], r["block_frames"], out.ctypes.data)
    assert rc == 0
    return out.tobytes()


def model_ramp(r):
    return FT.flywheel_ramp(r["blob"].tobytes(), r["channel_bytes"], r["in_samples"], r["sample_rate"], r["channels"],
                            r["out_frames"], r["block_frames"])


def test_model_equals_oracle_on_every_input_class_and_shape_edge():
    reqs = FC.input_classes()
    assert {FC.decimation(r["sample_rate"]) for r in reqs} == {1, 2, 4}
    assert any(r["out_frames"] < r["block_frames"] for r in reqs) and any(r["out_frames"] % r["block_frames"] for r in reqs)
    assert any(r["in_samples"] // FC.decimation(r["sample_rate"]) == FT.DEGREE + 1 for r in reqs)
    audible = 0
    for r in reqs:
        got = model_ramp(r)
        assert got == oracle_ramp(r), r["name"]
        audible += any(got)
    assert audible > len(reqs) // 2                             # (the zero-trained requests are silent, the others are not)


def test_model_equals_oracle_on_the_lane_count_batches():
    for n_lanes in FC.LANE_COUNTS:
        reqs = FC.lanes_batch(n_lanes, 7)
        for r in reqs[::max(1, len(reqs) // 40)]:               # the model's share; the oracle carries the rest on the device test
            assert model_ramp(r) == oracle_ramp(r), r["name"]


def test_no_shared_input_reaches_the_undefined_division():
    """Every request of every batch the GPU test runs, every channel: training never divides by a wrapped-to-zero sd."""
    batches = [FC.input_classes()] + [FC.lanes_batch(n, 7) for n in FC.LANE_COUNTS]
    lanes = 0
    for reqs in batches:
        for r in reqs:
            blob, cb = r["blob"].tobytes(), r["channel_bytes"]
            for c in range(r["channels"]):
                FT.channel_model(blob[c * cb:(c + 1) * cb], r["in_samples"], r["sample_rate"])      # raises UndefinedDivision if reached
                lanes += 1
    assert lanes > 3000


def test_the_model_raises_where_the_reference_is_undefined():
    """Order 0 has t1 = x[j + 1], t2 = x[j]: for x = -32768, -32768, 0, 0, -32768 the squares add up to 4 * 2^30 = 2^32, which is 0
    in 32 bits, while sn = -2 * 2^30 is not."""
    with pytest.raises(FT.UndefinedDivision):
        FT.burgs_method([-32768, -32768, 0, 0, -32768])
    assert FT.burgs_method([-32768, -32768, 0, 0, -32767]) != [0, 0, 0]      # (one LSB away it is defined)


def test_golden_fixture():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_pcm_textbook_fixtures as G
    finally:
        sys.path.pop(0)
    with open(FIXTURE) as f:
        fx = json.load(f)["flywheel"]
    reqs = G.flywheel_requests()
    assert len(fx) == len(reqs) == 2
    for e, (name, raw, cb, ins, rate, ch, outf, block) in zip(fx, reqs):
        y = FT.flywheel_ramp(raw, cb, ins, rate, ch, outf, block)
        assert e["name"] == name and hashlib.sha256(y).hexdigest() == e["sha256"] and y[:8 * ch].hex() == e["first_frames_hex"]
        r = dict(blob=np.frombuffer(raw, dtype=np.uint8), channel_bytes=cb, in_samples=ins, sample_rate=rate, channels=ch,
                 out_frames=outf, block_frames=block)
        assert oracle_ramp(r) == y
