"""The block resamplers at the rate ratios a pipeline can meet beyond 44.1 and 96 kHz -- ohgpu_src_design and ohgpu_src_create take any
rates, and the planner (csrc/src_plan.cpp) turns L/M into a block geometry: L_blk outputs from M_blk inputs, out_per_drain =
ceil(4L/M) outputs between two drains of the output ring and from it the ring's size, the coefficient table's share of the LDS and so
the waves per workgroup, and the rule that a block holds at least T input frames.  A matrix of cells as tests/test_gpu_src_textbook.py's
(its check_cell: the kernel asserted first, then the four input classes against the textbook model byte for byte), at decimators by
four and eight, 40/147, 147/320 (a 75 KB table), unity, and up-samplers by two, three, four, six and 320/147 -- where three advances in
four emit nothing, or one advance emits six outputs into a 240-byte ring, or a block is exactly T input frames.

Which block kernel a filter gets depends on its largest per-phase sum |c|: below 2^29 the lean kernel, in [2^29, 2^30) round 1's
(stereo, T = 32, OHGPU_BLOCK_FALLBACK_KERNELS).  A cell steers its table into the bracket it is meant for (test_gpu_src_textbook.steered:
the factor from the table's own sum) and Filter asserts the bracket before the filter is created.  DESIGN.md 5.1 has the cells' geometry."""
import pytest

from test_gpu_src_textbook import BE, BLOCK, BLOCK_LAYOUTS, LE, LEAN, LEAN_SUMS, ROUND1_SUMS, S24, V1, cell_id, check_cell
from test_gpu_src_textbook import ctx, filters, ramp_table  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

S24_6, S24_8, S16, MONO16 = (6, 24, LE, 24, BE, False), (8, 24, LE, 24, BE, False), (2, 16, LE, 24, BE, False), (1, 16, LE, 24, BE, False)
# filters: (rate in, rate out, T, pass edge, the bracket of sum |c| the table is steered into -- None: as designed)
D192, D384, D176 = (192000, 48000, 64, 15300.0, None), (384000, 48000, 64, 6700.0, None), (176400, 48000, 64, 16000.0, None)
D88, UNITY, D96_441, D88_441 = (88200, 48000, 32, 20000.0, None), (48000, 48000, 32, 20000.0, None), (96000, 44100, 64, 18000.0, None), (88200, 44100, 64, 18000.0, None)
UP = [(24000, 48000, 32, 10000.0), (16000, 48000, 32, 6000.0), (12000, 48000, 32, 4500.0), (22050, 48000, 32, 9000.0)]
# 8 -> 48 kHz with 32 taps is a block plan too: six outputs per input make 132 outputs the shortest block of whole periods, but a block
# is also whole 64-byte lines of output -- 8 x 132 = 1056 outputs from 176 input frames, more than T.  It has the most outputs between
# two drains (24) and the largest ring (240 bytes) of all cells.
UP6 = (8000, 48000, 32, 3000.0)

# (kernel, the variant the batch is created and run under, filter, layout)
CELLS = (
    # the lean kernel, tables as designed: decimators and unity.  192 -> 48 kHz is the plain 64-tap instantiation (three advances in
    # four emit nothing); 96 -> 44.1 kHz has the fewest waves per workgroup a 64-tap table is granted, and 4704-output blocks
    [(LEAN, 0, D192, S24), (LEAN, 0, D192, S24_8), (LEAN, 0, D384, S24), (LEAN, 0, D176, S24), (LEAN, 0, D176, S24_6), (LEAN, 0, D88, S16),
     (LEAN, 0, UNITY, S24), (LEAN, 0, UNITY, MONO16), (LEAN, 0, D96_441, S24)] +
    # 88.2 -> 44.1 kHz: ANY 2:1 decimator of ohgpu_src_design's rule is half-band -- the cutoff, midway between f_pass and
    # rate_out - f_pass, is a quarter of the input rate whatever f_pass -- so the library picks the half-band 64-tap kernel (asserted from
    # the table's zeros below); under variant 0 that is the workgroup matrix kernel's half-band form, the lean kernel's under variant 4
    [(LEAN, 4, D88_441, S24)] +
    # the lean kernel, up-samplers, tables steered below 2^29
    [(LEAN, 0, UP[0] + (LEAN_SUMS,), lay) for lay in (S24, S24_6, S24_8, MONO16)] +
    [(LEAN, 0, f + (LEAN_SUMS,), S24) for f in UP[1:] + [UP6]] +
    # round 1's block kernel, tables in [2^29, 2^30): the fallback list's five layouts
    [(BLOCK, 0, f + (ROUND1_SUMS,), lay) for f in UP for _, lay in BLOCK_LAYOUTS] +
    [(BLOCK, 0, (32000, 48000, 32, 14500.0, ROUND1_SUMS), S24), (BLOCK, 0, UP6 + (ROUND1_SUMS,), S24)] +
    # no block plan: the planner declines, the generic kernel runs the batch.  12 -> 96 kHz and 12 -> 48 kHz with 64 taps: a block of
    # 128 outputs is 16 or 32 input frames, fewer than T (plan_src_fast: "a block is at least one filter length of input"); 11.025 -> 48
    # kHz with 64 taps: 640 x 64 coefficients are 320 KB, beyond the LDS.  (Tables steered below 2^29, so that the lean kernel would take
    # them: the geometry alone declines)
    [(V1, 0, f + (LEAN_SUMS,), S24) for f in ((12000, 96000, 32, 4500.0), (12000, 48000, 64, 4500.0), (11025, 48000, 64, 4500.0))])


@pytest.mark.parametrize("cell", CELLS, ids=[cell_id(c) for c in CELLS])
def test_every_rate_ratio_equals_the_model(ctx, filters, ramp_table, cell):  # noqa: F811
    kernel, variant, f, lay = cell
    flt = filters(f)
    assert flt.halfband == (f == D88_441)            # which of the two 64-tap kernels a T = 64 plan runs on (csrc/api_src.hip, src_describe)
    check_cell(ctx, flt, ramp_table, kernel, variant, lay, cell_id(cell))
