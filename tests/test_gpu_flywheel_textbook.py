"""FlywheelRamper on the device against tests/flywheel_textbook.py (small batches: the model itself) and against the oracle that
tests/test_flywheel_textbook.py ties to the model (the batch of 3000 lanes), on the inputs of tests/flywheel_cases.py: every input
class (noise, sines, DC, full-scale squares, all-zero training, a single non-zero sample, alternating +/- full scale) at every
decimation factor, in_samples from degree + 1 up, out_frames that no block divides and below one block, batches of 1 / 63 / 64 /
65 / 3000 lanes (one lane = one channel of one request) with 1..10 channels and mixed rates in one batch (a different decimated
count per lane against the shared max_count workspace stride), unaligned source and destination offsets.  Zero differing bytes,
guard bytes included.

The flywheel batch has one kernel (csrc/flywheel_kernel.hip) under every kernel variant: there is no path to choose, so each test
asserts what ohgpu_batch_info reports for the batch it built (requests, training samples) and that the batch ran as ONE batch.

Mutations of the library these tests were seen to fail under on an MI355X (one build each, never committed; wrong bytes only):
  * csrc/flywheel_kernel.hip, Burg's inner loop: `t1 = wrap16(xs[...] + pef[...])` without the wrap16 (a 32-bit sum where the
    reference narrows to TInt16): all 8 tests fail.
  * csrc/flywheel_kernel.hip, output loop: `uint32_t hold = 0` moved out of the block loop (the sample-and-hold counter no longer
    restarts with every block): 7 of 8 fail (the one-lane batch is at 44.1 kHz, decimation 1, where there is no hold).
"""
import numpy as np
import pytest

import flywheel_cases as FC
import flywheel_textbook as FT
import oracle_lib as O
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

FILL = 0xEE
MODEL_MAX_LANES = 200


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def model_ramp(r):
    return np.frombuffer(FT.flywheel_ramp(r["blob"].tobytes(), r["channel_bytes"], r["in_samples"], r["sample_rate"], r["channels"],
                                          r["out_frames"], r["block_frames"]), dtype=np.uint8)


def oracle_ramp(r):
    out = np.zeros(r["out_frames"] * r["channels"] * 4, dtype=np.uint8)
    assert O.lib().ohp_flywheel_ramp(r["blob"].ctypes.data, r["channel_bytes"], r["in_samples"], r["sample_rate"], r["channels"],
                                     r["out_frames"], r["block_frames"], out.ctypes.data) == 0
    return out


def run_batch(ctx, reqs, unaligned, reference):
    src, offs, dst_bytes = FC.layout(reqs, unaligned)
    descs = np.zeros(len(reqs), dtype=capi.FLYWHEEL_DESC)
    want = np.full(dst_bytes, FILL, dtype=np.uint8)
    for i, (r, (so, do)) in enumerate(zip(reqs, offs)):
        descs["src_offset"][i], descs["dst_offset"][i] = so, do
        for f in ("channel_bytes", "in_samples", "out_frames", "block_frames", "sample_rate", "channels"):
            descs[f][i] = r[f]
        y = reference(r)
        want[do:do + y.size] = y
    d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
    ctx.memset(d_dst, FILL, dst_bytes)
    b = ctx.flywheel_batch(descs, src.size, dst_bytes)                  # arenas sized to the byte
    try:
        info = ctx.batch_info(b)
        assert info["n_msgs"] == len(reqs) and info["in_frames"] == sum(r["in_samples"] for r in reqs), info
        ctx.flywheel_run(b, d_src, d_dst)
        got = ctx.download(d_dst, dst_bytes)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        ends = np.cumsum([0] + [r["out_frames"] * r["channels"] * 4 + (8 if unaligned else 0) for r in reqs])
        first = reqs[int(np.searchsorted(ends, bad[0], side="right")) - 1]["name"]
        raise AssertionError(f"{bad.size} differing bytes, first at {bad[:6].tolist()} in request {first}")
    return got


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
def test_input_classes_and_shape_edges(ctx, unaligned):
    """One batch of every input class and shape edge (mixed rates, 1..10 channels), against the MODEL."""
    reqs = FC.input_classes()
    got = run_batch(ctx, reqs, unaligned, model_ramp)
    assert got.any()


@pytest.mark.parametrize("n_lanes", FC.LANE_COUNTS)
def test_lane_counts(ctx, n_lanes):
    """1, 63, 64, 65 lanes (a wave and one lane to either side) against the model; 3000 lanes against the oracle, with a sample of the
    same requests against the model as well."""
    reqs = FC.lanes_batch(n_lanes, 7)
    run_batch(ctx, reqs, True, model_ramp if n_lanes <= MODEL_MAX_LANES else oracle_ramp)
    if n_lanes > MODEL_MAX_LANES:
        run_batch(ctx, reqs[::max(1, len(reqs) // 20)], True, model_ramp)


def test_one_request_at_a_time_equals_the_batch(ctx):
    """Every request of the input classes as a batch of its own (lanes_padded and max_count are then the request's own): same bytes."""
    for r in FC.input_classes()[::3]:
        run_batch(ctx, [r], False, model_ramp)
