"""The second protected MPEG-4 family at arena offsets of 2^31 and more, in the manner of tests/test_gpu_cenc_far_offsets.py: a small case
laid twice into one batch -- copy 0 near the arenas' start, copy 1 across byte 2^31, across byte 2^32 or beyond it -- inside the two far
blocks of tests/far_cases.py, run once on either route, and compared by windows: both copies' clear bytes against the model of the near
layout, the guards and every alias window against the fill.  The descriptor's arena offsets are the sibling's two (tests/far_cenc_cases.py
moves them); the shares of the subsample table are rows, not places, and the second copy's move by the first's count."""
import numpy as np
import pytest

import cbcs_cases as BC
import far_cases as FAR
import far_cenc_cases as FARC
from ohpipeline_amd import capi
from test_gpu_cenc_far_offsets import moved_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arenas(ctx):
    a = FAR.FarArenas(ctx)                                   # (a failed allocation is an error here, not a skip)
    try:
        yield a
    finally:
        a.close()


@pytest.mark.parametrize("pair", FAR.PAIRS)
@pytest.mark.parametrize("variant", [0, 1], ids=["phases", "plain"])
def test_cbcs(ctx, arenas, variant, pair):
    good = BC.named_good()
    job = BC.Job([BC.stream(good["two_truns_under_one_subsample_senc_behind"], gather_first_row=3), BC.stream(good["cbcs_parts_of_63_to_129_blocks"]),
                  BC.stream(good["cenc_keystream_offsets_and_the_wrap"]), BC.stream(good["cbcs_1_9_constant_iv8_no_senc_alac"]), BC.stream(good["sibling_clear_plain_flac"])])
    assert all(m["status"] == 0 for m in job.models) and (job.want_dst != BC.FILL).sum() > 1000 and job.models[1]["blocks"] > 128 and job.models[0]["subsamples"] == 142
    twin = FAR.Twin(arenas, job.src, np.full(job.dst_bytes, BC.FILL, np.uint8), pair, *FARC.ALIGN["cenc"], BC.FILL)
    twin.prepare()
    copies = [FARC.relocate("cenc", {"descs": job.descs}, twin.src_at[k], twin.dst_at[k])["descs"] for k in (0, 1)]
    copies[1]["packet_first"] += job.n_packets
    copies[1]["run_first"] += job.n_runs
    copies[1]["subsample_first"] += job.n_subsamples
    descs = np.concatenate(copies)
    counts = (2 * job.n_packets, 2 * job.n_runs, 2 * job.n_subsamples)
    capi.cbcs_batch_check(descs, *counts, FAR.SPAN, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.cbcs_batch(descs, *counts, FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.cbcs_paths(batch)["route"] == (capi.MP4F_ROUTE_PLAIN if variant else capi.MP4F_ROUTE_PHASES)
            ctx.cbcs_run(batch, arenas.src, arenas.dst)
            results, runs, packets, samples = ctx.cbcs_results(batch, len(descs), counts[0], counts[1])
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    n, rows, rr = len(job.streams), job.n_packets, job.n_runs
    for k in (0, 1):
        assert results[k * n:(k + 1) * n].tobytes() == job.want_results.tobytes(), k
        assert packets[k * rows:(k + 1) * rows].tobytes() == moved_rows(job.want_packets, "src_offset", twin.dst_at[k]).tobytes(), k
        assert runs[k * rr:(k + 1) * rr].tobytes() == moved_rows(job.want_runs, "data_offset", twin.src_at[k]).tobytes(), k
        assert samples[k * rows:(k + 1) * rows].tobytes() == job.want_samples.tobytes(), k
    twin.check(job.want_dst, f"cbcs {pair}")
