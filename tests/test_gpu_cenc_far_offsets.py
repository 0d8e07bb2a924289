"""The protected MPEG-4 family at arena offsets of 2^31 and more, in the manner of tests/test_gpu_far_offsets.py: its small case laid
twice into one batch -- copy 0 near the arenas' start, copy 1 across byte 2^31, across byte 2^32 or beyond it -- inside the two far blocks
of tests/far_cases.py, run once on either route, and compared by windows: both copies' clear bytes against the model of the near layout,
the guards and every alias window against the fill.  The packet rows are places in the DESTINATION arena and move by that side's shift,
the run rows' data_offset by the source's; everything else is the near copy's."""
import numpy as np
import pytest

import cenc_cases as CC
import far_cases as FAR
import far_cenc_cases as FARC
from ohpipeline_amd import capi

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


def moved_rows(rows, field, shift):
    out = rows.copy()
    blank = bytes([0xA5]) * rows.dtype.itemsize
    for k in range(out.size):
        if out[k].tobytes() != blank:
            out[field][k] += np.uint64(shift)
    return out


@pytest.mark.parametrize("pair", FAR.PAIRS)
@pytest.mark.parametrize("variant", [0, 1], ids=["phases", "plain"])
def test_cenc(ctx, arenas, variant, pair):
    good = CC.named_good()
    job = CC.Job([CC.stream(good["two_truns_under_one_senc_behind"], gather_first_row=3), CC.stream(good["alac_iv8"]), CC.stream(good["clear_plain_flac"])])
    assert all(m["status"] == 0 for m in job.models) and (job.want_dst != CC.FILL).sum() > 1000 and job.models[0]["blocks"] > 64
    twin = FAR.Twin(arenas, job.src, np.full(job.dst_bytes, CC.FILL, np.uint8), pair, *FARC.ALIGN["cenc"], CC.FILL)
    twin.prepare()
    copies = [FARC.relocate("cenc", {"descs": job.descs}, twin.src_at[k], twin.dst_at[k])["descs"] for k in (0, 1)]
    copies[1]["packet_first"] += job.n_packets
    copies[1]["run_first"] += job.n_runs
    descs = np.concatenate(copies)
    capi.cenc_batch_check(descs, 2 * job.n_packets, 2 * job.n_runs, FAR.SPAN, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.cenc_batch(descs, 2 * job.n_packets, 2 * job.n_runs, FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.cenc_paths(batch)["route"] == (capi.MP4F_ROUTE_PLAIN if variant else capi.MP4F_ROUTE_PHASES)
            ctx.cenc_run(batch, arenas.src, arenas.dst)
            results, runs, packets, samples = ctx.cenc_results(batch, len(descs), 2 * job.n_packets, 2 * job.n_runs)
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
    twin.check(job.want_dst, f"cenc {pair}")
