"""The RAOP receiver at arena offsets of 2^31 and more, in the manner of tests/test_gpu_cenc_far_offsets.py: a small job laid twice into
one batch -- copy 0 near the source arena's start, copy 1 across byte 2^31, across byte 2^32 or beyond it -- inside the far blocks of
tests/far_cases.py, run once on either route.  The family writes to no arena: both copies' records and results must be the model's of
the near layout, the packet rows the near layout's moved by the copy's place, and the small destination window that FAR.Twin keeps
beside it (this family is handed none) comes back as it went in."""
import numpy as np
import pytest

import far_cases as FAR
import far_raop_rx_cases as FARR
import raop_rx_cases as RC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu
FILL = 0xA5


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
@pytest.mark.parametrize("variant", [0, 1], ids=["wave", "plain"])
def test_raop_rx(ctx, arenas, variant, pair):
    job = RC.Job(RC.lossy_streams()[:6] + RC.shape_streams()[:4])
    n, rows = len(job.streams), len(job.table)
    assert job.want_results["n_output"].sum() > 300 and any(r["n_pending"] for r in job.want_results)
    untouched = np.full(64, FILL, np.uint8)
    twin = FAR.Twin(arenas, np.frombuffer(job.src, dtype=np.uint8), untouched, pair, *FARR.ALIGN["raop_rx"], FILL)
    twin.prepare()
    grams = np.concatenate([FARR.relocate("raop_rx", {"datagrams": job.d_grams}, twin.src_at[k], 0)["datagrams"] for k in (0, 1)])
    streams = np.concatenate([job.d_streams, job.d_streams])
    streams["first_datagram"][n:] += rows
    capi.raop_rx_batch_check(streams, grams, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.raop_rx_batch(streams, grams, FAR.SPAN)
    finally:
        ctx.set_kernel_variant(0)
    try:
        assert ctx.batch_paths(batch)["raop_rx_route"] == (2 if variant else 1)
        ctx.raop_rx_run(batch, arenas.src)
        results, records = ctx.raop_rx_results(batch, 2 * n, 2 * rows)
        packets = ctx.raop_rx_packets(batch, 2 * rows)
    finally:
        ctx.batch_destroy(batch)
    for k in (0, 1):
        assert results[k * n:(k + 1) * n].tobytes() == job.want_results.tobytes(), k
        assert records[k * rows:(k + 1) * rows].tobytes() == job.want_records.tobytes(), k
        moved = job.want_rows.copy()
        moved["src_offset"][moved["bytes"] + moved["src_offset"] != 0] += np.uint64(twin.src_at[k])      # (a row behind the last output reads zero)
        assert packets[k * rows:(k + 1) * rows].tobytes() == moved.tobytes(), k
    twin.check(untouched, f"raop_rx {pair}")
