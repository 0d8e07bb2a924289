"""The DSD file layer on the device (ohgpu_dsd_file_*, csrc/dsd_file_kernel.hip) against the independent model
(tests/dsd_file_textbook.py), byte for byte and on both routes (the two launches, and the plain one a batch created under kernel
variant 1 takes, each first asserted through ohgpu_batch_paths_info): every result, and the whole destination arena -- pre-filled with
0xA5, with guard bytes in front of, between and behind the streams' runs.  The shapes are the smallest at which the conversion can go
wrong (tests/dsd_file_cases.py's phase_sweep and shape_sweep): DSF and DFF in the four formats; the audio at all sixteen addresses
mod 16; chunk totals round a lane of 8 chunks, a wave's piece of 2048 and a workgroup's two pieces (4096: the piece and group sizes
are restated in tests/dsd_file_cases.py); seeks; rooms of no block, one block and exactly the stream; prefixes that end inside the
left plane, at the plane boundary, inside the right plane and one byte short of a chunk; every named malformed file beside good
ones.  Every file is at most three DSF plane pairs (24 KB) or, for the 4101 chunks that reach a second workgroup, 16 KB of DFF
audio.  No launch is persistent -- a lane a stream, a wave per piece -- so there is no trip rule to restate."""
import numpy as np
import pytest

import dsd_file_cases as FC
import dsd_file_textbook as FX
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

assert FC.PIECE_CHUNKS == 2048 and FC.GROUP_PIECES == 2 and FC.UNIT_CHUNKS == 8


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["fused", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.dsd_file_route = capi.DSD_FILE_ROUTE_PLAIN if request.param else capi.DSD_FILE_ROUTE_FUSED
    yield ctx
    ctx.set_kernel_variant(0)


@pytest.fixture(scope="module")
def shapes():
    return FC.Job(FC.shape_sweep())


@pytest.fixture(scope="module")
def phases():
    return FC.phase_sweep()


def run(ctx, job, runs=1, stream=None):
    capi.dsd_file_batch_check(job.descs, job.src.size, job.dst_bytes)
    d_src, d_dst = ctx.upload(job.src), ctx.malloc(job.dst_bytes)
    assert d_src.value % 16 == 0 and d_dst.value % 16 == 0                     # (the phases of the jobs are those of the device)
    b = ctx.dsd_file_batch(job.descs, job.src.size, job.dst_bytes)
    try:
        assert ctx.batch_paths(b)["dsd_file_route"] == ctx.dsd_file_route
        for _ in range(runs):
            ctx.memset(d_dst, FC.FILL, job.dst_bytes)
            ctx.sync()
            ctx.dsd_file_run(b, d_src, d_dst, stream)
            results = ctx.dsd_file_results(b, len(job.streams))
            FC.assert_same(results, ctx.download(d_dst, job.dst_bytes), job)
        ms = ctx.dsd_file_phase_ms(b)
        assert all(v >= 0 for v in ms) and (ctx.dsd_file_route == capi.DSD_FILE_ROUTE_FUSED or ms[1] == 0.0)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return results


def test_the_audio_at_every_address_in_every_format(vctx, phases):
    seen = {(m["kind"], int(d["pad_bytes_per_chunk"]), phases.phase(i)) for i, (m, d) in enumerate(zip(phases.models, phases.descs))}
    assert seen == {(kind, P, phase) for kind in (FX.DSF, FX.DFF) for _, P in FC.FORMATS for phase in range(16)}
    # on the fused route every one of these has a body of whole lanes: every (kind, P) at every phase goes through the 16-byte path
    assert all(FC.has_wide_body(phases, i) for i in range(len(phases.streams)))
    run(vctx, phases)


def test_the_shape_sweep(vctx, shapes):
    models = shapes.models
    assert {m["status"] for m in models} == set(range(5))
    for kind in (FX.DSF, FX.DFF):
        assert {m["chunks_total"] for m in models if m["kind"] == kind} >= set(FC.TOTALS)
        assert {int(d["chunk_first"]) for m, d in zip(models, shapes.descs) if m["kind"] == kind} >= {0, 1, 2047, 2048, 2050, 2101}
        for W, P in FC.FORMATS:
            mine = [i for i, (m, d) in enumerate(zip(models, shapes.descs)) if m["kind"] == kind and (int(d["sample_block_words"]), int(d["pad_bytes_per_chunk"])) == (W, P)]
            assert any(FC.has_wide_body(shapes, i) for i in mine)
            assert any(models[i]["chunks_written"] > FC.PIECE_CHUNKS for i in mine)                      # a second wave's piece
            assert any(0 < models[i]["chunks_written"] < models[i]["chunks_available"] for i in mine)    # a room shorter than the audio
            assert any(models[i]["chunks_available"] < models[i]["chunks_total"] for i in mine)          # a prefix
            assert W - P == 1 or any(models[i]["bytes_written"] > models[i]["chunks_written"] * (4 + P) for i in mine)   # a 0x69 fill (a block of one chunk has none)
        assert any(m["kind"] == kind and m["chunks_written"] > FC.PIECE_CHUNKS * FC.GROUP_PIECES for m in models)   # a second workgroup
    run(vctx, shapes)


def test_every_named_file_in_every_format(vctx):
    good, bad = FC.named_good(), FC.named_malformed()
    job = FC.Job([FC.stream(w, W, P) for w in good.values() for W, P in FC.FORMATS] + [FC.stream(data, 8, 4) for data, _, _ in bad.values()])
    results = run(vctx, job)
    assert [(int(r["status"]), int(r["error_offset"])) for r in results[4 * len(good):]] == [(status, at) for _, status, at in bad.values()]


def test_an_empty_stream_and_an_empty_batch(vctx):
    good = FC.named_good()["dff_100"]
    run(vctx, FC.Job([FC.stream(b""), FC.stream(good), FC.stream(good, room=0), FC.stream(b"", room=0)]))
    run(vctx, FC.Job([FC.stream(b"")]))
    b = vctx.dsd_file_batch(np.zeros(0, dtype=capi.DSD_FILE_STREAM_DESC), 0, 0)
    try:
        vctx.dsd_file_run(b, None, None)
        assert vctx.dsd_file_results(b, 0).size == 0
    finally:
        vctx.batch_destroy(b)


def test_a_second_run_and_a_second_batch_allocate_nothing(vctx):
    jobs = [FC.Job([FC.stream(FC.make(FX.DSF, 2500, 71), 6, 2), FC.stream(FC.make(FX.DFF, 900, 72), 2, 0)]),
            FC.Job([FC.stream(FC.make(FX.DSF, 2500, 73), 6, 2), FC.stream(FC.make(FX.DFF, 900, 74), 2, 0)])]
    assert jobs[0].models[0]["blocks"] != jobs[1].models[0]["blocks"] and np.array_equal(jobs[0].descs, jobs[1].descs)
    d_src, d_dst = vctx.malloc(jobs[0].src.size), vctx.malloc(jobs[0].dst_bytes)
    b = vctx.dsd_file_batch(jobs[0].descs, jobs[0].src.size, jobs[0].dst_bytes)
    try:
        allocs = []
        for job in (jobs[0], jobs[1], jobs[0]):
            vctx.copy_h2d(d_src, job.src)
            vctx.memset(d_dst, FC.FILL, job.dst_bytes)
            vctx.sync()
            vctx.dsd_file_run(b, d_src, d_dst)
            FC.assert_same(vctx.dsd_file_results(b, 2), vctx.download(d_dst, job.dst_bytes), job)
            allocs.append(vctx.device_allocations())
        assert allocs[0] == allocs[1] == allocs[2]
    finally:
        vctx.batch_destroy(b)
    again = vctx.dsd_file_batch(jobs[0].descs, jobs[0].src.size, jobs[0].dst_bytes)             # a second batch of the same shape
    try:
        assert vctx.device_allocations() == allocs[0]
    finally:
        vctx.batch_destroy(again)
        vctx.free(d_src)
        vctx.free(d_dst)


def test_a_run_on_a_callers_stream(vctx):
    good = FC.named_good()
    job = FC.Job([FC.stream(good["dsf_one_pair"], 8, 4), FC.stream(FC.named_malformed()["dff_dst"][0]), FC.stream(good["dff_junk_everywhere"], 1, 0)])
    s = vctx.stream_create()
    try:
        run(vctx, job, runs=2, stream=s)
    finally:
        vctx.stream_destroy(s)


def test_the_host_buffer_call(vctx):
    good = FC.named_good()
    job = FC.Job([FC.stream(good["dsf_fmt_64"], 6, 2), FC.stream(FC.named_malformed()["dsf_msb_first"][0]), FC.stream(good["dff_100"], 2, 0, chunk_first=3, room=5 * 8),
                  FC.stream(good["dff_odd_local"], 8, 4)])
    dst = np.full(job.dst_bytes, FC.FILL, dtype=np.uint8)
    results = vctx.dsd_file_process_host(job.descs, job.src, dst)
    FC.assert_same(results, dst, job)                                         # (only the bytes written come home: the rest of dst stays)
