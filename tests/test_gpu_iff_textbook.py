"""The PCM file layer on the device (ohgpu_iff_*, csrc/iff_pcm_kernel.hip) against the independent model (tests/iff_textbook.py), byte
for byte and on both routes (the two launches, and the plain one a batch created under kernel variant 1 takes, each first asserted
through ohgpu_batch_paths_info): every result, and the whole destination arena -- pre-filled with 0xA5, with guard bytes in front of,
between and behind the streams' runs.  The shapes are the smallest at which the gather can go wrong (tests/iff_cases.py's
shape_sweep and alignment_sweep): every source width, output width and byte order; 1, 2, 3 and 6 channels; frame counts round a
piece and round one workgroup's pieces; the audio at every address mod 16 crossed with the run at every address mod 16; seeks, short
rooms, a file cut in mid-frame, a continuous stream; every kind beside refused neighbours.  No launch is persistent -- a lane a
stream, a workgroup per 1024 pieces -- so there is no trip rule to restate."""
import numpy as np
import pytest

import iff_cases as IC
import iff_textbook as IX
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["fused", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.iff_route = capi.IFF_ROUTE_PLAIN if request.param else capi.IFF_ROUTE_FUSED
    yield ctx
    ctx.set_kernel_variant(0)


@pytest.fixture(scope="module")
def sweep():
    return IC.Job(IC.shape_sweep())


@pytest.fixture(scope="module")
def alignments():
    return IC.alignment_sweep()


def run(ctx, job, runs=1):
    capi.iff_batch_check(job.descs, job.src.size, job.dst_bytes)
    d_src, d_dst = ctx.upload(job.src), ctx.malloc(job.dst_bytes)
    b = ctx.iff_batch(job.descs, job.src.size, job.dst_bytes)
    try:
        assert ctx.batch_paths(b)["iff_route"] == ctx.iff_route
        for _ in range(runs):
            ctx.memset(d_dst, IC.FILL, job.dst_bytes)
            ctx.sync()
            ctx.iff_run(b, d_src, d_dst)
            results = ctx.iff_results(b, len(job.streams))
            IC.assert_same(results, ctx.download(d_dst, job.dst_bytes), job)
        ms = ctx.iff_phase_ms(b)
        assert all(v >= 0 for v in ms) and (ctx.iff_route == capi.IFF_ROUTE_FUSED or ms[1] == 0.0)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return results


def test_the_shape_sweep(vctx, sweep):
    assert {m["status"] for m in sweep.models} == set(range(5))
    assert {(m["src_bit_depth"], m["out_bit_depth"], m["src_endian"]) for m in sweep.models if m["status"] == IX.OK} >= \
        {(s, o, e) for s, o in ((8, 8), (16, 16), (24, 24), (32, 32), (32, 24)) for e in (IX.LITTLE, IX.BIG)}
    assert {m["channels"] for m in sweep.models} >= {1, 2, 3, 6} and any(m["frames_total"] == 0 and m["frames_written"] for m in sweep.models)
    assert any(0 < m["frames_written"] < m["frames_available"] for m in sweep.models) and any(m["frames_available"] < m["frames_total"] for m in sweep.models)
    run(vctx, sweep)


def test_the_audio_at_every_address_and_the_run_at_every_address(vctx, alignments):
    assert len(alignments) >= 4
    for job in alignments:
        run(vctx, job)


def test_every_named_file_under_both_limits(vctx):
    good, bad = IC.named_good(), IC.named_malformed()
    job = IC.Job([IC.stream(w, max_bit_depth=depth) for w in good.values() for depth in (24, 32)] + [IC.stream(data) for data, _, _ in bad.values()])
    for m, w in zip(job.models[0:2 * len(good):2], good.values()):
        IC.check_against_record(m, w)
    run(vctx, job)


def test_three_hundred_damaged_headers_in_one_batch(vctx):
    job = IC.Job([IC.stream(data, frames=48) for data in IC.damaged(300)])
    statuses = [m["status"] for m in job.models]
    assert statuses.count(IX.OK) > 30 and len(set(statuses)) >= 4
    run(vctx, job)


def test_an_empty_stream_and_an_empty_batch(vctx):
    good = IC.named_good()["aifc_sowt"]
    run(vctx, IC.Job([IC.stream(b""), IC.stream(good), IC.stream(good, frames=0, room=0), IC.stream(b"", frames=0, room=0)]))
    run(vctx, IC.Job([IC.stream(b"")]))
    b = vctx.iff_batch(np.zeros(0, dtype=capi.IFF_STREAM_DESC), 0, 0)
    try:
        vctx.iff_run(b, None, None)
        assert vctx.iff_results(b, 0).size == 0
    finally:
        vctx.batch_destroy(b)


def test_a_second_run_and_a_second_batch_allocate_nothing(vctx):
    first = IC.wav(IC.samples(3000, 2, 3, 61), 2)
    other = IC.patched(first, first.data_offset, bytes(range(200)))          # other bytes of the same length
    jobs = [IC.Job([IC.stream(first)]), IC.Job([IC.stream(other, frames=first.frames, room=first.frames * 6)])]
    assert jobs[0].models[0]["pcm"] != jobs[1].models[0]["pcm"] and np.array_equal(jobs[0].descs, jobs[1].descs)
    d_src, d_dst = vctx.malloc(jobs[0].src.size), vctx.malloc(jobs[0].dst_bytes)
    b = vctx.iff_batch(jobs[0].descs, jobs[0].src.size, jobs[0].dst_bytes)
    try:
        allocs = []
        for job in (jobs[0], jobs[1], jobs[0]):
            vctx.copy_h2d(d_src, job.src)
            vctx.memset(d_dst, IC.FILL, job.dst_bytes)
            vctx.sync()
            vctx.iff_run(b, d_src, d_dst)
            IC.assert_same(vctx.iff_results(b, 1), vctx.download(d_dst, job.dst_bytes), job)
            allocs.append(vctx.device_allocations())
        assert allocs[0] == allocs[1] == allocs[2]
    finally:
        vctx.batch_destroy(b)
    again = vctx.iff_batch(jobs[0].descs, jobs[0].src.size, jobs[0].dst_bytes)             # a second batch of the same shape
    try:
        assert vctx.device_allocations() == allocs[0]
    finally:
        vctx.batch_destroy(again)
        vctx.free(d_src)
        vctx.free(d_dst)


def test_the_host_buffer_call(vctx):
    good = IC.named_good()
    job = IC.Job([IC.stream(good["wav_data_first"]), IC.stream(IC.named_malformed()["adpcm"][0]), IC.stream(good["aiff32"], frame_first=2, frames=4),
                  IC.stream(good["wav8_mono"], flags=IX.FLAG_WAV8_UNSIGNED)])
    dst = np.full(job.dst_bytes, IC.FILL, dtype=np.uint8)
    results = vctx.iff_process_host(job.descs, job.src, dst)
    IC.assert_same(results, dst, job)                                         # (only the frames written come home: the rest of dst stays)
