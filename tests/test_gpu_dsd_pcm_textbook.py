"""DSD -> PCM on the device (ohgpu_dsd_pcm_*: csrc/dsd_pcm_kernel.hip) against tests/dsd_pcm_textbook.py, on both routes:

    fast    dsd_pcm_table_kernel, byte-indexed partial sums in LDS -- every filter of N = D * T <= 1024 coefficients, unless kernel
            variant 1 is in force;
    plain   dsd_pcm_kernel_v1, csrc/dsd_pcm_core.h per thread -- kernel variant 1, and filters the tables do not fit.

Conventions, as tests/test_gpu_dsd_textbook.py: both arenas allocated to the byte, the destination pre-filled with 0xA5, the WHOLE
destination arena compared with the model's, zero differing bytes (the specification is integer: no tolerance).  Every check
first asks ohgpu_dsd_pcm_batch_paths which route the batch was planned onto and asserts it.  The shapes and what they are there for:
tests/dsd_pcm_cases.py (tests/test_dsd_pcm_core_cpu.py takes the same batches through the core on the CPU under sanitizers)."""
import json
import os

import numpy as np
import pytest

import dsd_pcm_cases as DC
import dsd_pcm_textbook as DP
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

FILL = DC.FILL
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dsd_pcm_textbook.json")
KEYS = list(DC.DESIGNS)
IDS = [f"D{D}T{T}" for D, T in KEYS]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["fast", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.route = "plain" if request.param else "fast"
    yield ctx
    ctx.set_kernel_variant(0)


@pytest.fixture(scope="module")
def filters(ctx):
    made = {}

    def get(key, coef=None):
        if coef is not None:
            return ctx.dsd_pcm_create(key[0], key[1], coef)
        if key not in made:
            made[key] = ctx.dsd_pcm_create(key[0], key[1], DC.coef(key))
        return made[key]
    yield get
    for f in made.values():
        ctx.dsd_pcm_destroy(f)


def run(ctx, filt, descs, src, dst_bytes, times=1):
    d_src = ctx.upload(src if src.size else np.zeros(1, np.uint8))
    d_dst = ctx.malloc(max(dst_bytes, 1))
    ctx.memset(d_dst, FILL, max(dst_bytes, 1))
    b = ctx.dsd_pcm_batch(filt, descs, src.size, dst_bytes)
    try:
        paths, info = ctx.dsd_pcm_batch_paths(b), ctx.batch_info(b)
        with pytest.raises(capi.OhGpuError):                               # (the PCM / fmt query does not know this kind of batch)
            ctx.batch_paths(b)
        outs, allocs = [], []
        for _ in range(times):
            ctx.dsd_pcm_run(b, d_src, d_dst)
            outs.append(ctx.download(d_dst, dst_bytes) if dst_bytes else np.zeros(0, np.uint8))
            allocs.append(ctx.device_allocations())
            ctx.memset(d_dst, FILL, max(dst_bytes, 1))
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return outs, paths, info, allocs


def check(ctx, filt, case, times=1):
    with_frames = int((case.descs["n_frames"] > 0).sum())
    outs, paths, info, allocs = run(ctx, filt, case.descs, case.src, case.dst_bytes, times)
    fast = ctx.route == "fast" and case.key[0] * case.key[1] <= 1024
    assert paths == {"fast_descs": with_frames if fast else 0, "plain_descs": 0 if fast else with_frames, "launches": 1 if with_frames else 0}, (case.label, paths)
    assert info == DP.totals(case.descs, *case.key), case.label
    for got in outs:
        bad = np.nonzero(got != case.want())[0]
        assert bad.size == 0, f"{case.label} ({ctx.route}): {bad.size} differing bytes, first at {bad[:6].tolist()}"
    return allocs


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_every_shape(vctx, filters, key):
    """n_frames 1, 15, 16, 17, 511, 512, 513, 1025 x out_frame0 0, 7, 1001; P, byte order, ramp, input and offsets rotating."""
    check(vctx, filters(key), DC.shapes(key))


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_every_input_under_every_ramp(vctx, filters, key):
    """Noise, all ones, all zeros, 0x69 and 0xAA x out_frame0 x (unramped, every pair of RAMPS), both byte orders."""
    check(vctx, filters(key), DC.inputs(key))


def test_mixed_batch_twice_allocates_nothing(vctx, filters):
    """64 streams x 2048 frames of mixed P in one launch, run twice: the same bytes, and ohgpu_device_allocations flat."""
    case = DC.mixed()
    assert case.descs.size == 256 and int(case.descs["n_frames"].sum()) == 64 * 2048
    allocs = check(vctx, filters(case.key), case, times=2)
    assert allocs[0] == allocs[1], allocs


def test_a_filter_the_tables_do_not_fit_takes_the_plain_route(vctx, filters):
    """D = 64, T = 24: N = 1536 > 1024, so the batch is planned onto the plain kernel under either variant -- and is still right."""
    key = (64, 24)
    D, coef = capi.dsd_pcm_design(5644800, 88200, 24, DC.BETA, DC.F_PASS, 1.0)
    assert D == 64 and np.array_equal(coef, DP.design(5644800, 88200, 24, DC.BETA, DC.F_PASS, 1.0)[1])
    b = DC.Batch(key, 9400, src_lead=1, dst_lead=1)
    b.add(0, 17, (6, 2), "noise", DC.RAMPS[2]).add(1001, 513, (2, 0), "noise", None, capi.ENDIAN_LITTLE, dst_gap=3).add(7, 16, (8, 4), "idle")
    case = b.finish("long filter")
    case._want = DP.batch_bytes(case.descs, coef, D, case.src, case.dst_bytes, FILL)
    filt = filters(key, coef)
    try:
        outs, paths, _, _ = run(vctx, filt, case.descs, case.src, case.dst_bytes)
        assert paths == {"fast_descs": 0, "plain_descs": 3, "launches": 1}
        assert np.array_equal(outs[0], case.want())
    finally:
        vctx.dsd_pcm_destroy(filt)


def test_golden_fixture(vctx, filters):
    """tests/golden/dsd_pcm_textbook.json: the designs' coefficient hashes, and per case the first 64 output frames the model gave
    when the fixture was written -- the device gives them now."""
    import hashlib
    with open(FIXTURE) as f:
        fx = json.load(f)
    for entry in fx["cases"]:
        key = (entry["D"], entry["T"])
        assert hashlib.sha256(DC.coef(key).astype("<i4").tobytes()).hexdigest() == fx["designs"][f"{key[0]}x{key[1]}"]["coef_sha256"]
        b = DC.Batch(key, entry["seed"])
        b.add(entry["out_frame0"], 64, tuple(entry["format"]), "noise", tuple(entry["ramp"]) if entry["ramp"] else None, entry["dst_endian"])
        case = b.finish("fixture")
        outs, _, _, _ = run(vctx, filters(key), case.descs, case.src, case.dst_bytes)
        assert outs[0].tolist() == entry["first_64_frames"], (key, entry["seed"])


# ---------------------------------------------------------------- validation
def _desc(key, out0=0, n=16, fmt=(2, 0), **over):
    b = DC.Batch(key, 9500).add(out0, n, fmt)
    case = b.finish("one")
    for k, v in over.items():
        case.descs[k][0] = v
    return case


def _refused(ctx, filt, descs, src_bytes, dst_bytes, code):
    before = ctx.device_allocations()
    with pytest.raises(capi.OhGpuError) as e:
        ctx.batch_destroy(ctx.dsd_pcm_batch(filt, descs, src_bytes, dst_bytes))
    assert e.value.code == code, (code, str(e.value))
    assert ctx.device_allocations() == before                              # (a refusal keeps nothing)


def test_refused_descriptors_beside_a_valid_neighbour(vctx, filters):
    """Each refusal by its code, the same descriptor with the field put right accepted and converted right."""
    key = (32, 16)
    filt = filters(key)
    good = _desc(key, out0=1001, n=17, fmt=(6, 2))
    check(vctx, filt, good)                                                # (the neighbour; the context's cache holds blocks from here on)
    S, Dst = good.src.size, good.dst_bytes
    for field, value in (("sample_block_words", 5), ("pad_bytes_per_chunk", 4), ("dst_endian", 0), ("dst_endian", 3), ("flags", 2),
                         ("flags", capi.FLAG_RAMP | 4), ("ramp_start", capi.RAMP_MAX + 1), ("ramp_end", capi.RAMP_MAX + 1),
                         ("src_chunk0", int(good.descs["src_chunk0"][0]) + 1),          # the window starts one chunk late
                         ("src_chunks", int(good.descs["src_chunks"][0]) - 1),          # ... ends one chunk early
                         ("out_frame0", (1 << 40) + 1)):
        bad = good.descs.copy()
        bad[field][0] = value
        _refused(vctx, filt, bad, S, Dst, capi.ERR_INVALID)
    bad = good.descs.copy()
    bad["reserved"][0][7] = 1
    _refused(vctx, filt, bad, S, Dst, capi.ERR_INVALID)
    bad = good.descs.copy()
    bad["flags"][0], bad["n_frames"][0] = capi.FLAG_RAMP, 131072
    _refused(vctx, filt, bad, S, 6 * 131072, capi.ERR_INVALID)
    _refused(vctx, filt, good.descs, S - 1, Dst, capi.ERR_BOUNDS)          # each arena one byte short
    _refused(vctx, filt, good.descs, S, Dst - 1, capi.ERR_BOUNDS)
    two = np.concatenate([good.descs, good.descs])
    two["src_chunks"][1] -= 1
    _refused(vctx, filt, two, S, Dst, capi.ERR_INVALID)                    # behind a good descriptor
    # a message of no frames is accepted wherever its offsets point, and nothing is launched for it
    empty = good.descs.copy()
    empty["n_frames"][0], empty["src_offset"][0], empty["dst_offset"][0] = 0, 1 << 40, 1 << 41
    outs, paths, info, _ = run(vctx, filt, empty, good.src, 8)
    assert paths == {"fast_descs": 0, "plain_descs": 0, "launches": 0} and (outs[0] == FILL).all() and info["n_msgs"] == 1


def test_filter_refusals(ctx):
    """ohgpu_dsd_pcm_create: a (D, T) outside the specification and a coefficient set at the 2^30 bound are refused, one below is taken."""
    for D, T in ((4, 16), (128, 16), (32, 4), (32, 72), (32, 12), (12, 16)):
        with pytest.raises(capi.OhGpuError) as e:
            ctx.dsd_pcm_create(D, T, np.zeros(D * T, dtype=np.int32))
        assert e.value.code == capi.ERR_INVALID
    coef = np.zeros(64, dtype=np.int32)
    coef[:4] = 1 << 28
    with pytest.raises(capi.OhGpuError) as e:
        ctx.dsd_pcm_create(8, 8, coef)
    assert e.value.code == capi.ERR_INVALID
    coef[3] -= 1
    ctx.dsd_pcm_destroy(ctx.dsd_pcm_create(8, 8, coef))


def test_process_host_preserves_uncovered_bytes(vctx, filters):
    """ohgpu_dsd_pcm_process_host: host arrays in and out, bytes between the messages left as they were, nothing allocated when steady."""
    case = DC.inputs((16, 24))
    allocs = []
    for _ in range(3):
        dst = np.full(case.dst_bytes, FILL, dtype=np.uint8)
        vctx.dsd_pcm_process_host(filters(case.key), case.descs, case.src, dst)
        assert np.array_equal(dst, case.want())
        allocs.append(vctx.device_allocations())
    assert allocs[1] == allocs[2], allocs
