"""Every persistent kernel past its first trip.  The hot kernels cap their launch at a few workgroups per CU and loop over a work
list; what they do to go round that loop -- a staging buffer reused behind a barrier or a fence, the next item's input and the one
after's record in flight, a unit claimed with an atomic, counters that reset themselves -- only runs when the list is longer than
the launch.  Each test here reads the device's CU count (tests/device_shape.py), takes from tests/many_trips_cases.py a batch
whose list is longer than a stated multiple of what the launch can hold, ASSERTS THAT LENGTH FIRST (from the documented chunking
rule, from ohgpu_src_batch_units, or from the models' own counts), and then compares the WHOLE destination arena, guard bytes
included, with the reference: zero differing bytes.

"What the launch can hold" is the larger of today's cap at the launch site and what the CUs keep resident (32 waves each, hence
floor(32 / waves per workgroup) workgroups), so that retuning a per-CU constant does not take a test out of the regime.  The
formula is in each test's docstring; tests/test_many_trips_cases.py holds the same conditions at 256 and 304 CUs on the CPU.

Families whose trip tests live with their own suites: the protected MPEG-4 layer's persistent decrypt-gather launch (cenc_crypt_kernel)
in tests/test_gpu_cenc_textbook.py::test_more_chunk_slots_than_the_launch_has_waves, its builder's claims in tests/test_cenc_cases.py.

Mutations of the library (the convention of tests/test_gpu_pcm_textbook.py's docstring): each built once, run once against this
file on an MI355X of 256 CUs right after a run of the unchanged library that passed all of it, never committed.
  * pcm_line_kernel, staged loop: `buf ^= 1` dropped (every later chunk of a wave is converted from the first buffer's stale bytes):
    test_line_kernel_staged_list_every_wave_goes_round FAILED, "282983 of 755360 bytes differ, first at [186882, ...]" -- the
    first trip's chunks are right, everything behind them is wrong.
  * pcm_line_kernel, register loop: `h0 = n0` replaced by `h0 = h0`, in the same library as the change above.  NO RECORD: the first
    register-list test (16to24_heavy) ended in the runtime's "illegal memory access", and everything after it in that process only
    reported the same error.  So this change is not the bytes-only change it was taken for (the stale head's loads and the
    current record's stores no longer describe the same chunk, yet every address in the source is one the first trip used), the
    cause was not established, and it was not run again.  No other change to what the register loop carries from trip to trip
    (h0, h1, has1) is bytes-only beyond doubt either, so the register lists and the narrow Songcast frames have no mutation
    record; what shows that they can fail is the staged record above for the same file's comparison, no more.
  A second library, with the line kernel unchanged and one change in each of four other kernels:
  * dsd_pcm_table_kernel: the loop-top `__syncthreads()` dropped for all threads (every LDS index stays in range): the fast route
    FAILED, "4134 tiles (fast): 1027 of 405535 bytes differ, first at [45627, ...]"; the plain route (another kernel) passed.
  * src_pull_kernel: the same barrier dropped: mixed-T32 FAILED ("128675 of 607123 bytes differ"), mixed-T64 FAILED ("185493 of
    661811"); stereo-T32 PASSED.  In the stereo batch a short tile writes `win` below index 20 or so while the slow readers of a
    256-output tile before it are far above that, so the race has nothing to show unless two long tiles meet; src_pull_kernel<2>'s
    barrier is therefore NOT shown to be needed by this file (its arithmetic and its loop are, by the comparison).
  * src_lean_kernel and src_block_kernel: the two `__hip_atomic_store(..., 0u)` of the counters' reset dropped: in every case on
    those kernels the first run passed and the SECOND FAILED -- stereo_s24 under variants 4 and 2 ("run 2: 15758234 of 26344291
    bytes differ"), halfband_stereo-v4 (12560400 of 26171876), six_s24-v4 (41231475 of 78480633), stereo_to_s16-v0 (10511322 of
    17513453), stereo_s24_block-v0 (15945606 of 26392540); the four cases on src_mfma_wg_kernel (variant 0) passed, as they must.
  No byte-only mutation exists for ohm_wide_kernel, dsd_pcm_kernel_v1 and src_mfma_wg_kernel's unit loop (nothing but the item's
  index goes from one trip to the next: any change to it is an address), nor for flac_run's second attempt (host control flow).
"""
import numpy as np
import pytest

import many_trips_cases as MT
import ohm_textbook as OT
import oracle_lib as O
import pcm_textbook as PT
from device_shape import compute_units
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

FILL = MT.FILL


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[:8].tolist()}"


def run_pcm(ctx, case):
    d_src, d_dst = ctx.upload(case.src), ctx.malloc(case.dst_bytes)
    ctx.memset(d_dst, FILL, case.dst_bytes)
    b = ctx.pcm_batch(case.descs, case.src.size, case.dst_bytes)
    try:
        paths = ctx.batch_paths(b)
        ctx.pcm_run(b, d_src, d_dst)
        return ctx.download(d_dst, case.dst_bytes), paths
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)


def sampled_messages_equal_the_model(case):
    """tests/pcm_textbook.py for every 61st message against the oracle's arena."""
    want = case.want()
    for k in case.sampled():
        d = case.descs[k]
        out = np.frombuffer(PT.process_message(d, case.src), dtype=np.uint8)
        assert np.array_equal(out, want[int(d["dst_offset"]):int(d["dst_offset"]) + out.size]), (case.label, k)


# ---------------------------------------------------------------- 1, 2: the PCM line kernel
def test_line_kernel_staged_list_every_wave_goes_round(ctx):
    """pcm_line_kernel<0, 0>: chunks on list 0 > 3 x W + 131 with W = max(6 x 4, 32) x CUs waves (today's cap: 6 workgroups of 4
    waves per CU; resident: 32 waves per CU): every wave stages into `s_in` four times and more, the record two trips ahead.
    Chunks by the rule ceil(subsamples / 512); the 512-subsample chunks among the small ones make stage_in issue 0, 1, 2 and 3 loads
    for a NEXT chunk, one `s_waitcnt vmcnt` branch each (3 is the most the 2304-byte buffer admits: the fourth branch's `else`)."""
    cus = compute_units()
    case = MT.pcm_staged(cus)
    assert case.counts["chunks"] > 3 * max(6 * 4, 32) * cus + 131, case.counts
    assert case.counts["loads"] == {0, 1, 2, 3} and case.counts["residues"] == set(range(16)), case.counts
    got, paths = run_pcm(ctx, case)
    assert paths["line_planned"] == 1 and paths["launches"] == 1, paths
    assert paths["staged_chunks"] == case.counts["chunks"] and paths["group_chunks"] == 0 and paths["heavy_chunks"] == 0, paths
    same(got, case.want(), case.label)
    sampled_messages_equal_the_model(case)


@pytest.mark.parametrize("which", list(MT.REGISTER_LISTS))
def test_line_kernel_register_list_every_wave_goes_round(ctx, which):
    """pcm_line_kernel<S, D>, the register paths: chunks on the list > 2 x 2 x W + 131 with W = max(6 x 4, 32) x CUs waves, two
    neighbouring chunks per wave and trip, the next trip's heads loaded one trip ahead; an odd count, so that the last trip's
    `has1` / `more1` are false for one wave.  One chunk per message by construction (see the builder): the planner's counts say so."""
    cus = compute_units()
    case = MT.pcm_register(cus, which)
    assert case.counts["group"] + case.counts["heavy"] > 2 * 2 * max(6 * 4, 32) * cus + 131, case.counts
    assert (case.counts["group"] + case.counts["heavy"]) % 2 == 1
    got, paths = run_pcm(ctx, case)
    assert paths["line_planned"] == 1 and paths["launches"] == 1 and paths["staged_chunks"] == 0, paths
    assert paths["group_chunks"] == case.counts["group"] and paths["heavy_chunks"] == case.counts["heavy"], (paths, case.counts)
    same(got, case.want(), case.label)
    sampled_messages_equal_the_model(case)


# ---------------------------------------------------------------- 3: Songcast frames
def run_ohm(ctx, case):
    frames, want, dst_bytes, grams = case.want()
    d_src, d_dst = ctx.upload(case.src), ctx.malloc(dst_bytes)
    ctx.memset(d_dst, FILL, dst_bytes)
    b = ctx.ohm_batch(case.streams, frames, case.fragments, case.src.size, dst_bytes)
    try:
        paths = ctx.batch_paths(b)
        ctx.ohm_run(b, d_src, d_dst)
        return ctx.download(d_dst, dst_bytes), paths
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)


def sampled_datagrams_equal_the_model(case):
    """tests/ohm_textbook.py (headers by struct.pack) over tests/pcm_textbook.py for every 61st datagram against the oracle's."""
    frames, _, _, grams = case.want()
    for k in range(0, case.n, MT.SAMPLE_EVERY):
        fr, d, m = frames[k], case.msgs[k], case.meta[int(frames[k]["stream"])]
        s = case.streams[int(fr["stream"])]
        wire_ch, wire_bits = OT.wire_format(m["ch"], m["bits"])
        header = OT.stream_header(int(s["samples_total"]), m["rate"], int(s["bit_rate"]), int(s["volume_offset"]), wire_bits, wire_ch, m["codec"])
        audio = OT.sender_audio(PT.process_message(d, case.src), m["ch"], m["bits"])
        gram = OT.audio_frame(int(fr["flags"]), int(d["n_frames"]), int(fr["frame"]), int(fr["network_timestamp"]), int(fr["media_latency"]),
                              int(fr["sample_start"]), header, audio)
        assert grams[k][1].tobytes() == gram, (case.label, k)


@pytest.mark.parametrize("bits", MT.OHM_NARROW_BITS)
def test_songcast_narrow_frames_prefix_path_every_trip(ctx, bits):
    """Mono and stereo OHM frames of ONE depth through the frame batch: prefixed chunks > 2 x 2 x W + 67 with W = max(6 x 4, 32) x
    CUs waves of the line kernel (today's cap: 6 workgroups of 4 waves per CU; resident: 32 waves per CU; two chunks per wave and
    trip).  The line kernel keeps a list per (source depth, wire depth) and launches each on its own -- 16 -> 16, 24 -> 24,
    32 -> 24 -- so the condition is per depth: one launch, and the planner's chunk counts add up to the frames.  The prefix load /
    store then runs trip after trip, beside the next trip's heads."""
    cus = compute_units()
    case = MT.ohm_narrow(cus, bits)
    assert case.n > 2 * 2 * max(6 * 4, 32) * cus + 67 and {m["bits"] for m in case.meta} == {bits}
    got, paths = run_ohm(ctx, case)
    assert paths["line_planned"] == 1 and paths["launches"] == 1, paths
    # (the launch's list: a chunk per frame at least -- a prefixed chunk is never appended to its neighbour, the planner may cut a
    # plain one in two at a 128-byte line of the destination; silent ones count as staged)
    assert paths["staged_chunks"] + paths["group_chunks"] + paths["heavy_chunks"] >= case.n, paths
    assert paths["prefixed_chunks"] == case.n == paths["ohm_headers_fused"], paths
    assert paths["ohm_wide_fragments"] == 0 and paths["ohm_headers_separate"] == 0, paths
    same(got, case.want()[1], case.label)
    sampled_datagrams_equal_the_model(case)


def test_songcast_wide_frames_record_loop(ctx):
    """Six- and eight-channel OHM frames: records of ohm_wide_kernel > 2 x W + 67 with W = max(4 x 4, 32) x CUs waves (today's cap:
    4 workgroups of 4 waves per CU; one record per wave and trip).  A record is a fragment with audio: the silent ones among them are
    not the kernel's.  Nothing is carried from one trip to the next in this kernel but the record index."""
    cus = compute_units()
    case = MT.ohm_wide(cus)
    assert case.records > 2 * max(4 * 4, 32) * cus + 67
    got, paths = run_ohm(ctx, case)
    assert paths["ohm_wide_fragments"] == case.records < case.n and paths["ohm_headers_fused"] == 0 and paths["prefixed_chunks"] == 0, paths
    same(got, case.want()[1], case.label)
    sampled_datagrams_equal_the_model(case)


# ---------------------------------------------------------------- 4: DSD -> PCM
@pytest.mark.parametrize("route", ["fast", "plain"])
def test_dsd_pcm_every_workgroup_takes_several_tiles(ctx, route):
    """fast (dsd_pcm_table_kernel, `stage` reused behind the loop-top barrier): tiles > 3 x G x CUs + 37 with G = max(today's
    occupancy <= 2, floor(32 waves / 16 per workgroup) = 2); plain (dsd_pcm_kernel_v1, 1024 threads too): tiles > 2 x G x CUs + 37 with
    G = max(8 = today's cap at the launch site, floor(32 / 16) = 2 resident).  Tiles by the rule sum of ceil(n_frames / 512); one batch serves both (the model's arena is kept)."""
    cus = compute_units()
    case, tiles = MT.dsd_pcm(cus)
    assert tiles == int(((case.descs["n_frames"].astype(np.int64) + 511) // 512).sum()) > (3 * 2 * cus + 37 if route == "fast" else 2 * 8 * cus + 37)
    assert {int(v) for v in case.descs["out_frame0"]} == {0, 7, 1001} and int(case.descs["n_frames"].max()) == 512
    ctx.set_kernel_variant(0 if route == "fast" else 1)
    filt = d_src = d_dst = b = None
    try:
        filt = ctx.dsd_pcm_create(case.key[0], case.key[1], MT.DC.coef(case.key))
        d_src, d_dst = ctx.upload(case.src), ctx.malloc(case.dst_bytes)
        ctx.memset(d_dst, FILL, case.dst_bytes)
        b = ctx.dsd_pcm_batch(filt, case.descs, case.src.size, case.dst_bytes)
        n = case.descs.size
        assert ctx.dsd_pcm_batch_paths(b) == {"fast_descs": n if route == "fast" else 0, "plain_descs": 0 if route == "fast" else n, "launches": 1}
        ctx.dsd_pcm_run(b, d_src, d_dst)
        same(ctx.download(d_dst, case.dst_bytes), case.want(), f"{case.label} ({route})")
    finally:
        ctx.set_kernel_variant(0)
        if b is not None:
            ctx.batch_destroy(b)
        if d_src is not None:
            ctx.free(d_src)
            ctx.free(d_dst)
        if filt is not None:
            ctx.dsd_pcm_destroy(filt)


# ---------------------------------------------------------------- 5: the pulled resampler
@pytest.mark.parametrize("stereo_only,T", [(False, 32), (False, 64), (True, 32)], ids=["mixed-T32", "mixed-T64", "stereo-T32"])
def test_pulled_resampler_every_workgroup_takes_several_tiles(ctx, stereo_only, T):
    """src_pull_kernel<0> (mixed layouts) and <2> (stereo only): tiles > 3 x G x CUs + 37 with G = max(today's occupancy <= 8,
    floor(32 waves / 4 per workgroup) = 8) workgroups per CU; `win` is reused tile after tile, by another layout each time.  A tile
    never spans two messages, so the count of messages with frames is a lower bound of the tiles."""
    cus = compute_units()
    case = MT.pull(cus, stereo_only, T)
    assert int((case.descs["n_frames"] > 0).sum()) > 3 * 8 * cus + 37
    assert (set(case.descs["channels"].tolist()) == {2}) == stereo_only and int(case.descs["n_frames"].max()) == 256
    flt = ctx.src_pull_create(T, MT.PULL_S, case.table())
    d_src, d_dst = ctx.upload(case.src), ctx.malloc(case.dst_bytes)
    b = None
    try:
        ctx.memset(d_dst, FILL, case.dst_bytes)
        b = ctx.src_pull_batch(flt, case.descs, case.src.size, case.dst_bytes)
        ctx.src_pull_run(b, d_src, d_dst)
        same(ctx.download(d_dst, case.dst_bytes), case.want(capi.ramp_table()), case.label)
    finally:
        if b is not None:
            ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        ctx.src_pull_destroy(flt)


# ---------------------------------------------------------------- 6: the block resamplers' claim path
SRC_RUNS = [(name, variant, kernel) for name, (_, _, runs) in MT.SRC_CASES.items() for variant, kernel in runs]


@pytest.mark.parametrize("name,variant,kernel", SRC_RUNS, ids=[f"{n}-v{v}" for n, v, _ in SRC_RUNS])
def test_block_resamplers_claim_units_and_reset_their_counters(ctx, name, variant, kernel):
    """Units (ohgpu_src_batch_units) > 2 x 32 x CUs: the lean kernel starts CUs x <= 12 waves and the matrix kernel
    3 x CUs workgroups today, a CU keeps 32 waves, one unit per wave (workgroup) and trip -- so every wave takes its first unit by
    its index and CLAIMS the later ones with an atomic, and the grid's last wave zeroes the counters.  The batch runs TWICE into a
    re-filled destination: both outputs are the oracle's, the second only if the counters were left at zero."""
    cus = compute_units()
    case = MT.src_streams(cus, name)
    flt, _, _ = MT.SRC_CASES[name]
    L, M, coef = MT.src_filter(flt)
    ctx.set_kernel_variant(variant)
    h = b = d_src = d_dst = None
    try:
        h = ctx.src_create(L, M, flt[2], coef)
        b = ctx.src_batch(h, case.descs, case.src.size, case.dst_bytes)
        assert ctx.src_units(b)["units"] > 2 * 32 * cus, (ctx.src_units(b), case.n_streams)
        assert ctx.src_kernel_name(b) == kernel
        assert ctx.src_plan(b)["generic_pieces"] > 0
        d_src, d_dst = ctx.upload(case.src), ctx.malloc(case.dst_bytes)
        for turn in (1, 2):
            ctx.memset(d_dst, FILL, case.dst_bytes)
            ctx.src_run(b, d_src, d_dst)
            same(ctx.download(d_dst, case.dst_bytes), case.want(), f"{case.label}, variant {variant}, run {turn}")
    finally:
        ctx.set_kernel_variant(0)
        if b is not None:
            ctx.batch_destroy(b)
        if d_src is not None:
            ctx.free(d_src)
            ctx.free(d_dst)
        if h is not None:
            ctx.src_destroy(h)


# ---------------------------------------------------------------- 7: the FLAC scan's second attempt
@pytest.mark.parametrize("variant", [0, 1], ids=["tuned", "v1"])
def test_flac_scan_outgrows_its_first_list(ctx, variant):
    """Not a kernel loop but flac_run's second scan attempt: candidates (the model's count) >= 2 x (1.5 x (S / 512 + 256) + 32) for the
    arena's S source bytes -- twice the list flac_run sizes first (S / 512 + 256 entries asked for, half as much again plus 32
    handed out); should that sizing change, MT.flac_first_list changes with it.  Two runs: results equal field by field, arenas
    equal, and the second run allocates nothing (the longer list is kept)."""
    import flac_cases as FC
    from test_gpu_flac_textbook import Layout
    lay = Layout(list(MT.flac_cases()), seed=11)
    candidates = sum(FC.model(c)[0].candidates for c in lay.cases)
    assert candidates >= 2 * MT.flac_first_list(lay.src.size), (candidates, lay.src.size)
    ctx.set_kernel_variant(variant)
    try:
        lay.check(ctx, times=2)
    finally:
        ctx.set_kernel_variant(0)
    assert lay.allocs[1] == lay.allocs[0], lay.allocs
