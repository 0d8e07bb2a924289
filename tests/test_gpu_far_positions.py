"""Stream positions past 2^31, past 2^32 and at the ABI's limits, on the device: the block resamplers (src_frame0, out_frame0 up to
2^48), the pulled resampler (pos_frame up to 2^48, a pos_frac that carries), DSD -> PCM on both routes (out_frame0 up to 2^40, the
stream's bit, byte and chunk index past 2^32) and the FLAC decoder (first_sample, coded numbers of every length).  Small arenas, as
in the textbook tests; only the positions are far.

These operations are invariant under a shift of the stream's positions by whole periods, so a far case has a near twin: the same
arenas, the same layout, positions a few thousand frames in.  The model (tests/src_textbook.py, tests/src_pull_model.py,
tests/dsd_pcm_textbook.py) is run on both -- the two must agree, which tests/test_far_cases.py pins without a device -- and the
device's bytes for the far descriptors must equal them: whole destination arenas, zero differing bytes."""
import numpy as np
import pytest

import dsd_pcm_cases as DC
import dsd_pcm_textbook as DP
import flac_cases as FC
import src_cases as SC
import src_pull_cases as PC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ramp_table():
    return capi.ramp_table()


# ---------------------------------------------------------------- the block resamplers
@pytest.fixture(scope="module")
def filters(ctx):
    made = {}

    def get(f):
        if f not in made:
            made[f] = SC.Filter(ctx, *f)
        return made[f]
    yield get
    for f in made.values():
        ctx.src_destroy(f.handle)


SRC_CELLS = [(SC.WG, 0, SC.F44, SC.S24), (SC.WG, 0, SC.F96, SC.S24), (SC.LEAN, 4, SC.F44, SC.S24), (SC.BLOCK, 0, SC.F48, SC.S24),
             (SC.V1, 1, SC.F44, SC.S24)]
ANCHORS = ("out_2p31", "out_2p32", "in_2p32", "limit")


@pytest.mark.parametrize("label", ANCHORS)
@pytest.mark.parametrize("cell", SRC_CELLS, ids=[SC.cell_id(c) for c in SRC_CELLS])
def test_src_far_stream(ctx, filters, ramp_table, cell, label):
    """One stream of six blocks mid-stream in ragged, ramped messages: out_frame0 passes 2^31 and 2^32 inside a message, the input
    frame read passes 2^32 inside one, and the stream ends at the last position the creation admits (out_frame0 = 2^48 for an
    interpolator, src_frame0 = 2^48 for a decimator)."""
    kernel, variant, f, lay = cell
    flt = filters(f)
    L_blk, _ = SC.block_of(ctx, flt, lay, variant)
    anchor = SC.far_anchors(flt.L, flt.M)[label]
    n_out = max(6 * L_blk + 50, 3300)
    near, sizes = SC.far_stream(flt.L, flt.M, flt.T, lay, anchor, False, n_out)
    far, _ = SC.far_stream(flt.L, flt.M, flt.T, lay, anchor, True, n_out)
    dn, df = near.descs(), far.descs()
    assert bytes(near.src) == bytes(far.src) and near.dst == far.dst
    lo, hi = df["out_frame0"].astype(object), df["out_frame0"].astype(object) + df["n_frames"] - 1
    if anchor[0] == "out":
        assert ((lo < anchor[1]) & (anchor[1] < hi)).sum() == 1                # strictly inside one message
    elif anchor[0] == "last":
        assert int(df["out_frame0"][-1]) == SC.FAR_LIMIT
    elif anchor[0] == "first":
        assert int(df["src_frame0"][0]) == SC.FAR_LIMIT
    want = SC.model(flt, dn, near.arena(), near.dst, ramp_table)
    assert np.array_equal(SC.model(flt, df, far.arena(), far.dst, ramp_table), want)
    for what, b, descs in (("near", near, dn), ("far", far, df)):
        got, plan = SC.run(ctx, flt, variant, kernel, descs, b.arena(), b.dst)
        SC.assert_same(got, want, f"{label} {what}")
        assert kernel == SC.V1 or (plan["block_kernel_out_frames"] >= 4 * L_blk and plan["generic_pieces"] > 0), plan


@pytest.mark.parametrize("cell", SRC_CELLS[:4], ids=[SC.cell_id(c) for c in SRC_CELLS[:4]])
def test_src_advance_across_2p32(ctx, filters, ramp_table, cell):
    """A period of whole blocks that ends just below out_frame0 = 2^32, then ohgpu_src_batch_advance by the period: the second
    period starts below 2^32 and ends above it.  Both against the model on that period's descriptors, and against the near twin."""
    kernel, variant, f, lay = cell
    flt = filters(f)
    L_blk, M_blk = SC.block_of(ctx, flt, lay, variant)
    blocks = max(3, -(-2000 // L_blk))
    head, tail, hist = 37, 13, M_blk + flt.T
    rng = np.random.default_rng(48)
    lo, hi = SC.full_scale(lay[1])
    whole = rng.integers(lo, hi + 1, size=(3 * blocks * M_blk + hist, lay[0]))

    def make(first_block, period):
        b = SC.Batch()
        y = whole[period * blocks * M_blk:(period + 1) * blocks * M_blk + hist]
        s = b.add_stream(y, lay, None, first=first_block * M_blk - hist)
        m, end, i = first_block * L_blk + head, (first_block + blocks) * L_blk - tail, 0
        while m < end:
            n = min(240, end - m)
            b.add_msg(s, m, n, capi.FLAG_RAMP if i % 7 < 2 else 0, (SC.kMax, 2000) if i % 7 < 2 else (SC.kMax, SC.kMax))
            m, i = m + n, i + 1
        return b.descs(), b.arena(), b.dst

    at = (1 << 32) // L_blk - blocks - blocks // 2           # period 0 ends below 2^32, period 1 holds it
    near_at = 8
    d0, a0, dst_bytes = make(at, 0)
    d1, a1, _ = make(at + blocks, 1)
    assert int(d0["out_frame0"].max()) + 240 < 1 << 32 and int(d1["out_frame0"].min()) < 1 << 32 < int(d1["out_frame0"].max())
    wants = [SC.model(flt, d, a, dst_bytes, ramp_table) for d, a in ((d0, a0), (d1, a1))]
    for k, first in enumerate((near_at, near_at + blocks)):
        d, a, _ = make(first, k)
        assert np.array_equal(a, (a0, a1)[k]) and np.array_equal(SC.model(flt, d, a, dst_bytes, ramp_table), wants[k])
    b = d_src = d_dst = None
    try:
        ctx.set_kernel_variant(variant)
        b = ctx.src_batch(flt.handle, d0, a0.size, dst_bytes)
        assert ctx.src_kernel_name(b) == kernel
        d_src, d_dst = ctx.upload(a0), ctx.malloc(dst_bytes)
        for k, arena in enumerate((a0, a1)):
            if k:
                ctx.src_batch_advance(b, blocks)
                ctx.copy_h2d(d_src, arena)
            ctx.memset(d_dst, SC.FILL, dst_bytes)
            ctx.src_run(b, d_src, d_dst)
            SC.assert_same(ctx.download(d_dst, dst_bytes), wants[k], f"period {k}")
    finally:
        ctx.set_kernel_variant(0)
        if b is not None:
            ctx.batch_destroy(b)
        if d_src is not None:
            ctx.free(d_src)
            ctx.free(d_dst)


# ---------------------------------------------------------------- the pulled resampler
@pytest.mark.parametrize("T", [32, 64])
def test_src_pull_far_positions(ctx, ramp_table, T):
    """pos_frame passing 2^31 and 2^32 inside a message, a window that begins below 2^32 under a pos_frame above it, streams that
    end just below pos_frame = 2^48 and one message at 2^48 itself; every stream entered at pos_frac = 2^32 - 5, so that the first
    step carries into the frame; stereo (the stereo kernel cannot be told apart here: the batch is mixed) and five channels."""
    table = capi.src_pull_design(44100, 48000, T, PC.S, 8.0 if T == 32 else 9.0, 20000.0, 0.001)
    flt = ctx.src_pull_create(T, PC.S, table)
    try:
        (near, _), (far, labels) = PC.far_streams(T, False), PC.far_streams(T, True)
        src, dn = near.arrays()
        src_far, df = far.arrays()
        assert np.array_equal(src, src_far) and near.dst_bytes == far.dst_bytes
        assert int(df["pos_frame"].max()) == 1 << 48 and int(df["pos_frac"][0]) + int(df["step"][0]) >= 1 << 32
        want = PC.expected(table, dn, src, near.dst_bytes, ramp_table)
        assert np.array_equal(PC.expected(table, df, src, far.dst_bytes, ramp_table), want)
        for what, descs in (("near", dn), ("far", df)):
            d_src, d_dst = ctx.upload(src), ctx.malloc(near.dst_bytes)
            b = ctx.src_pull_batch(flt, descs, src.size, near.dst_bytes)
            try:
                ctx.memset(d_dst, 0, near.dst_bytes)
                ctx.src_pull_run(b, d_src, d_dst)
                got = ctx.download(d_dst, near.dst_bytes)
            finally:
                ctx.batch_destroy(b)
                ctx.free(d_src)
                ctx.free(d_dst)
            for d, label in zip(descs, labels):
                lo, n = int(d["dst_offset"]), int(d["n_frames"]) * int(d["channels"]) * 3
                assert np.array_equal(got[lo:lo + n], want[lo:lo + n]), f"{what} {label}"
    finally:
        ctx.src_pull_destroy(flt)


@pytest.mark.parametrize("ch", [2, 5])
def test_src_pull_stereo_and_any_channel_kernels_far(ctx, ramp_table, ch):
    """The same far streams a channel count at a time: a batch of stereo messages alone runs the stereo instantiation."""
    T = 32
    table = capi.src_pull_design(44100, 48000, T, PC.S, 8.0, 20000.0, 0.001)
    flt = ctx.src_pull_create(T, PC.S, table)
    try:
        (near, _), (far, _) = PC.far_streams(T, False), PC.far_streams(T, True)
        src, dn = near.arrays()
        _, df = far.arrays()
        keep = df["channels"] == ch
        want = PC.expected(table, dn[keep], src, near.dst_bytes, ramp_table)
        d_src, d_dst = ctx.upload(src), ctx.malloc(near.dst_bytes)
        b = ctx.src_pull_batch(flt, df[keep], src.size, near.dst_bytes)
        try:
            ctx.memset(d_dst, 0, near.dst_bytes)
            ctx.src_pull_run(b, d_src, d_dst)
            assert np.array_equal(ctx.download(d_dst, near.dst_bytes), want)
        finally:
            ctx.batch_destroy(b)
            ctx.free(d_src)
            ctx.free(d_dst)
    finally:
        ctx.src_pull_destroy(flt)


# ---------------------------------------------------------------- DSD -> PCM
@pytest.mark.parametrize("variant", [0, 1], ids=["fast", "plain"])
@pytest.mark.parametrize("key", list(DC.DESIGNS), ids=[f"D{D}T{T}" for D, T in DC.DESIGNS])
def test_dsd_pcm_far_positions(ctx, key, variant):
    """tests/dsd_pcm_cases.positions: the bit, byte and chunk index of the stream passing 2^32 inside a tile, out_frame0 passing 2^31
    and 2^32, the last frames below 2^40 and the one frame at out_frame0 = 2^40 -- on the route asserted."""
    near, far = DC.positions(key, False), DC.positions(key, True)
    assert np.array_equal(near.src, far.src) and near.dst_bytes == far.dst_bytes and int(far.descs["out_frame0"].max()) == 1 << 40
    want = near.want()
    assert np.array_equal(far.want(), want)
    filt = ctx.dsd_pcm_create(key[0], key[1], DC.coef(key))
    ctx.set_kernel_variant(variant)
    try:
        for case in (near, far):
            d_src, d_dst = ctx.upload(case.src), ctx.malloc(case.dst_bytes)
            b = ctx.dsd_pcm_batch(filt, case.descs, case.src.size, case.dst_bytes)
            try:
                n = case.descs.size
                assert ctx.dsd_pcm_batch_paths(b) == {"fast_descs": 0 if variant else n, "plain_descs": n if variant else 0, "launches": 1}
                assert ctx.batch_info(b) == DP.totals(case.descs, *key)
                ctx.memset(d_dst, DC.FILL, case.dst_bytes)
                ctx.dsd_pcm_run(b, d_src, d_dst)
                bad = np.flatnonzero(ctx.download(d_dst, case.dst_bytes) != want)
                assert bad.size == 0, f"{case.label}: {bad.size} differing bytes, first at {bad[:6].tolist()}"
            finally:
                ctx.batch_destroy(b)
                ctx.free(d_src)
                ctx.free(d_dst)
    finally:
        ctx.set_kernel_variant(0)
        ctx.dsd_pcm_destroy(filt)


# ---------------------------------------------------------------- FLAC
FAR_FLAC = [n for n in FC.fixture_names() if n.startswith(("fixed_from_frame_", "variable_from_"))]


@pytest.mark.parametrize("variant", [0, 1], ids=["tuned", "v1"])
@pytest.mark.parametrize("packed", [False, True], ids=["planes", "packed_be"])
def test_flac_far_first_samples(ctx, variant, packed):
    """The eight streams of far positions in one batch, each whole at its own first_sample (up to 2^36 - 48; coded numbers of 1 to
    7 bytes): results, the whole arena, and every delivered frame's 64-bit first_sample against the model's."""
    assert len(FAR_FLAC) == 8
    cases = [FC.whole(FC.fixture(n), packed) for n in FAR_FLAC]
    assert max(c.first_sample for c in cases) == (1 << 36) - 48 and sum(c.first_sample >= 1 << 32 for c in cases) >= 2
    lay = FC.Layout(cases, seed=11)
    ctx.set_kernel_variant(variant)
    d_src, d_dst = ctx.upload(lay.src), ctx.upload(lay.dst0)
    b = ctx.flac_batch(lay.descs, lay.src.size, lay.dst0.size)
    try:
        ctx.flac_run(b, d_src, d_dst)
        res, frames = ctx.flac_results(b, len(cases)), ctx.flac_frames(b)
        got = ctx.download(d_dst, lay.dst0.size)
    finally:
        ctx.set_kernel_variant(0)
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    want_frames = []
    for i, c in enumerate(cases):
        model = FC.model(c)[0]
        r = res[i]
        mine = (int(r["status"]), int(r["frames"]), int(r["samples"]), int(r["first_sample_decoded"]), int(r["bytes_consumed"]),
                int(r["candidates"]), int(r["candidates_rejected"]))
        assert mine == FC.result_tuple(model) and mine[:4] == (capi.FLAC_OK, 3, 48, c.first_sample), (c.label, mine)
        want_frames += [(i, f.header.blocksize, c.first_sample + place) for f, place in zip(model.frames, model.places)]
    assert [(int(f["stream"]), int(f["blocksize"]), int(f["first_sample"])) for f in frames] == want_frames
    assert np.array_equal(got, lay.want)
