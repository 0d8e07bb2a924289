"""What the block resamplers' GPU tests share (tests/test_gpu_src_textbook.py, tests/test_gpu_far_positions.py,
tests/test_gpu_far_offsets.py) and tests/test_far_cases.py checks without a device: the matrix of cells (kernel, variant, filter,
layout), the filters as the library designs them, the batch builder, the run that asserts the kernel a batch is planned onto, and
the model's bytes (tests/src_textbook.py).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import src_textbook as TB
from ohpipeline_amd import capi

LE, BE = capi.ENDIAN_LITTLE, capi.ENDIAN_BIG
kMax = capi.RAMP_MAX
RAMPS = [(kMax, 0), (0, kMax), (kMax, 8192), (8191, 8190), (5, 5), (kMax, kMax), (0, 0), (12345, 54), (17, 16001)]   # test_gpu_parity.RAMPS
FILL = 0xA5
F44, F96, F48, F32 = (44100, 48000, 32), (96000, 48000, 64), (48000, 44100, 32), (32000, 48000, 16)
WG, LEAN, BLOCK, V1 = "src_mfma_wg_kernel", "src_lean_kernel", "src_block_kernel", "src_kernel_v1"

# layouts: (channels, source bits, source byte order, destination bits, destination byte order, planar source)
S24 = (2, 24, LE, 24, BE, False)
WG_LAYOUTS = [(F44, S24), (F44, (6, 24, LE, 24, BE, False)), (F44, (8, 24, LE, 24, BE, False)), (F96, S24),
              (F96, (8, 24, LE, 24, BE, False)), (F44, (2, 16, LE, 24, BE, False)), (F44, (2, 16, BE, 24, BE, True)),
              (F44, (2, 24, BE, 24, BE, True))]
LEAN_ONLY_LAYOUTS = [(F44, (1, 16, LE, 24, BE, False)), (F44, (2, 32, LE, 24, BE, False)), (F44, (5, 24, LE, 24, BE, False)),
                     (F44, (2, 24, LE, 16, BE, False)), (F44, (2, 24, LE, 32, BE, False))]
BLOCK_LAYOUTS = [(F48, (2, 24, LE, 24, BE, False)), (F48, (2, 24, LE, 24, LE, False)), (F48, (2, 24, BE, 24, BE, False)),
                 (F48, (2, 16, LE, 24, BE, False)), (F48, (2, 16, BE, 24, BE, False))]     # OHGPU_BLOCK_FALLBACK_KERNELS
# (kernel, the variant the batch is created and run under, filter, layout)
CELLS = ([(WG, 0, f, lay) for f, lay in WG_LAYOUTS] + [(LEAN, 4, f, lay) for f, lay in WG_LAYOUTS + LEAN_ONLY_LAYOUTS] +
         [(BLOCK, 0, f, lay) for f, lay in BLOCK_LAYOUTS] +
         [(V1, 1, F44, S24), (V1, 0, F44, (2, 24, LE, 8, BE, False)), (V1, 0, F32, (8, 24, LE, 24, BE, False))])


def layout_id(lay):
    ch, sb, se, db, de, planar = lay
    return f"{ch}ch-{'planar' if planar else ('le' if se == LE else 'be')}{sb}-{'le' if de == LE else 'be'}{db}"


def cell_id(c):
    kernel, variant, (rin, rout, T, *_), lay = c
    return f"{kernel[4:].replace('_kernel', '')}-v{variant}-{rin // 100}to{rout // 100}x{T}-{layout_id(lay)}"


def phase_sum(coef, L, T):
    """The largest per-phase sum |c| (ohgpu_src::max_sum_abs): which block kernel a filter gets."""
    return int(np.abs(np.asarray(coef, dtype=np.int64).reshape(L, T)).sum(axis=1).max())


LEAN_SUMS, ROUND1_SUMS = (0, 1 << 29), (1 << 29, 1 << 30)       # [lo, hi): the lean kernel's rounding bias; round 1's kernel, the fallback


def steered(coef, L, T, sums):
    """The table as it is if its sum |c| lies in `sums`, else times k/4 (floored), k from the table's own sum: 3/4 or 1/2 to go
    down, the smallest k/4 above 1 to go up.  A scaled filter is still a filter, and the model takes the same table."""
    lo, hi = sums
    if lo <= phase_sum(coef, L, T) < hi:
        return coef
    for k in ((3, 2) if phase_sum(coef, L, T) >= hi else range(5, 9)):
        scaled = ((coef.astype(np.int64) * k) // 4).astype(np.int32)
        if lo <= phase_sum(scaled, L, T) < hi:
            return scaled
    raise AssertionError(f"no k/4 takes sum |c| = {phase_sum(coef, L, T)} into [{lo}, {hi})")


class Filter:
    """capi.src_design's table at Kaiser(9) and pass edge f_pass -- `sums` given: steered into that bracket of sum |c|."""

    def __init__(self, ctx, rin, rout, T, f_pass=20000.0, sums=None):
        self.rin, self.rout, self.T = rin, rout, T
        self.L, self.M, self.coef = capi.src_design(rin, rout, T, 9.0, f_pass)
        if sums is not None:
            self.coef = steered(self.coef, self.L, T, sums)
            assert sums[0] <= phase_sum(self.coef, self.L, T) < sums[1]
        # a half-band 2:1 decimator, from the table's zeros as ohgpu_src_create finds it (csrc/api_src.hip, src_describe)
        self.halfband = (self.L, self.M, T) == (1, 2, 64) and self.coef[T - 1] == 0 and \
            not any(self.coef[k] for k in range(1, T, 2) if k != T // 2 - 1)
        self.handle = ctx.src_create(self.L, self.M, T, self.coef)


class Batch:
    """Streams of one or more layouts in one source arena (a planar stream: its planes, 5 frames apart), their messages' outputs
    in one destination arena, each stream's contiguous, a few bytes between streams."""

    def __init__(self):
        self.src = bytearray()
        self.rows = []
        self.dst = 0
        self.streams = []

    def add_stream(self, y, lay, rng, first=0):
        """y: source-unit samples of input frames first .. first + len(y) - 1 (the stream's buffer).  Returns the stream's index."""
        ch, sb, se, db, de, planar = lay
        stride = (y.shape[0] + 5) * 4 if planar else None
        off = len(self.src)
        self.src += bytes(TB.encode(y, sb, se, rng, stride))
        self.src += bytes((-len(self.src)) % 16)
        self.dst += 3
        self.streams.append(dict(off=off, first=first, frames=y.shape[0], stride=stride or 0, lay=lay, dst0=self.dst, out0=None))
        return len(self.streams) - 1

    def add_msg(self, s, out0, n, flags=0, ramp=(kMax, kMax)):
        """Message [out0, out0 + n) of stream s; a stream's messages must come in output order (their bytes are back to back)."""
        st = self.streams[s]
        ch, sb, se, db, de, planar = st["lay"]
        if st["out0"] is None:
            st["out0"] = out0
        dst = st["dst0"] + (out0 - st["out0"]) * ch * db // 8
        self.rows.append((st["off"], st["first"], st["frames"], out0, dst, n, ramp[0], ramp[1], 256, ch, sb, se, db, de,
                          flags | (capi.FLAG_SRC_PLANAR32 if planar else 0), st["stride"]))
        self.dst = max(self.dst, dst + n * ch * db // 8)

    def descs(self):
        return np.array(self.rows, dtype=capi.SRC_MSG_DESC)

    def arena(self):
        return np.frombuffer(bytes(self.src), dtype=np.uint8).copy()


def model(flt, descs, src, dst_bytes, ramp_table):
    return TB.batch_bytes(flt.coef, flt.L, flt.M, flt.T, descs, src, dst_bytes, ramp_table, FILL)


def assert_same(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[:8]}"


def run(ctx, flt, variant, kernel, descs, src, dst_bytes):
    """Create the batch under `variant`, assert the kernel it runs on, run it once: (bytes, plan)."""
    ctx.set_kernel_variant(variant)
    try:
        b = ctx.src_batch(flt.handle, descs, src.size, dst_bytes)
        try:
            assert ctx.src_kernel_name(b) == kernel
            plan = ctx.src_plan(b)
            d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
            try:
                ctx.memset(d_dst, FILL, dst_bytes)
                ctx.src_run(b, d_src, d_dst)
                got = ctx.download(d_dst, dst_bytes)
            finally:
                ctx.free(d_src)
                ctx.free(d_dst)
        finally:
            ctx.batch_destroy(b)
    finally:
        ctx.set_kernel_variant(0)
    return got, plan


def block_of(ctx, flt, lay, variant):
    """(outputs, inputs) of the cell's blocks (ohgpu_src_batch_block on a probe batch); a plan without blocks: the filter's period
    times what makes some 160 outputs."""
    probe = Batch()
    s = probe.add_stream(np.zeros((30000, lay[0]), dtype=np.int64), lay, None)
    end = min(TB.out_frames(flt.L, flt.M, 30000), 24000)
    for m in range(0, end, 4000):
        probe.add_msg(s, m, min(4000, end - m))
    ctx.set_kernel_variant(variant)
    try:
        b = ctx.src_batch(flt.handle, probe.descs(), len(probe.src), probe.dst)
        try:
            return ctx.src_batch_block(b)
        except capi.OhGpuError as e:
            assert e.code == capi.ERR_UNSUPPORTED
            k = -(-160 // flt.L)
            return k * flt.L, k * flt.M
        finally:
            ctx.batch_destroy(b)
    finally:
        ctx.set_kernel_variant(0)


def full_scale(bits):
    return -(1 << (min(bits, 24) - 1)), (1 << (min(bits, 24) - 1)) - 1


def one_stream(flt, lay, y, rng, msg=240, ramp_every=4):
    """One stream from its start, every output the input allows, in messages of `msg` frames (the last ragged); every
    ramp_every-th message ramped with the next of RAMPS, every fifth ZERO_LSB32."""
    b = Batch()
    s = b.add_stream(y, lay, rng)
    n_out = TB.out_frames(flt.L, flt.M, y.shape[0])
    for i, m in enumerate(range(0, n_out, msg)):
        ramped = ramp_every and i % ramp_every == ramp_every - 1
        b.add_msg(s, m, min(msg, n_out - m), (capi.FLAG_RAMP if ramped else 0) | (capi.FLAG_ZERO_LSB32 if i % 5 == 4 else 0),
                  RAMPS[i % len(RAMPS)] if ramped else (kMax, kMax))
    return b, n_out


# ------------------------------------------------------------------------------------------ far stream positions
FAR_NEAR_OUT = 4096                                     # a far stream's near twin starts within a period (L outputs, M inputs) of this output
FAR_MSGS = (1, 5, 43, 220, 239, 241, 700)               # message sizes in turn, as check_cell's ragged streams
FAR_LIMIT = 1 << 48                                     # the last out_frame0 and src_frame0 the creation admits


def far_anchors(L, M):
    """label -> (what, value): where a far stream sits.  'out': output frame `value` lies strictly inside the stream's fourth message
    (220 frames); 'last': the last message's out_frame0 is `value` (an interpolator: its outputs run ahead of its inputs); 'first':
    the buffer's first frame src_frame0 is `value` (a decimator: its inputs run ahead)."""
    limit = ("last", FAR_LIMIT) if L >= M else ("first", FAR_LIMIT)
    return {"out_2p31": ("out", 1 << 31), "out_2p32": ("out", 1 << 32), "in_2p32": ("in", 1 << 32), "limit": limit}


def far_stream(L, M, T, lay, anchor, far, n_out=3300, seed=1):
    """(Batch, message sizes): one stream mid-stream, n_out outputs in ragged messages (RAMPS on two in three, ZERO_LSB32 on one in
    four), its buffer holding just the frames they read plus a few.  far: placed by `anchor` (far_anchors); else the same stream k
    whole periods earlier -- out_frame0 down by k * L, src_frame0 by k * M, every byte of the arenas and every other field the same:
    the operation is invariant under that shift, so the model's bytes are too."""
    what, value = anchor
    sizes, i = [], 0
    while sum(sizes) < n_out:
        sizes.append(min(FAR_MSGS[i % 7], n_out - sum(sizes)))
        i += 1
    slack = T + 24
    if what == "out":
        m0 = value - sum(sizes[:3]) - sizes[3] // 2
    elif what == "in":                                  # the input frame `value` is read in the middle of the fourth message
        m0 = -(-value * L // M) - sum(sizes[:3]) - sizes[3] // 2
    elif what == "last":
        m0 = value - sum(sizes[:-1])
    else:
        m0 = -(-(value + slack) * L // M)
    f0 = value if what == "first" else (m0 * M) // L - slack
    frames = ((m0 + n_out - 1) * M) // L - f0 + 1 + 7
    k = (m0 - FAR_NEAR_OUT) // L
    if not far:
        m0, f0 = m0 - k * L, f0 - k * M
    assert f0 > T and (m0 * M) // L - f0 >= T
    rng = np.random.default_rng(seed)
    lo, hi = full_scale(lay[1])
    b = Batch()
    s = b.add_stream(rng.integers(lo, hi + 1, size=(frames, lay[0])), lay, rng, first=f0)
    m = m0
    for i, n in enumerate(sizes):
        b.add_msg(s, m, n, (capi.FLAG_RAMP if i % 3 else 0) | (capi.FLAG_ZERO_LSB32 if i % 4 == 1 else 0), RAMPS[i % len(RAMPS)])
        m += n
    return b, sizes
