"""The shell every batch family of the C ABI shares (include/ohgpu.h), pinned family by family: what a failed create leaves behind,
what a run refuses (another family's batch, null arenas) and what it accepts (an empty batch, a batch that reads no source), that
the host-buffer calls equal create + run on device arenas and count what they move, and that a batch with per-launch device state
runs one launch at a time.  The family tests (test_gpu_*_textbook.py) check WHAT each family computes; they touch this shell only
in passing.  Every expectation here was first observed on the library as it was before the C ABI was split by family
(csrc/api_*.hip, csrc/api_common.h): the file pins that behaviour, not the split.

The batches are the smallest valid ones of each family:

    pcm        2 messages x 16 frames, stereo S16LE -> S24BE
    fmt        2 x 16 frames, stereo unpack-planar
    dsd        2 descriptors of one whole sample block each (raw, 6-word blocks, 2 pad bytes a chunk)
    flywheel   1 request, 1 channel, 4 training samples at 44.1 kHz: the least the validator admits
    src        44.1 -> 48 kHz, T = 32, stereo S24: two messages of 160 outputs (whole blocks: a plan, its slab and unit counters)
               and one of 16 (the generic kernel's remainder)
    src_pull   2 x 16 frames
    ohm        1 stream, 1 frame, 1 fragment of 16 frames
    flac       tests/golden/flac_decode/tiny_s16_stereo_44k1_b16.flac

Where the table's batch has ONE output (flywheel, ohm, flac) the host-buffer test takes two of them: adjacent outputs and outputs
with a hole between them are its two cases."""
import ctypes as C

import numpy as np
import pytest

import flac_cases as FC
import src_pull_model as PM
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

HOLE = 64
DEV_FILL, HOST_FILL = 0xA5, 0x5A
ZERO_INFO = {"n_msgs": 0, "in_frames": 0, "out_frames": 0, "src_bytes_touched": 0, "dst_bytes_written": 0}
FAMILIES = ("pcm", "fmt", "dsd", "flywheel", "src", "src_pull", "ohm", "flac")
# family -> (noun of "not a <noun> batch", has a host-buffer call, runs without a source arena when it reads none, one launch at a time)
NOUN = {"pcm": "pcm", "fmt": "fmt", "dsd": "DSD", "flywheel": "flywheel", "src": "src", "src_pull": "pulled", "ohm": "Songcast frame", "flac": "FLAC"}
HAS_HOST = {"pcm", "dsd", "flywheel", "src", "src_pull", "ohm", "flac"}
# what last_error says of the last descriptor when its destination lies past the arena
BOUNDS_TEXT = {"pcm": "desc 1: writes [", "fmt": "fmt desc 1: writes up to", "dsd": "dsd desc 1: writes [", "flywheel": "flywheel desc 0: writes up to",
               "src": "src desc 2: writes [", "src_pull": "src pull desc 1: writes [", "ohm": "ohm frame 0: writes [", "flac": "flac desc 0: writes ["}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class Case:
    """One batch: `head` = the create call's arguments between the context and the arena sizes, the source arena, the
    destination arena's size, and the (dst_offset, bytes) of every output."""

    def __init__(self, family, head, keep, src, dst_bytes, ranges):
        self.family, self.head, self.keep, self.src, self.dst_bytes, self.ranges = family, head, keep, src, dst_bytes, ranges


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _offsets(sizes, hole):
    """Outputs back to back, `hole` bytes between the first and the second."""
    at, out = 0, []
    for k, s in enumerate(sizes):
        out.append(at)
        at += s + (hole if k == 0 and len(sizes) > 1 else 0)
    return out, at


class Fixtures:
    def __init__(self):
        self.ctx = capi.Context(0)
        self.L, self.M, coef = capi.src_design(44100, 48000, 32, 9.0, 20000.0)
        self.src_filter = self.ctx.src_create(self.L, self.M, 32, coef)
        table = capi.src_pull_design(44100, 48000, 32, 8, 8.0, 20000.0, 0.001)
        self.pull_filter = self.ctx.src_pull_create(32, 8, table)
        self.tiny = FC.fixture("tiny_s16_stereo_44k1_b16")

    def close(self):
        self.ctx.src_destroy(self.src_filter)
        self.ctx.src_pull_destroy(self.pull_filter)
        self.ctx.close()

    # ---- the families' smallest batches.  hole: bytes between the first output and the second; outputs: how many descriptors
    # (None: the table's); bad: the last descriptor's destination starts where the arena ends; silent: no source byte is read
    def case(self, family, hole=0, outputs=None, bad=False, silent=False, empty=False):
        c = getattr(self, "_" + family)(hole, outputs, silent, empty)
        if bad:
            last = c.keep[-1]                       # the array that carries the destination offsets
            last["dst_offset"][-1] = c.dst_bytes
        return c

    def _pcm(self, hole, outputs, silent, empty):
        n = 0 if empty else (outputs or 2)
        offs, dst_bytes = _offsets([96] * n, hole)
        d = np.zeros(n, dtype=capi.MSG_DESC)
        for i in range(n):
            d[i] = (64 * i, offs[i], 16, 0, 0, capi.UNITY_ATTENUATION, 2, 16, capi.ENDIAN_LITTLE, 24, capi.ENDIAN_BIG, capi.FLAG_SILENCE if silent else 0)
        return Case("pcm", (_ptr(d), n), [d], _noise(64 * n, 1), dst_bytes, [(o, 96) for o in offs])

    def _fmt(self, hole, outputs, silent, empty):
        n = 0 if empty else (outputs or 2)
        offs, dst_bytes = _offsets([128] * n, hole)
        d = np.zeros(n, dtype=capi.FMT_DESC)
        for i in range(n):
            d[i] = (64 * i, offs[i], 0, 64, 16, capi.FMT_UNPACK_PLANAR, 2, 16, 32, [0] * 8)
        return Case("fmt", (_ptr(d), n), [d], _noise(64 * n, 2), dst_bytes, [(o, 128) for o in offs])

    def _dsd(self, hole, outputs, silent, empty):
        n = 0 if empty else (outputs or 2)
        src_each, dst_each = capi.dsd_layout(capi.DSD_RAW, 6, 2, 4)
        assert (src_each, dst_each) == (16, 24)
        offs, dst_bytes = _offsets([dst_each] * n, hole)
        d = np.zeros(n, dtype=capi.DSD_DESC)
        for i in range(n):
            d[i] = (src_each * i, offs[i], 4, capi.DSD_RAW, capi.DSD_FLAG_SILENCE if silent else 0, 6, 2, [0] * 8)
        return Case("dsd", (_ptr(d), n), [d], _noise(src_each * n, 3), dst_bytes, [(o, dst_each) for o in offs])

    def _flywheel(self, hole, outputs, silent, empty):
        n = 0 if empty else (outputs or 1)
        offs, dst_bytes = _offsets([64] * n, hole)
        d = np.zeros(n, dtype=capi.FLYWHEEL_DESC)
        for i in range(n):
            d[i] = (16 * i, 16, offs[i], 4, 16, 16, 44100, 1, 0)
        train = (np.array([1000, -2000, 3000, -500] * n, dtype=np.int64) << 16).astype(">i4").view(np.uint8)
        return Case("flywheel", (_ptr(d), n), [d], train.copy(), dst_bytes, [(o, 64) for o in offs])

    def _src(self, hole, outputs, silent, empty):
        frames = [] if empty else [160, 160, 16]
        offs, dst_bytes = _offsets([f * 6 for f in frames], hole)
        d = np.zeros(len(frames), dtype=capi.SRC_MSG_DESC)
        out0 = 0
        for i, f in enumerate(frames):      # one stream from its first frame on; every message's window is the whole 320-frame buffer
            d[i] = (0, 0, 320, out0, offs[i], f, 0, 0, capi.UNITY_ATTENUATION, 2, 24, capi.ENDIAN_LITTLE, 24, capi.ENDIAN_BIG, 0, 0)
            out0 += f
        return Case("src", (self.src_filter, _ptr(d), len(frames)), [d], _noise(320 * 6 if frames else 0, 4), dst_bytes, [(o, f * 6) for o, f in zip(offs, frames)])

    def _src_pull(self, hole, outputs, silent, empty):
        n = 0 if empty else (outputs or 2)
        offs, dst_bytes = _offsets([96] * n, hole)
        step = capi.src_pull_step(44100, 48000)
        d = np.zeros(n, dtype=capi.SRC_PULL_MSG_DESC)
        pos, frac, need = 0, 0, 0
        for i in range(n):
            first, count = capi.src_pull_window(pos, frac, step, 16, 32)
            d[i]["src_offset"], d[i]["src_frame0"], d[i]["src_frames"] = first * 6, first, count
            d[i]["pos_frame"], d[i]["pos_frac"], d[i]["step"], d[i]["n_frames"], d[i]["dst_offset"] = pos, frac, step, 16, offs[i]
            d[i]["attenuation"], d[i]["channels"], d[i]["src_bits"], d[i]["src_endian"] = capi.UNITY_ATTENUATION, 2, 24, capi.ENDIAN_LITTLE
            d[i]["dst_bits"], d[i]["dst_endian"] = 24, capi.ENDIAN_BIG
            need = max(need, (first + count) * 6)
            pos, frac = PM.advance(pos, frac, step, 16)
        return Case("src_pull", (self.pull_filter, _ptr(d), n), [d], _noise(need, 5), dst_bytes, [(o, 96) for o in offs])

    def _ohm(self, hole, outputs, silent, empty):
        n = 0 if empty else (outputs or 1)
        st = np.zeros(0 if empty else 1, dtype=capi.OHM_STREAM)
        if not empty:
            st["sample_rate"], st["bit_rate"], st["src_channels"], st["src_bits"], st["src_endian"] = 44100, 44100 * 32, 2, 16, capi.ENDIAN_BIG
            st["codec_bytes"], st["codec"][0, :3] = 3, np.frombuffer(b"PCM", dtype=np.uint8)
        header, total = C.c_uint32(0), C.c_uint32(0)
        if not empty:
            capi.check(capi.lib().ohgpu_ohm_frame_layout(_ptr(st), 16, C.byref(header), C.byref(total)))
        offs, dst_bytes = _offsets([total.value] * n, hole)
        fg = np.zeros(n, dtype=capi.OHM_FRAGMENT)
        fr = np.zeros(n, dtype=capi.OHM_FRAME_DESC)
        for i in range(n):
            fg[i]["src_offset"], fg[i]["n_frames"], fg[i]["attenuation"], fg[i]["flags"] = 64 * i, 16, capi.UNITY_ATTENUATION, capi.FLAG_SILENCE if silent else 0
            fr[i]["dst_offset"], fr[i]["sample_start"], fr[i]["frame"], fr[i]["first_fragment"], fr[i]["n_fragments"] = offs[i], 16 * i, i + 1, i, 1
        return Case("ohm", (_ptr(st), st.size, _ptr(fr), n, _ptr(fg), n), [st, fg, fr], _noise(64 * n, 6), dst_bytes, [(o, total.value) for o in offs])

    def _flac(self, hole, outputs, silent, empty):
        n = 0 if empty else (outputs or 1)
        c = FC.whole(self.tiny)
        each = FC.arena_bytes(c)                                    # planes of max_samples * 4 bytes, one after the other
        offs, dst_bytes = _offsets([each] * n, hole)
        d = np.zeros(n, dtype=capi.FLAC_STREAM_DESC)
        audio = np.frombuffer(c.data[c.offset:c.offset + c.src_bytes], dtype=np.uint8)
        for i in range(n):
            d[i]["src_offset"], d[i]["src_bytes"], d[i]["dst_offset"], d[i]["dst_plane_stride"] = audio.size * i, audio.size, offs[i], c.max_samples * 4
            d[i]["first_sample"], d[i]["max_samples"], d[i]["sample_rate"], d[i]["blocksize"] = c.first_sample, c.max_samples, c.rate, c.blocksize
            d[i]["max_blocksize"], d[i]["channels"], d[i]["bits"], d[i]["flags"] = c.max_blocksize, c.channels, c.bits, c.flags
        return Case("flac", (_ptr(d), n), [d], np.tile(audio, n), dst_bytes, [(o, each) for o in offs])

    # ---- the calls, by family, returning the library's code
    def create(self, case):
        b = C.c_void_p(1)                                           # (a failed create must have nulled it)
        code = getattr(capi.lib(), f"ohgpu_{case.family}_batch_create")(self.ctx.handle, *case.head, case.src.size, case.dst_bytes, C.byref(b))
        return code, b

    def run(self, family, batch, d_src, d_dst, stream=None):
        return getattr(capi.lib(), f"ohgpu_{family}_batch_run")(self.ctx.handle, batch, d_src, d_dst, stream)

    def process_host(self, case, dst):
        tail = ()
        if case.family == "flac":
            self.flac_results = np.zeros(case.head[1], dtype=capi.FLAC_STREAM_RESULT)
            tail = (_ptr(self.flac_results), None, 0, None)
        return getattr(capi.lib(), f"ohgpu_{case.family}_process_host")(self.ctx.handle, *case.head, _ptr(case.src), case.src.size, _ptr(dst), dst.size, *tail)

    def on_device(self, case, fill=DEV_FILL, stream=None):
        """create + run + destroy on device arenas: the destination arena afterwards (it starts as `fill`)."""
        ctx = self.ctx
        d_src, d_dst = ctx.upload(case.src), ctx.malloc(max(case.dst_bytes, 1))
        ctx.memset(d_dst, fill, case.dst_bytes)
        ctx.sync()
        code, b = self.create(case)
        assert code == capi.OK, capi.last_error()
        assert self.run(case.family, b, d_src, d_dst, stream) == capi.OK, capi.last_error()
        ctx.sync(stream)
        got = ctx.download(d_dst, case.dst_bytes)
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        return got


@pytest.fixture(scope="module")
def fx():
    f = Fixtures()
    yield f
    f.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_failed_create_leaves_nothing_behind(fx, family):
    good = fx.case(family)
    fx.on_device(good)                                              # warm-up: the context's block cache holds this batch's blocks
    allocs = fx.ctx.device_allocations()
    for _ in range(3):
        bad = fx.case(family, bad=True)
        code, b = fx.create(bad)
        assert code == capi.ERR_BOUNDS, (code, capi.last_error())
        assert b.value is None
        assert BOUNDS_TEXT[family] in capi.last_error(), capi.last_error()
    fx.on_device(good)
    assert fx.ctx.device_allocations() == allocs


@pytest.mark.parametrize("family", FAMILIES)
def test_run_refuses_another_familys_batch(fx, family):
    code, other = fx.create(fx.case("dsd" if family == "pcm" else "pcm"))
    assert code == capi.OK
    d = fx.ctx.malloc(4096)
    try:
        assert fx.run(family, other, d, d) == capi.ERR_INVALID
        assert capi.last_error() == f"ohgpu_{family}_batch_run: not a {NOUN[family]} batch"
        assert fx.run(family, None, d, d) == capi.ERR_INVALID
        assert capi.last_error() == f"ohgpu_{family}_batch_run: not a {NOUN[family]} batch"
    finally:
        fx.ctx.batch_destroy(other)
        fx.ctx.free(d)


@pytest.mark.parametrize("family", FAMILIES)
def test_null_arenas(fx, family):
    case = fx.case(family)
    code, b = fx.create(case)
    assert code == capi.OK, capi.last_error()
    d_src, d_dst = fx.ctx.upload(case.src), fx.ctx.malloc(case.dst_bytes)
    try:
        for src, dst in ((d_src, None), (None, d_dst), (None, None)):   # (this batch reads source bytes: no family runs it without them)
            assert fx.run(family, b, src, dst) == capi.ERR_INVALID
            assert capi.last_error() == f"ohgpu_{family}_batch_run: null arena pointer"
    finally:
        fx.ctx.batch_destroy(b)
    # a batch that reads no source byte: pcm and dsd run it without a source arena
    if family in ("pcm", "dsd"):
        silent = fx.case(family, silent=True)
        code, b = fx.create(silent)
        assert code == capi.OK, capi.last_error()
        try:
            assert fx.ctx.batch_info(b)["src_bytes_touched"] == 0
            assert fx.run(family, b, None, d_dst) == capi.OK, capi.last_error()
            fx.ctx.sync()
            assert fx.run(family, b, None, None) == capi.ERR_INVALID
        finally:
            fx.ctx.batch_destroy(b)
    fx.ctx.free(d_src)
    fx.ctx.free(d_dst)


@pytest.mark.parametrize("family", FAMILIES)
def test_empty_batch(fx, family):
    ctx = fx.ctx
    code, b = fx.create(fx.case(family, empty=True))
    assert code == capi.OK, capi.last_error()
    d = ctx.malloc(64)
    try:
        assert ctx.batch_info(b) == ZERO_INFO
        assert fx.run(family, b, d, d) == capi.OK, capi.last_error()
        if family != "flac":                                        # (FLAC has no "empty" rule: its run looks at the arenas first)
            assert fx.run(family, b, None, None) == capi.OK, capi.last_error()
        if family == "src":                                         # the timed run still records the caller's two events
            e0, e1 = ctx.event(), ctx.event()
            ctx.src_run(b, None, None, events=(e0, e1))
            assert ctx.elapsed_ms(e0, e1) >= 0.0
            ctx.event_destroy(e0)
            ctx.event_destroy(e1)
        ctx.sync()
    finally:
        ctx.batch_destroy(b)
        ctx.free(d)


@pytest.mark.parametrize("hole", [0, HOLE], ids=["adjacent", "hole"])
@pytest.mark.parametrize("family", sorted(HAS_HOST))
def test_process_host_equals_create_and_run(fx, family, hole):
    case = fx.case(family, hole=hole, outputs=None if family in ("pcm", "dsd", "src", "src_pull") else 2)
    assert len(case.ranges) >= 2
    want = fx.on_device(case)
    before = fx.ctx.host_transfer_stats()
    dst = np.full(case.dst_bytes, HOST_FILL, dtype=np.uint8)
    assert fx.process_host(case, dst) == capi.OK, capi.last_error()
    after = fx.ctx.host_transfer_stats()
    covered = np.zeros(case.dst_bytes, dtype=bool)
    for off, n in case.ranges:
        covered[off:off + n] = True
        assert np.array_equal(dst[off:off + n], want[off:off + n]), (family, off)
    assert np.all(dst[~covered] == HOST_FILL) and np.all(want[~covered] == DEV_FILL)      # the hole: nobody writes it
    assert int((~covered).sum()) == hole
    lo, hi = min(o for o, _ in case.ranges), max(o + n for o, n in case.ranges)
    moved = hi - lo                                                  # one copy of the covered span, hole included
    if family == "flac":                                             # ... FLAC: exactly what was decoded, plane by plane
        moved = int(sum(int(r["samples"]) * 4 * fx.tiny.info["channels"] for r in fx.flac_results))
        assert all(int(r["samples"]) == fx.tiny.samples for r in fx.flac_results)
    delta = {k: after[k] - before[k] for k in after}
    assert delta == {"calls": 1, "src_calls": 1 if family in ("src", "src_pull") else 0, "h2d_bytes": case.src.size, "d2h_bytes": moved}


@pytest.mark.parametrize("family", ["src", "flywheel"])
def test_one_launch_at_a_time(fx, family):
    ctx = fx.ctx
    case = fx.case(family)
    code, b = fx.create(case)
    assert code == capi.OK, capi.last_error()
    if family == "src":
        assert ctx.src_plan(b)["block_kernel_out_frames"] > 0       # (the unit counters are the plan's)
    d_src, d_dst = ctx.upload(case.src), ctx.malloc(case.dst_bytes)
    sa, sb = ctx.stream_create(), ctx.stream_create()
    try:
        ctx.memset(d_dst, DEV_FILL, case.dst_bytes)
        ctx.sync()
        assert fx.run(family, b, d_src, d_dst, sa) == capi.OK, capi.last_error()
        second = fx.run(family, b, d_src, d_dst, sb)                # at once, on another stream: refused, unless the first is over
        if second != capi.OK:
            assert second == capi.ERR_INVALID
            assert capi.last_error().startswith(f"ohgpu_{family}_batch_run: the batch is still running on another stream")
        ctx.sync(sa)
        ctx.sync(sb)
        first = ctx.download(d_dst, case.dst_bytes)
        ctx.memset(d_dst, DEV_FILL, case.dst_bytes)
        ctx.sync()
        assert fx.run(family, b, d_src, d_dst, sb) == capi.OK, capi.last_error()
        ctx.sync(sb)
        assert np.array_equal(ctx.download(d_dst, case.dst_bytes), first)
        assert np.any(first != DEV_FILL)
    finally:
        ctx.batch_destroy(b)
        ctx.stream_destroy(sa)
        ctx.stream_destroy(sb)
        ctx.free(d_src)
        ctx.free(d_dst)
