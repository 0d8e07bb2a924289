"""Arena offsets of 2^31 and more: what tests/test_gpu_far_offsets.py runs and tests/test_far_cases.py checks without a device.

Every descriptor of include/ohgpu.h carries 64-bit arena offsets and the header puts no upper limit on an arena's size.  A far test
runs a family's existing small case twice in one batch -- copy 0 at a near offset, copy 1 at a far one -- inside two device blocks
of LEAD + SPAN bytes, one a side, and compares windows: the far copy's bytes must equal the near copy's, which must equal the
family's textbook model, with the guards either side untouched.

The lead-in.  A kernel that truncated an offset would write (or read) at another address.  So that such a kernel fails a comparison
instead of faulting a shared card, every address the wrong arithmetic could make lies inside the block: the arena's base is LEAD =
2^31 bytes into it, the arena is SPAN = 2^32 + 2^26 bytes, and aliases() lists where a range lands under the low 32 bits of the
offset (down to 0), those sign-extended (down to -2^31: the lead-in) and the low 31 bits.  The destination's alias windows are
filled before a run and must still hold the fill after it.

Placements.  For a moved range of n bytes: straddle31 and straddle32 put byte 2^31 (2^32) strictly inside it, beyond lies past
2^32 at an odd offset; each rounded down to the family's alignment.  NEAR: where copy 0 goes.  (A range that straddles 2^32 has an
alias at offset 0, n / 2 bytes long: the near copy sits above it, at 2^20.)

relocate() moves a family's descriptor tables: it adds the shifts to the fields RELOCATE lists, and to nothing else; RESULTS lists
every 64-bit field of the result structs, by whether it is absolute in an arena (expected shifted by the relocation) or relative
to its stream's src_offset / dst_offset (expected unchanged).  TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

LEAD = 1 << 31
SPAN = (1 << 32) + (1 << 26)
GUARD = 4096
NEAR = 1 << 20
BEYOND = (1 << 32) + (1 << 25) + 4099
MAX_RANGE = 2 * (NEAR - 2 * GUARD)                  # a moved range longer than this: its alias at 0 would reach the near copy
PAIRS = ("s32_s31", "s31_s32", "beyond")            # (source placement, destination placement) of the far copy


def straddle(boundary, n, align):
    """The offset of an n-byte range, a multiple of align, with byte `boundary` strictly inside it (n >= 2 * align + 2)."""
    off = (boundary - n // 2) // align * align
    assert off < boundary < off + n - 1, (boundary, n, align)
    return off


def placement(kind, n, align):
    if kind == "s31":
        return straddle(1 << 31, n, align)
    if kind == "s32":
        return straddle(1 << 32, n, align)
    assert kind == "beyond"
    return BEYOND // align * align


def near(align):
    return NEAR + (4099 // align * align) % 4096     # (4099: odd where the family takes any address)


def pair(name, n_src, n_dst, src_align, dst_align):
    """(source offset, destination offset) of the far copy under one of PAIRS."""
    s, d = {"s32_s31": ("s32", "s31"), "s31_s32": ("s31", "s32"), "beyond": ("beyond", "beyond")}[name]
    return placement(s, n_src, src_align), placement(d, n_dst, dst_align)


def _pieces(offset, length):
    """[offset, offset + length) cut at the multiples of 2^31: on each piece the wrong arithmetics are shifts."""
    at, end = offset, offset + length
    while at < end:
        stop = min(end, (at // (1 << 31) + 1) << 31)
        yield at, stop - at
        at = stop


def aliases(offset, length):
    """[(alias offset, bytes)]: where the bytes of [offset, + length) would be looked for under the low 32 bits of their offset,
    those sign-extended, and the low 31 bits -- the pieces that land somewhere else than they belong, relative to the arena's base
    (negative: in the lead-in), without repeats."""
    out = []
    for at, n in _pieces(offset, length):
        low32 = at & 0xffffffff
        for wrong in (low32, low32 - (1 << 32) if low32 & (1 << 31) else low32, at & 0x7fffffff):
            if wrong != at and (wrong, n) not in out:
                out.append((wrong, n))
    return out


def overlaps(a, n_a, b, n_b):
    return a < b + n_b and b < a + n_a


class FarArenas:
    """Two device blocks of LEAD + SPAN bytes, one a side; src and dst: the arenas' bases, LEAD bytes in.  Allocated once a module by
    one process (about 6.1 GiB a side), never filled or downloaded whole; close() frees them."""

    def __init__(self, ctx):
        self.ctx, self.blocks = ctx, []
        try:
            for _ in range(2):
                self.blocks.append(ctx.malloc(LEAD + SPAN))
        except BaseException:
            self.close()
            raise
        self.src, self.dst = (ctypes.c_void_p(b.value + LEAD) for b in self.blocks)

    def close(self):
        while self.blocks:
            self.ctx.free(self.blocks.pop())

    @staticmethod
    def at(base, offset):
        assert -LEAD <= offset < SPAN
        return ctypes.c_void_p(base.value + offset)

    def fill(self, base, offset, n, value):
        assert -LEAD <= offset and offset + n <= SPAN
        self.ctx.memset(self.at(base, offset), value, n)

    def put(self, base, offset, data):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        assert 0 <= offset and offset + data.size <= SPAN
        if data.size:
            self.ctx.copy_h2d(self.at(base, offset), data)
            self.ctx.sync()

    def get(self, base, offset, n):
        assert -LEAD <= offset and offset + n <= SPAN
        return self.ctx.download(self.at(base, offset), n)


class Twin:
    """One case laid twice into the far arenas: its whole source arena (src: uint8) and its whole destination arena (dst0: what it
    holds before the run, uint8; the bytes no message writes must come back as they went in) at (src_at[k], dst_at[k]), k = 0 the
    near copy and 1 the far one.  prepare() fills the windows and the alias windows and uploads; check(want) downloads them and
    holds both copies to `want`, the model's whole destination arena of the near layout, the guards and the alias windows to the
    fill."""

    def __init__(self, arenas, src, dst0, pair_name, src_align, dst_align, fill):
        self.arenas, self.fill = arenas, fill
        self.src = np.ascontiguousarray(src, dtype=np.uint8)
        self.dst0 = np.ascontiguousarray(dst0, dtype=np.uint8)
        assert 2 * max(src_align, dst_align) + 2 <= min(self.src.size, self.dst0.size) and max(self.src.size, self.dst0.size) <= MAX_RANGE
        far = pair(pair_name, self.src.size, self.dst0.size, src_align, dst_align)
        self.src_at, self.dst_at = (near(src_align), far[0]), (near(dst_align), far[1])

    def alias_windows(self, side):
        at, n = (self.src_at, self.src.size) if side == "src" else (self.dst_at, self.dst0.size)
        return [w for k in (0, 1) for w in aliases(at[k], n)]

    def prepare(self):
        a = self.arenas
        for base, side in ((a.src, "src"), (a.dst, "dst")):
            for off, n in self.alias_windows(side):
                a.fill(base, off, n, self.fill)
        for k in (0, 1):
            a.fill(a.src, self.src_at[k] - GUARD, self.src.size + 2 * GUARD, self.fill)
            a.put(a.src, self.src_at[k], self.src)
            a.fill(a.dst, self.dst_at[k] - GUARD, self.dst0.size + 2 * GUARD, self.fill)
            a.put(a.dst, self.dst_at[k], self.dst0)
        a.ctx.sync()

    def check(self, want, what):
        a, n = self.arenas, self.dst0.size
        assert want.size == n
        for k, name in ((0, "near"), (1, "far")):
            got = a.get(a.dst, self.dst_at[k] - GUARD, n + 2 * GUARD)
            bad = np.flatnonzero(got[GUARD:GUARD + n] != want)
            assert bad.size == 0, f"{what}, {name} copy at {self.dst_at[k]:#x}: {bad.size} of {n} bytes differ, first at {bad[:6].tolist()}"
            assert (got[:GUARD] == self.fill).all() and (got[GUARD + n:] == self.fill).all(), f"{what}, {name} copy: a guard was written"
        for off, m in self.alias_windows("dst"):
            assert (a.get(a.dst, off, m) == self.fill).all(), f"{what}: the alias window at {off:#x} (+{m}) was written"


# ---------------------------------------------------------------- relocation
# family (the * of ohgpu_*_batch_create) -> {table: (fields that are source arena offsets, fields that are destination arena offsets)}
RELOCATE = {
    "pcm": {"descs": (("src_offset",), ("dst_offset",))},
    "fmt": {"descs": (("src_offset",), ("dst_offset",))},
    "dsd": {"descs": (("src_offset",), ("dst_offset",))},
    "dsd_pcm": {"descs": (("src_offset",), ("dst_offset",))},
    "flac": {"descs": (("src_offset",), ("dst_offset",))},
    "alac": {"descs": ((), ("dst_offset",)), "packets": (("src_offset",), ())},
    "raop": {"descs": ((), ("dst_offset",)), "packets": (("src_offset",), ())},
    "flywheel": {"descs": (("src_offset",), ("dst_offset",))},
    "ohm": {"streams": ((), ()), "frames": ((), ("dst_offset",)), "fragments": (("src_offset",), ())},
    "ohm_rx": {"streams": ((), ("dst_offset",)), "datagrams": (("src_offset",), ())},
    "ogg": {"descs": (("src_offset",), ("dst_offset",))},
    "mp4": {"descs": (("src_offset",), ())},
    "mp4f": {"descs": (("src_offset",), ("dst_offset",))},
    "iff": {"descs": (("src_offset",), ("dst_offset",))},
    "dsd_file": {"descs": (("src_offset",), ("dst_offset",))},
    "src": {"descs": (("src_offset",), ("dst_offset",))},
    "src_pull": {"descs": (("src_offset",), ("dst_offset",))},
}

# The alignment a family's header text asks of an offset, a side: what a placement is rounded to.  (The block resamplers and the
# Songcast receiver ask it of base + offset; the bases here are 2^31 past a device allocation, aligned far beyond 16.  The line
# kernels -- pcm, fmt, dsd -- take any address but plan a message onto a path by its addresses' residues modulo 16: a shift that is
# a multiple of 16 keeps every message's own residue, odd ones among them, so that the far copy is planned onto the near copy's paths.)
ALIGN = {
    "pcm": (16, 16), "fmt": (16, 16), "dsd": (16, 16), "dsd_pcm": (1, 1), "flac": (1, 4), "alac": (1, 4), "raop": (16, 4), "flywheel": (1, 1),
    "ohm": (1, 1), "ohm_rx": (4, 1), "ogg": (1, 1), "mp4": (1, 1), "mp4f": (1, 1), "iff": (1, 1), "dsd_file": (1, 16), "src": (16, 1),
    "src_pull": (16, 1),
}

# Every 64-bit field of the result structs and tables a run writes: absolute in an arena (src / dst: expected moved by that side's
# shift) or not (counts, stream positions, and offsets from the stream's own src_offset / dst_offset: expected unchanged).
RESULTS = {
    "ohgpu_flac_stream_result": {"same": ("samples", "first_sample_decoded", "bytes_consumed", "reserved")},
    "ohgpu_flac_frame": {"same": ("first_sample",)},
    "ohgpu_alac_stream_result": {"same": ("samples",)},
    "ohgpu_alac_packet": {"src": ("src_offset",)},                       # the rows the MPEG-4 and fragmented MPEG-4 walks write
    "ohgpu_ohm_rx_record": {"dst": ("dst_offset",), "same": ("sample_start", "samples_total")},
    "ohgpu_ohm_rx_stream_result": {"same": ("last_sample_start", "out_bytes")},
    "ohgpu_ogg_stream_result": {"same": ("bytes_delivered", "bytes_consumed", "last_granule", "reserved2")},
    "ohgpu_ogg_packet": {"same": ("run_pos", "granule", "page_offset")},
    "ohgpu_mp4_stream_result": {"same": ("duration", "frames", "moov_offset", "mdat_offset", "mdat_bytes", "error_offset")},
    "ohgpu_mp4_sample": {"same": ("first_frame",)},
    "ohgpu_mp4f_run": {"src": ("data_offset",), "same": ("first_frame", "bytes")},
    "ohgpu_mp4f_stream_result": {"same": ("duration", "frames", "samples", "bytes_gathered", "moov_offset", "first_moof_offset", "error_offset")},
    "ohgpu_iff_stream_result": {"same": ("frames_total", "frames_available", "frames_written", "data_offset", "data_bytes", "error_offset")},
    "ohgpu_dsd_file_stream_result": {"same": ("sample_count", "chunks_total", "chunks_available", "chunks_written", "bytes_written", "data_offset",
                                              "data_bytes", "metadata_offset", "error_offset")},
}


def relocate(family, tables, src_shift, dst_shift):
    """Copies of a family's descriptor tables ({name: structured array}) with the shifts added to the fields RELOCATE lists."""
    spec = RELOCATE[family]
    assert set(tables) == set(spec), (family, sorted(tables))
    out = {}
    for name, (src_fields, dst_fields) in spec.items():
        t = tables[name].copy()
        for f in src_fields:
            t[f] += np.uint64(src_shift)
        for f in dst_fields:
            t[f] += np.uint64(dst_shift)
        out[name] = t
    return out


def twice(family, descs, twin):
    """A single-table family's descriptors for both copies of `twin`, the near copy's first."""
    return np.concatenate([relocate(family, {"descs": descs}, twin.src_at[k], twin.dst_at[k])["descs"] for k in (0, 1)])
