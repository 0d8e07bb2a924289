"""What the layout-changing kernels' GPU tests share (tests/test_gpu_fmt_textbook.py, tests/test_gpu_far_offsets.py): the batch
builder, the planner's documented chunk rule, the route a batch's paths name, and the expected destination arena from
tests/fmt_textbook.py.  TEST INFRASTRUCTURE ONLY."""
import hashlib

import numpy as np

import fmt_textbook as FT
from ohpipeline_amd import capi

A11, A13, A14 = capi.FMT_UNPACK_PLANAR, capi.FMT_SENDER_PACK, capi.FMT_FLAC_PACK
FILL = 0xA5
PCM_LINE, OHM_WIDE, FMT_LINE, FMT_V1 = "pcm_line", "ohm_wide", "fmt_line_kernel", "fmt_kernel_v1"
STEREO = {(A11, 2): "unpack_stereo_kernel<2>", (A11, 3): "unpack_stereo_kernel<3>", (A11, 4): "unpack_stereo_kernel<4>",
          (A14, 1): "flac_stereo_kernel<1>", (A14, 2): "flac_stereo_kernel<2>", (A14, 3): "flac_stereo_kernel<3>"}
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
EDGES = sorted({0, 1, -1, INT32_MIN, INT32_MAX, INT32_MIN + 1, INT32_MAX - 1}
               | {s * (1 << p) + e for p in (7, 15, 23) for s in (1, -1) for e in (-1, 0, 1)})


def frames_per_chunk(kind, ch, width):
    """The documented rule (module docstring); width = source bytes per subsample (a11, a13); a14's source is 4 bytes."""
    budget = 2304 - 32
    if kind == A11:
        return min(512, budget // (ch * width) - 4)
    if kind == A13:
        return min(512 // min(ch, 2), budget // (ch * width) - 4)
    return min(512 // ch, (budget // ch - 64) // 4)


class Batch:
    """Descriptors laid one after another into a source arena of seeded bytes and a destination arena, each where the caller
    asks: `sres` = the source offset's residue mod 16, `dres` = the destination offset's mod 4, `gap` = untouched bytes before the
    output."""

    def __init__(self, seed, src_lead=0, dst_lead=0):
        self.rng = np.random.default_rng(seed)
        self.src = bytearray(self.rng.bytes(src_lead))
        self.rows, self.dp = [], dst_lead

    def _src_at(self, mod, res):
        if res is not None:
            self.src += self.rng.bytes((res - len(self.src)) % mod)
        return len(self.src)

    def _dst_at(self, res, gap):
        dp = self.dp + gap
        return dp if res is None else dp + (res - dp) % 4

    def _row(self, kind, ch, n, sbits, dbits, so, do, sstride, dstride, out_bytes):
        self.rows.append((so, do, sstride, dstride, n, kind, ch, sbits, dbits, [0] * 8))
        if n:
            self.dp = do + out_bytes
        return self

    def unpack(self, ch, sb, n, sres=None, dres=None, extra=0, gap=0):
        so = self._src_at(16, sres)
        self.src += self.rng.bytes(n * ch * sb)
        stride = 4 * n + extra
        return self._row(A11, ch, n, 8 * sb, 0, so, self._dst_at(dres, gap), 0, stride, (ch - 1) * stride + 4 * n)

    def sender(self, ch, sb, n, sres=None, dres=None, gap=0):
        so = self._src_at(16, sres)
        self.src += self.rng.bytes(n * ch * sb)
        return self._row(A13, ch, n, 8 * sb, 0, so, self._dst_at(dres, gap), 0, 0, n * min(ch, 2) * min(sb, 3))

    def flac(self, ch, bits, n, sres=None, dres=None, stride=None, values=None, gap=0):
        """stride: bytes between planes (default 4 * n rounded up to 16); values: what every plane holds (rolled by one per channel),
        default seeded bytes, that is, the whole TInt32 range."""
        so = self._src_at(16, sres) if sres is not None else self._src_at(4, 0)
        stride = (4 * n + 15) // 16 * 16 if stride is None else stride
        assert so % 4 == 0 and stride % 4 == 0 and stride >= 4 * n
        for c in range(ch):
            if values is None:
                plane = self.rng.bytes(4 * n)
            else:
                plane = np.roll(np.array(values, dtype=np.int64), c).astype("<i4").tobytes()
                assert len(plane) == 4 * n
            self.src += plane + (self.rng.bytes(stride - 4 * n) if c + 1 < ch else b"")
        return self._row(A14, ch, n, 32, bits, so, self._dst_at(dres, gap), stride, 0, n * ch * bits // 8)

    def zero(self, kind, ch=2, sbits=16, dbits=0):
        """A descriptor of no frames, its offsets far beyond both arenas: accepted, writes nothing, takes no record."""
        self.rows.append((1 << 40, (1 << 41) + 1, 1 << 20 if kind == A14 else 0, 0, 0, kind, ch, sbits, dbits, [0] * 8))
        return self

    def finish(self, dst_tail=0):
        return np.array(self.rows, dtype=capi.FMT_DESC), np.frombuffer(bytes(self.src), dtype=np.uint8), self.dp + dst_tail


def route_of(paths):
    """The route's name, after checking that the counts of no other route are set."""
    fmt_keys = ("fmt_wide_records", "fmt_stereo_records", "fmt_stereo_kind", "fmt_stereo_bytes", "fmt_staged_chunks")
    ohm_keys = ("prefixed_chunks", "ohm_wide_fragments", "ohm_staged_fragments", "ohm_headers_fused", "ohm_headers_separate")
    assert all(paths[k] == 0 for k in ohm_keys), paths
    if paths["line_planned"]:
        assert all(paths[k] == 0 for k in fmt_keys) and paths["launches"] == 1 and paths["group_chunks"] > 0, paths
        assert paths["staged_chunks"] == 0 and paths["heavy_chunks"] == 0, paths
        return PCM_LINE
    assert all(paths[k] == 0 for k in ("launches", "staged_chunks", "group_chunks", "heavy_chunks")), paths
    set_ = [k for k in ("fmt_wide_records", "fmt_stereo_records", "fmt_staged_chunks") if paths[k]]
    assert len(set_) <= 1, paths
    if not set_:
        assert all(paths[k] == 0 for k in fmt_keys), paths
        return FMT_V1
    if set_[0] == "fmt_stereo_records":
        return STEREO[(paths["fmt_stereo_kind"], paths["fmt_stereo_bytes"])]
    assert paths["fmt_stereo_kind"] == 0 and paths["fmt_stereo_bytes"] == 0, paths
    return OHM_WIDE if set_[0] == "fmt_wide_records" else FMT_LINE


_WANT = {}


def expected(descs, src, dst_bytes):
    """(kept per input: `vctx` runs every test twice on the same seeded bytes, and the model is slow)"""
    key = hashlib.sha256(descs.tobytes() + src.tobytes() + dst_bytes.to_bytes(8, "little")).digest()
    if key not in _WANT:
        _WANT[key] = np.frombuffer(FT.batch_bytes(descs, src.tobytes(), dst_bytes, FILL), dtype=np.uint8)
    return _WANT[key]
