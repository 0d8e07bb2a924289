"""The shell every batch family of the C ABI shares (tests/test_gpu_batch_lifecycle.py), for the Apple Lossless family: what a failed
create leaves behind, what a run refuses (another family's batch, null arenas) and accepts (an empty batch), and that the
host-buffer call equals create + run on device arenas and moves exactly what was decoded.  The batch is the smallest there is: one
stereo stream of one handmade packet of eight samples (tests/alac_cases.handmade: hand_stereo8)."""
import ctypes as C

import numpy as np
import pytest

import alac_cases as AC
import alac_textbook as T
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

HOLE = 64
DEV_FILL, HOST_FILL = 0xA5, 0x5A
ZERO_INFO = {"n_msgs": 0, "in_frames": 0, "out_frames": 0, "src_bytes_touched": 0, "dst_bytes_written": 0}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


class Fixtures:
    def __init__(self):
        self.ctx = capi.Context(0)
        cookie, (self.packet,) = AC.handmade()["hand_stereo8"]
        self.cfg = T.parse_config(cookie)
        self.each = 2 * self.cfg["frame_length"] * 4               # two planes of one packet's frame length, one after the other

    def close(self):
        self.ctx.close()

    def case(self, n=1, hole=0, bad=False):
        """n streams of the one packet; `hole` bytes between the first stream's planes and the second's"""
        descs = np.zeros(n, dtype=capi.ALAC_STREAM_DESC)
        packets = np.zeros(n, dtype=capi.ALAC_PACKET)
        at = 0
        for i in range(n):
            for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "sample_rate"):
                descs[i][k] = self.cfg[k]
            descs[i]["first_packet"], descs[i]["n_packets"], descs[i]["dst_offset"], descs[i]["dst_plane_stride"] = i, 1, at, self.cfg["frame_length"] * 4
            packets[i]["src_offset"], packets[i]["bytes"] = i * len(self.packet), len(self.packet)
            at += self.each + (hole if i == 0 and n > 1 else 0)
        if bad:
            descs[-1]["dst_offset"] = at
        src = np.frombuffer(self.packet * n, dtype=np.uint8)
        return descs, packets, src, at

    def create(self, case):
        descs, packets, src, dst_bytes = case
        b = C.c_void_p(1)                                           # (a failed create must have nulled it)
        code = capi.lib().ohgpu_alac_batch_create(self.ctx.handle, _ptr(descs), descs.size, _ptr(packets), packets.size, src.size, dst_bytes, C.byref(b))
        return code, b

    def run(self, batch, d_src, d_dst, stream=None):
        return capi.lib().ohgpu_alac_batch_run(self.ctx.handle, batch, d_src, d_dst, stream)

    def on_device(self, case):
        ctx = self.ctx
        _, _, src, dst_bytes = case
        d_src, d_dst = ctx.upload(src), ctx.malloc(max(dst_bytes, 1))
        ctx.memset(d_dst, DEV_FILL, dst_bytes)
        ctx.sync()
        code, b = self.create(case)
        assert code == capi.OK, capi.last_error()
        assert self.run(b, d_src, d_dst) == capi.OK, capi.last_error()
        ctx.sync()
        got = ctx.download(d_dst, dst_bytes)
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        return got


@pytest.fixture(scope="module")
def fx():
    f = Fixtures()
    yield f
    f.close()


def test_failed_create_leaves_nothing_behind(fx):
    good = fx.case()
    fx.on_device(good)                                              # warm-up: the context's block cache holds this batch's blocks
    allocs = fx.ctx.device_allocations()
    for _ in range(3):
        code, b = fx.create(fx.case(bad=True))
        assert code == capi.ERR_BOUNDS, (code, capi.last_error())
        assert b.value is None
        assert "alac desc 0: writes [" in capi.last_error(), capi.last_error()
    fx.on_device(good)
    assert fx.ctx.device_allocations() == allocs


def test_run_refuses_another_familys_batch_and_the_others_refuse_this_one(fx):
    d = np.zeros(2, dtype=capi.MSG_DESC)
    for i in range(2):
        d[i] = (64 * i, 96 * i, 16, 0, 0, capi.UNITY_ATTENUATION, 2, 16, capi.ENDIAN_LITTLE, 24, capi.ENDIAN_BIG, 0)
    other = fx.ctx.pcm_batch(d, 128, 192)
    code, mine = fx.create(fx.case())
    assert code == capi.OK, capi.last_error()
    dev = fx.ctx.malloc(4096)
    try:
        for batch in (other, None):
            assert fx.run(batch, dev, dev) == capi.ERR_INVALID
            assert capi.last_error() == "ohgpu_alac_batch_run: not a lossless-packet (ALAC) batch"
        assert capi.lib().ohgpu_pcm_batch_run(fx.ctx.handle, mine, dev, dev, None) == capi.ERR_INVALID
        assert capi.last_error() == "ohgpu_pcm_batch_run: not a pcm batch"
        assert capi.lib().ohgpu_flac_batch_run(fx.ctx.handle, mine, dev, dev, None) == capi.ERR_INVALID
        res = np.zeros(1, dtype=capi.ALAC_STREAM_RESULT)
        assert capi.lib().ohgpu_alac_batch_results(fx.ctx.handle, other, _ptr(res), 1, None, 0) == capi.ERR_INVALID
    finally:
        fx.ctx.batch_destroy(other)
        fx.ctx.batch_destroy(mine)
        fx.ctx.free(dev)


def test_null_arenas(fx):
    case = fx.case()
    code, b = fx.create(case)
    assert code == capi.OK, capi.last_error()
    d_src, d_dst = fx.ctx.upload(case[2]), fx.ctx.malloc(case[3])
    try:
        for src, dst in ((d_src, None), (None, d_dst), (None, None)):
            assert fx.run(b, src, dst) == capi.ERR_INVALID
            assert capi.last_error() == "ohgpu_alac_batch_run: null arena pointer"
    finally:
        fx.ctx.batch_destroy(b)
        fx.ctx.free(d_src)
        fx.ctx.free(d_dst)


def test_empty_batch(fx):
    ctx = fx.ctx
    code, b = fx.create(fx.case(n=0))
    assert code == capi.OK, capi.last_error()
    d = ctx.malloc(64)
    try:
        assert ctx.batch_info(b) == ZERO_INFO
        assert fx.run(b, d, d) == capi.OK, capi.last_error()
        assert fx.run(b, None, None) == capi.OK, capi.last_error()
        sres, pres = ctx.alac_results(b, 0, 0)
        assert sres.size == 0 and pres.size == 0
        ctx.sync()
    finally:
        ctx.batch_destroy(b)
        ctx.free(d)


@pytest.mark.parametrize("hole", [0, HOLE], ids=["adjacent", "hole"])
def test_process_host_equals_create_and_run(fx, hole):
    case = fx.case(n=2, hole=hole)
    descs, packets, src, dst_bytes = case
    want = fx.on_device(case)
    before = fx.ctx.host_transfer_stats()
    dst = np.full(dst_bytes, HOST_FILL, dtype=np.uint8)
    sres, pres = fx.ctx.alac_process_host(descs, packets, src, dst)
    after = fx.ctx.host_transfer_stats()
    assert [int(p["samples"]) for p in pres] == [8, 8] and [int(s["packets_ok"]) for s in sres] == [1, 1]
    covered = np.zeros(dst_bytes, dtype=bool)
    for d in descs:
        for c in range(2):
            at = int(d["dst_offset"]) + c * int(d["dst_plane_stride"])
            covered[at:at + 8 * 4] = True                           # the packet's eight samples of a frame length of 64
    assert np.array_equal(dst[covered], want[covered]) and np.any(want[covered] != DEV_FILL)
    assert np.all(dst[~covered] == HOST_FILL) and np.all(want[~covered] == DEV_FILL)
    delta = {k: after[k] - before[k] for k in after}
    assert delta == {"calls": 1, "src_calls": 0, "h2d_bytes": src.size, "d2h_bytes": 2 * 2 * 8 * 4}      # exactly what was decoded, plane by plane
