"""tests/fmt_textbook.py (the three layout-changing processors from their definitions) tied to the oracle's restatement, to answers
written out by hand from the reference's text, and to the fixture tests/golden/fmt_textbook.json.  The oracle and the kernels were
written from the same reading of the reference; the model is a second reading, so a misreading the two share shows up here (CPU) or
in test_gpu_fmt_textbook.py.  Every comparison is of bytes, over everything the operation may write."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fmt_textbook as FT
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "fmt_textbook.json")
GENERATOR = os.path.join(HERE, "golden", "make_fmt_textbook_fixtures.py")
FRAMES = [0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 511, 512, 513]
FILL = 0xA5
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
EDGES = sorted({0, 1, -1, INT32_MIN, INT32_MAX, INT32_MIN + 1, INT32_MAX - 1}
               | {s * (1 << p) + e for p in (7, 15, 23) for s in (1, -1) for e in (-1, 0, 1)})


def desc(kind, channels, n_frames, src_bits=0, dst_bits=0, src_offset=0, dst_offset=0, src_plane_stride=0, dst_plane_stride=0):
    return {"kind": kind, "channels": channels, "n_frames": n_frames, "src_bits": src_bits, "dst_bits": dst_bits, "src_offset": src_offset,
            "dst_offset": dst_offset, "src_plane_stride": src_plane_stride, "dst_plane_stride": dst_plane_stride}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_unpack(src, ch, sb, n, stride):
    want = np.full(max((ch - 1) * stride + 4 * n, 1), FILL, dtype=np.uint8)
    pos = np.zeros(ch, dtype=np.uint32)
    data = np.frombuffer(src, dtype=np.uint8) if src else np.zeros(1, np.uint8)
    assert O.lib().ohp_flywheel_unpack(_ptr(data), len(src), ch, sb, _ptr(want), stride, pos.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert pos.tolist() == [4 * n] * ch
    return want[:(ch - 1) * stride + 4 * n].tobytes() if n else b""


def oracle_sender(src, ch, sb, n):
    counted = n * min(ch, 2) * min(sb, 3)
    want = np.full(counted + 8, FILL, dtype=np.uint8)
    nb = C.c_uint32(0)
    data = np.frombuffer(src, dtype=np.uint8) if src else np.zeros(1, np.uint8)
    assert O.lib().ohp_sender_pack(_ptr(data), len(src), ch, sb, _ptr(want), C.byref(nb)) == 0
    assert nb.value == counted
    return want[:counted].tobytes()


def oracle_flac(planes, bits):
    ch, n = planes.shape
    want = np.full(n * ch * bits // 8 + 8, FILL, dtype=np.uint8)
    rows = [np.ascontiguousarray(planes[c]) for c in range(ch)]
    ptrs = (C.POINTER(C.c_int32) * ch)(*[r.ctypes.data_as(C.POINTER(C.c_int32)) for r in rows])
    nb = C.c_uint32(0)
    assert O.lib().ohp_flac_pack(ptrs, ch, 0, n, bits, _ptr(want), C.byref(nb)) == 0
    assert nb.value == n * ch * bits // 8 and (want[nb.value:] == FILL).all()
    return want[:nb.value].tobytes()


@pytest.mark.parametrize("sb", [1, 2, 3, 4])
def test_unpack_planar_model_equals_oracle(sb):
    rng = np.random.default_rng(100 + sb)
    for ch in range(1, 11):
        for n in FRAMES:
            src = rng.integers(0, 256, size=n * ch * sb, dtype=np.uint8).tobytes()
            stride = 4 * n + 4 * (ch % 3)                               # bytes between the planes stay untouched
            d = desc(FT.UNPACK_PLANAR, ch, n, src_bits=8 * sb, dst_plane_stride=stride)
            size = (ch - 1) * stride + 4 * n if n else 0
            assert FT.batch_bytes([d], src, size, FILL) == oracle_unpack(src, ch, sb, n, stride), (sb, ch, n)


@pytest.mark.parametrize("sb", [1, 2, 3, 4])
def test_sender_pack_model_equals_oracle(sb):
    rng = np.random.default_rng(200 + sb)
    for ch in range(1, 11):
        for n in FRAMES:
            src = rng.integers(0, 256, size=n * ch * sb, dtype=np.uint8).tobytes()
            (off, got), = FT.sender_pack(desc(FT.SENDER_PACK, ch, n, src_bits=8 * sb, dst_offset=7), src)
            assert off == 7 and got == oracle_sender(src, ch, sb, n), (sb, ch, n)


@pytest.mark.parametrize("bits", [8, 16, 24])
def test_flac_pack_model_equals_oracle(bits):
    """Seeded planes over the whole TInt32 range (so most values lie outside the depth), then planes built from the edge values."""
    rng = np.random.default_rng(300 + bits)
    for ch in range(1, 11):
        for n in FRAMES:
            planes = rng.integers(INT32_MIN, INT32_MAX + 1, size=(ch, n + ch % 3), dtype=np.int64).astype(np.int32)
            d = desc(FT.FLAC_PACK, ch, n, src_bits=32, dst_bits=bits, src_plane_stride=4 * (n + ch % 3))
            (off, got), = FT.flac_pack(d, planes.astype("<i4").tobytes())
            assert off == 0 and got == oracle_flac(planes[:, :n], bits), (bits, ch, n)
    for ch in (1, 2, 3):
        planes = np.array([np.roll(EDGES, c) for c in range(ch)], dtype=np.int64).astype(np.int32)
        d = desc(FT.FLAC_PACK, ch, len(EDGES), src_bits=32, dst_bits=bits, src_plane_stride=4 * len(EDGES))
        (_, got), = FT.flac_pack(d, planes.astype("<i4").tobytes())
        assert got == oracle_flac(planes, bits), (bits, ch)
        if ch == 1:                                                     # truncation, stated once more without the oracle
            assert got == b"".join((v & ((1 << bits) - 1)).to_bytes(bits // 8, "big") for v in EDGES)


def test_known_answers_from_the_reference_text():
    h = bytes.fromhex
    # a13, Sender.cpp:351-377.  Ten channels of 16 bits, bytes 00..13 hex: FirstChannelToSend(10) == 8 -> channels 8 and 9
    ten = bytes(range(20)) + bytes(range(0x80, 0x94))
    assert FT.sender_pack(desc(FT.SENDER_PACK, 10, 2, src_bits=16), ten) == [(0, h("10111213" "90919293"))]
    # nine channels: FirstChannelToSend(9) == 0 -> channels 0 and 1
    nine = bytes(range(18)) + bytes(range(0x80, 0x92))
    assert FT.sender_pack(desc(FT.SENDER_PACK, 9, 2, src_bits=16), nine) == [(0, h("00010203" "80818283"))]
    # mono, 24 bits: one subsample per frame survives; the second copy is overwritten a frame later and the last is not counted
    assert FT.sender_pack(desc(FT.SENDER_PACK, 1, 3, src_bits=24, dst_offset=5), h("010203" "040506" "070809")) == [(5, h("010203040506070809"))]
    # mono, 32 bits: three of every four bytes
    assert FT.sender_pack(desc(FT.SENDER_PACK, 1, 2, src_bits=32), h("01020304" "05060708")) == [(0, h("010203" "050607"))]
    # stereo, 32 bits: each subsample loses its fourth byte
    assert FT.sender_pack(desc(FT.SENDER_PACK, 2, 1, src_bits=32), h("11223344" "55667788")) == [(0, h("112233" "556677"))]
    # three channels of 8 bits, two frames: the third channel is dropped
    assert FT.sender_pack(desc(FT.SENDER_PACK, 3, 2, src_bits=8), h("a1a2a3" "b1b2b3")) == [(0, h("a1a2" "b1b2"))]
    # a11, StarvationRamper.cpp:117-186: stereo, channel 1's plane `stride` bytes after channel 0's, at offset 3
    u = lambda sb, n, data: FT.unpack_planar(desc(FT.UNPACK_PLANAR, 2, n, src_bits=8 * sb, dst_offset=3, dst_plane_stride=100), h(data))
    assert u(1, 2, "01020304") == [(3, h("01000000" "03000000")), (103, h("02000000" "04000000"))]
    assert u(2, 2, "0102030405060708") == [(3, h("01020000" "05060000")), (103, h("03040000" "07080000"))]
    assert u(3, 1, "010203040506") == [(3, h("01020300")), (103, h("04050600"))]
    assert u(4, 1, "0102030405060708") == [(3, h("01020304")), (103, h("05060708"))]
    # a14, Flac.cpp:379-417: the low bytes of each TInt32, most significant first; what lies above the depth is dropped
    le = lambda *v: b"".join((x & 0xFFFFFFFF).to_bytes(4, "little") for x in v)
    assert FT.flac_pack(desc(FT.FLAC_PACK, 1, 2, src_bits=32, dst_bits=8), le(-2, 0x1234)) == [(0, h("fe34"))]
    assert FT.flac_pack(desc(FT.FLAC_PACK, 2, 1, src_bits=32, dst_bits=16, src_plane_stride=4), le(-2, 0x12345)) == [(0, h("fffe" "2345"))]
    assert FT.flac_pack(desc(FT.FLAC_PACK, 2, 2, src_bits=32, dst_bits=24, src_plane_stride=8, dst_offset=9),
                        le(-0x800000, 1, 0x7F123456, -1)) == [(9, h("800000" "123456" "000001" "ffffff"))]
    with pytest.raises(FT.Unsupported):
        FT.flac_pack(desc(FT.FLAC_PACK, 2, 1, src_bits=32, dst_bits=32, src_plane_stride=4), le(1, 2))


def test_batch_bytes_and_totals():
    """Pieces land at their offsets, everything else keeps the fill; totals are spans, first byte to last."""
    src = bytes(range(1, 25))
    descs = [desc(FT.UNPACK_PLANAR, 2, 2, src_bits=16, dst_offset=2, dst_plane_stride=11),
             desc(FT.SENDER_PACK, 3, 2, src_bits=16, src_offset=8, dst_offset=24),
             desc(FT.FLAC_PACK, 2, 1, src_bits=32, dst_bits=16, src_offset=4, src_plane_stride=12, dst_offset=34),
             desc(FT.SENDER_PACK, 2, 0, src_bits=24, src_offset=1000, dst_offset=1000)]
    got = FT.batch_bytes(descs, src, 40, FILL)
    a5 = bytes([FILL])
    assert got == (a5 * 2 + bytes.fromhex("01020000" "05060000") + a5 * 3 + bytes.fromhex("03040000" "07080000") + a5 * 3
                   + bytes.fromhex("090a0b0c" "0f101112") + a5 * 2 + bytes.fromhex("0605" "1211") + a5 * 2)
    assert FT.totals(descs, src) == {"n_msgs": 4, "in_frames": 5, "out_frames": 5, "src_bytes_touched": 8 + 12 + 16,
                                     "dst_bytes_written": 19 + 8 + 4}


def test_golden_fixture():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_fmt_textbook_fixtures as G
    finally:
        sys.path.pop(0)
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx == G.fixture()
    kinds = set()
    for b in fx["batches"]:
        assert len(b["dst_sha256"]) == 64 and b["descriptors"] == len(b["kinds"])
        kinds |= set(b["kinds"])
        descs, src, dst_bytes = G.batches()[b["name"]]
        assert hashlib.sha256(FT.batch_bytes(descs, src, dst_bytes, fx["fill"])).hexdigest() == b["dst_sha256"]
    assert kinds == {FT.UNPACK_PLANAR, FT.SENDER_PACK, FT.FLAC_PACK}
    assert os.path.getsize(FIXTURE) < 8192
    assert subprocess.run([sys.executable, GENERATOR, "--check"], capture_output=True).returncode == 0
