"""tests/dsd_textbook.py (the model the device's DSD kernels are held to, tests/test_gpu_dsd_textbook.py) against a second,
independent statement of the same format -- bit reversal by a table, chunks assembled by np.stack / reshape where the model loops
-- and against the worked bytes of its docstring; ohgpu_dsd_layout (host only) against the model's sizes and refusals; the
descriptor's layout against the header; the fixture against its generator.  No device is needed."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dsd_textbook as DT
from ohpipeline_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ACCEPTED = [(W, 0) for W in (1, 2, 3, 4, 5, 16, 255)] + [(P + 4, P) for P in (2, 4, 6, 8, 250)]
REFUSED = [(0, 0), (6, 1), (7, 3), (6, 4), (8, 2), (4, 2), (5, 2), (3, 2), (9, 4), (16, 4), (2, 2), (1, 2), (12, 6), (255, 250)]
TABLE = np.array([int(f"{v:08b}"[::-1], 2) for v in range(256)], dtype=np.uint8)    # reversal by reading the digits backwards


def second_statement(kind, W, P, src, n, silence=False):
    """The same conversion, vectorised: (n, 4) arrays of (l0, l1, r0, r1), padded by np.concatenate, tail by np.full."""
    per_block = (W * 4) // (4 + P)
    total = -(-n // per_block) * W * 4
    if silence:
        return np.full(total, 0x69, np.uint8).tobytes()
    s = np.frombuffer(src, dtype=np.uint8)
    if kind == DT.PASS:
        body = s[:n * (4 + P)]
    else:
        if kind == DT.DSF:
            planes = s[:-(-n // 2048) * 8192].reshape(-1, 2, 4096)          # (pair, channel, byte)
            left, right = planes[:, 0, :].reshape(-1), planes[:, 1, :].reshape(-1)
            lr = np.stack([TABLE[left[:2 * n]].reshape(n, 2), TABLE[right[:2 * n]].reshape(n, 2)], axis=1)     # (chunk, channel, byte)
        elif kind == DT.DFF:
            lr = s[:4 * n].reshape(n, 2, 2).transpose(0, 2, 1)              # (chunk, byte, channel) -> (chunk, channel, byte)
        else:
            lr = s[:4 * n].reshape(n, 2, 2)
        pad = np.zeros((n, 2, P // 2), np.uint8)
        body = np.concatenate([pad, lr], axis=2).reshape(-1)
    return np.concatenate([body, np.full(total - body.size, 0x69, np.uint8)]).tobytes()


def test_bit_reversal_against_a_table():
    assert [DT.reverse_bits(v) for v in range(256)] == TABLE.tolist()
    assert DT.reverse_bits(0x01) == 0x80 and DT.reverse_bits(0x83) == 0xC1 and DT.reverse_bits(0x69) == 0x96


def test_worked_bytes():
    for kind, W, P, src, n, want in DT.WORKED:
        if kind == DT.DSF:
            src = DT.dsf_image(*src)
        assert b"".join(bytes(DT.chunk_bytes(kind, P, src, j)) for j in range(n)) == want, (kind, W, P)    # (one Raw chunk is no whole block)
        if kind != DT.RAW:
            assert DT.convert(kind, W, P, src, n)[:len(want)] == want, (kind, W, P)
        assert second_statement(kind, W, P, src, n)[:len(want)] == want, (kind, W, P)
    rng = np.random.default_rng(1)
    for kind in (DT.DSF, DT.DFF):                                           # five chunks at (6, 2): 30 bytes, then 18 of 0x69
        src = rng.bytes(8192)
        out = DT.convert(kind, 6, 2, src, 5)
        assert len(out) == 48 and out[30:] == b"\x69" * 18 and out[:30] == DT.convert(kind, 6, 2, src, 8)[:30]
    assert DT.convert(DT.RAW, 6, 2, b"", 8, silence=True) == b"\x69" * 48
    assert DT.convert(DT.PASS, 6, 2, bytes(range(48)), 8) == bytes(range(48))


@pytest.mark.parametrize("kind", [DT.PASS, DT.DSF, DT.DFF, DT.RAW])
def test_model_against_the_second_statement(kind):
    rng = np.random.default_rng(100 + kind)
    for (W, P), k in itertools.product(ACCEPTED, range(4)):
        per_block = W - P
        n = per_block * int(rng.integers(0, 40)) if k < 2 else int(rng.integers(0, 5000))
        if kind in (DT.RAW, DT.PASS):
            n -= n % per_block
        src = rng.bytes(DT.layout(kind, W, P, n)[0])
        assert DT.convert(kind, W, P, src, n) == second_statement(kind, W, P, src, n), (kind, W, P, n)
    assert DT.convert(kind, 8, 4, b"", 12, silence=True) == second_statement(kind, 8, 4, b"", 12, silence=True) == b"\x69" * 96


def test_dsf_runs_cross_block_pairs():
    """Chunk 2047 is the last of pair 0, chunk 2048 the first of pair 1: its left bytes lie 8192 into the file."""
    src = bytearray(3 * 8192)
    src[4094], src[4095], src[8190], src[8191] = 0x01, 0x02, 0x03, 0x04     # pair 0: the last two bytes of each plane
    src[8192], src[8193], src[8192 + 4096], src[8192 + 4097] = 0x10, 0x20, 0x30, 0x40
    out = DT.convert(DT.DSF, 1, 0, bytes(src), 4100)
    assert out[4 * 2047:4 * 2047 + 4] == bytes([0x80, 0x40, 0xC0, 0x20]) and out[4 * 2048:4 * 2048 + 4] == bytes([0x08, 0x04, 0x0C, 0x02])
    assert DT.layout(DT.DSF, 1, 0, 2048)[0] == 8192 and DT.layout(DT.DSF, 1, 0, 2049)[0] == 16384 and DT.layout(DT.DSF, 1, 0, 0)[0] == 0


def test_layout_call_against_the_model():
    """ohgpu_dsd_layout: sizes for every accepted (W, P), kind and a range of chunk counts; refusals where the model refuses."""
    for (W, P), kind in itertools.product(ACCEPTED, (DT.PASS, DT.DSF, DT.DFF, DT.RAW)):
        per_block = W - P
        for n in sorted({0, 1, per_block - 1, per_block, per_block + 1, 7 * per_block, 2047, 2048, 2049, 4096, 12 * per_block * 2048 + 3 * per_block}):
            try:
                want = DT.layout(kind, W, P, n)
            except DT.Refused:
                want = None
            if want is None:
                with pytest.raises(capi.OhGpuError) as e:
                    capi.dsd_layout(kind, W, P, n)
                assert e.value.code == capi.ERR_INVALID
                assert kind in (DT.RAW, DT.PASS) and n % per_block
            else:
                assert capi.dsd_layout(kind, W, P, n) == want, (kind, W, P, n)
    for (W, P), kind in itertools.product(REFUSED, (DT.PASS, DT.DSF, DT.DFF, DT.RAW)):
        with pytest.raises(DT.Refused):
            DT.layout(kind, W, P, 0)
        with pytest.raises(capi.OhGpuError) as e:
            capi.dsd_layout(kind, W, P, 0)
        assert e.value.code == capi.ERR_INVALID, (W, P)
    for kind in (0, 5, 255):
        with pytest.raises(capi.OhGpuError) as e:
            capi.dsd_layout(kind, 6, 2, 4)
        assert e.value.code == capi.ERR_INVALID
    assert capi.lib().ohgpu_dsd_layout(DT.DFF, 6, 2, 5, None, None) == capi.OK     # (either result may be left out)
    assert (capi.DSD_PASS, capi.DSD_DSF, capi.DSD_DFF, capi.DSD_RAW, capi.DSD_FLAG_SILENCE, capi.DSD_SILENCE_BYTE) == \
           (DT.PASS, DT.DSF, DT.DFF, DT.RAW, DT.FLAG_SILENCE, DT.SILENCE)


def test_descriptor_layout_matches_header(tmp_path):
    names = ("src_offset", "dst_offset", "n_chunks", "kind", "flags", "sample_block_words", "pad_bytes_per_chunk", "reserved")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\nint main(){printf("%zu %d %d %d %d %d %d ' + "%zu " * len(names) + '\\n", '
                   'sizeof(ohgpu_dsd_desc), OHGPU_DSD_PASS, OHGPU_DSD_DSF, OHGPU_DSD_DFF, OHGPU_DSD_RAW, (int)OHGPU_DSD_FLAG_SILENCE, OHGPU_DSD_SILENCE_BYTE, '
                   + ", ".join(f"offsetof(ohgpu_dsd_desc, {n})" for n in names) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == capi.DSD_DESC.itemsize == 32
    assert out[1:7] == [capi.DSD_PASS, capi.DSD_DSF, capi.DSD_DFF, capi.DSD_RAW, capi.DSD_FLAG_SILENCE, capi.DSD_SILENCE_BYTE] == [1, 2, 3, 4, 1, 0x69]
    assert out[7:] == [capi.DSD_DESC.fields[n][1] for n in names] == [0, 8, 16, 20, 21, 22, 23, 24]
    assert capi.lib().ohgpu_abi_version() == 1


def test_calls_refuse_without_a_context():
    """No context, no device: every DSD entry point answers OHGPU_ERR_INVALID and says why, and starts nothing."""
    L = capi.lib()
    d = np.zeros(1, dtype=capi.DSD_DESC)
    b = C.c_void_p()
    assert L.ohgpu_dsd_batch_create(None, d.ctypes.data_as(C.c_void_p), 1, 0, 0, C.byref(b)) == capi.ERR_INVALID
    assert b"null context" in L.ohgpu_last_error() and not b.value
    assert L.ohgpu_dsd_batch_run(None, None, None, None, None) == capi.ERR_INVALID
    assert L.ohgpu_dsd_process_host(None, d.ctypes.data_as(C.c_void_p), 1, None, 0, None, 0) == capi.ERR_INVALID
    assert L.ohgpu_dsd_batch_paths(None, None, None, None) == capi.ERR_INVALID
    assert b"not a DSD batch" in L.ohgpu_last_error()


def test_fixture_is_what_the_model_gives():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_dsd_textbook_fixtures as G
    finally:
        sys.path.pop(0)
    with open(G.OUT) as f:
        assert f.read() == G.text(G.fixture())
    fx = json.load(open(G.OUT))
    assert len(fx["batches"]) == 3 and os.path.getsize(G.OUT) < 16384
    for entry in fx["batches"]:                                             # ... and the second statement agrees with every head
        descs, src, _ = G.batches()[entry["name"]]
        for d, head in zip(descs, entry["heads"]):
            sil = bool(d["flags"])
            need = DT.layout(d["kind"], d["sample_block_words"], d["pad_bytes_per_chunk"], d["n_chunks"], sil)[0]
            out = second_statement(d["kind"], d["sample_block_words"], d["pad_bytes_per_chunk"], src[d["src_offset"]:d["src_offset"] + need], d["n_chunks"], sil)
            assert out[:len(bytes.fromhex(head))].hex() == head
