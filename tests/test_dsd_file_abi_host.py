"""The DSD file layer's host-only entry points: the struct sizes the header states against the numpy dtypes, every refusal of
ohgpu_dsd_file_batch_check with its code, ohgpu_dsd_file_head against the model for every named file and every prefix of them, and
ohgpu_dsd_file_seek's rounding.  No device."""
import os
import re

import numpy as np
import pytest

import dsd_file_cases as FC
import dsd_file_textbook as FX
from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_struct_sizes_the_header_states():
    text = open(os.path.join(ROOT, "include", "ohgpu.h")).read()
    for name, dtype, size in (("ohgpu_dsd_file_stream_desc", capi.DSD_FILE_STREAM_DESC, 64), ("ohgpu_dsd_file_stream_result", capi.DSD_FILE_STREAM_RESULT, 96)):
        stated = re.search(r"typedef struct %s \{\s*/\* (\d+) bytes \*/" % name, text)
        assert stated and int(stated.group(1)) == dtype.itemsize == size
        body = text[stated.end():text.index("} %s;" % name)]
        fields = [f for line in body.splitlines() for f in re.findall(r"^\s*uint(?:32|64)_t\s+(\w+)", line)]
        assert fields == list(dtype.names)                                               # the same fields in the same order
    assert list(capi.DSD_FILE_STREAM_RESULT.names) == list(FX.FIELDS)
    for name in ("OK", "NOT_DSD", "TRUNCATED", "INVALID", "UNSUPPORTED", "KIND_DSF", "KIND_DFF", "MAX_CHUNKS"):
        assert int(re.search(r"#define OHGPU_DSD_FILE_%s\s+(\d+)u" % name, text).group(1)) == getattr(capi, "DSD_FILE_" + name)
    assert (capi.DSD_FILE_KIND_DSF, capi.DSD_FILE_KIND_DFF, capi.DSD_FILE_MAX_CHUNKS) == (FX.DSF, FX.DFF, FX.MAX_CHUNKS)
    assert (capi.DSD_FILE_OK, capi.DSD_FILE_NOT_DSD, capi.DSD_FILE_TRUNCATED, capi.DSD_FILE_INVALID, capi.DSD_FILE_UNSUPPORTED) == \
        (FX.OK, FX.NOT_DSD, FX.TRUNCATED, FX.INVALID, FX.UNSUPPORTED)


def descs_of(*rows):
    d = np.zeros(len(rows), dtype=capi.DSD_FILE_STREAM_DESC)
    for x, (off, size, dst, room) in zip(d, rows):
        x["src_offset"], x["src_bytes"], x["dst_offset"], x["dst_bytes_capacity"], x["sample_block_words"], x["pad_bytes_per_chunk"] = off, size, dst, room, 6, 2
    return d


def refused(descs, src_bytes, dst_bytes):
    with pytest.raises(capi.OhGpuError) as e:
        capi.dsd_file_batch_check(descs, src_bytes, dst_bytes)
    return e.value.code


def test_the_refusals_and_their_codes():
    good = descs_of((3, 1000, 16, 400), (1003, 500, 416, 584), (1503, 0, 1008, 0))
    capi.dsd_file_batch_check(good, 1503, 1008)

    def broken(field, i, value, src_bytes=1503, dst_bytes=1008):
        d = good.copy()
        d[field][i] = value
        return refused(d, src_bytes, dst_bytes)

    assert broken("reserved", 1, 1) == capi.ERR_INVALID
    d = good.copy()
    d["reserved"][2][3] = 7
    assert refused(d, 1503, 1008) == capi.ERR_INVALID
    assert broken("flags", 0, 1) == capi.ERR_INVALID
    for W, P in ((0, 0), (256, 0), (6, 4), (6, 1), (7, 3), (8, 2), (4, 2)):              # what ohgpu_dsd_desc refuses
        d = good.copy()
        d["sample_block_words"][1], d["pad_bytes_per_chunk"][1] = W, P
        assert refused(d, 1503, 1008) == capi.ERR_INVALID, (W, P)
    for W, P in FC.FORMATS + ((255, 0), (12, 8)):
        d = good.copy()
        d["sample_block_words"][1], d["pad_bytes_per_chunk"][1] = W, P
        capi.dsd_file_batch_check(d, 1503, 1008)
    assert broken("src_bytes", 0, 1 << 31) == capi.ERR_INVALID
    for off in (17, 24, 31):
        assert broken("dst_offset", 0, off) == capi.ERR_INVALID                          # no multiple of 16
    assert broken("dst_offset", 1, 400) == capi.ERR_INVALID                              # destination ranges that overlap
    assert broken("dst_bytes_capacity", 0, 401) == capi.ERR_INVALID
    assert broken("src_offset", 1, 1004) == capi.ERR_BOUNDS                              # a range outside the source arena
    assert refused(good, 1502, 1008) == capi.ERR_BOUNDS
    assert broken("src_offset", 2, 1504) == capi.ERR_BOUNDS                              # (an empty stream too lies inside the arena)
    assert broken("dst_offset", 1, 432) == capi.ERR_BOUNDS                               # ... or the destination arena
    assert refused(good, 1503, 1007) == capi.ERR_BOUNDS
    assert broken("dst_offset", 2, 1024) == capi.ERR_BOUNDS
    capi.dsd_file_batch_check(np.zeros(0, dtype=capi.DSD_FILE_STREAM_DESC), 0, 0)        # the empty batch is legal
    sources_may_overlap = descs_of((0, 1000, 0, 400), (0, 1000, 400, 400))
    capi.dsd_file_batch_check(sources_may_overlap, 1000, 800)


def same_as_model(data, W, P):
    r, m = capi.dsd_file_head(data, W, P), FX.read(data, W, P)
    got = {k: int(r[k]) for k in FX.FIELDS}
    assert got == {k: m[k] for k in FX.FIELDS}, (got, {k: m[k] for k in FX.FIELDS})
    return m


def test_the_head_is_the_model_for_every_named_file():
    good, bad = FC.named_good(), FC.named_malformed()
    for k, w in enumerate(good.values()):
        for W, P in FC.FORMATS:
            assert same_as_model(w.data, W, P)["status"] == FX.OK
    for name, (data, status, at) in bad.items():
        m = same_as_model(data, 6, 2)
        assert (m["status"], m["error_offset"]) == (status, at), name


def test_the_head_is_the_model_for_every_prefix_round_every_header_boundary():
    statuses = set()
    for k, w in enumerate(FC.named_good().values()):
        for n, data in enumerate(FC.cuts(w)):
            statuses.add(same_as_model(data, *FC.FORMATS[(k + n) % 4])["status"])
    assert statuses == {FX.OK, FX.NOT_DSD, FX.TRUNCATED}


def test_the_heads_own_refusals():
    with pytest.raises(capi.OhGpuError) as e:
        capi.dsd_file_head(b"DSD " + bytes(100), 6, 4)
    assert e.value.code == capi.ERR_INVALID
    res = np.zeros(1, dtype=capi.DSD_FILE_STREAM_RESULT)
    assert capi.lib().ohgpu_dsd_file_head(None, 0, 2, 0, None) == capi.ERR_INVALID
    assert capi.lib().ohgpu_dsd_file_head(None, 5, 2, 0, res.ctypes.data) == capi.ERR_INVALID
    assert capi.lib().ohgpu_dsd_file_head(res.ctypes.data, 1 << 31, 2, 0, res.ctypes.data) == capi.ERR_INVALID
    assert int(capi.dsd_file_head(b"", 2, 0)["status"]) == FX.NOT_DSD


def test_the_seeks_rounding():
    for kind in (FX.DSF, FX.DFF):
        for sample in (0, 1, 32767, 32768, 2047, 2048, 32769, 65535, 65536, (1 << 40) + 12345):
            assert capi.dsd_file_seek(kind, sample) == FX.seek(kind, sample), (kind, sample)
    assert [capi.dsd_file_seek(FX.DSF, s) for s in (0, 1, 32767, 32768, 2047, 2048)] == [(0, 0), (0, 0), (0, 0), (2048, 32768), (0, 0), (0, 0)]
    assert [capi.dsd_file_seek(FX.DFF, s) for s in (0, 1, 32767, 32768, 2047, 2048)] == [(0, 0), (0, 0), (1920, 30720), (2048, 32768), (0, 0), (128, 2048)]
    for kind in (0, 1, 4):
        with pytest.raises(capi.OhGpuError) as e:
            capi.dsd_file_seek(kind, 5)
        assert e.value.code == capi.ERR_INVALID
