"""The PCM file layer's host-only entry point: the struct sizes the header states against the numpy dtypes, and every refusal of
ohgpu_iff_batch_check with its code.  No device."""
import os
import re

import numpy as np
import pytest

from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_struct_sizes_the_header_states():
    text = open(os.path.join(ROOT, "include", "ohgpu.h")).read()
    for name, dtype in (("ohgpu_iff_stream_desc", capi.IFF_STREAM_DESC), ("ohgpu_iff_stream_result", capi.IFF_STREAM_RESULT)):
        stated = re.search(r"typedef struct %s \{\s*/\* (\d+) bytes \*/" % name, text)
        assert stated and int(stated.group(1)) == dtype.itemsize
        body = text[stated.end():text.index("} %s;" % name)]
        fields = [f for line in body.splitlines() for f in re.findall(r"^\s*uint(?:32|64)_t\s+(\w+)", line)]
        assert fields == list(dtype.names)                                               # the same fields in the same order
    for name in ("OK", "NOT_IFF", "TRUNCATED", "INVALID", "UNSUPPORTED", "KIND_WAV", "KIND_AIFF", "KIND_AIFC", "MAX_CHUNKS", "MAX_CHANNELS", "MAX_FRAME_BYTES",
                 "FLAG_WAV8_UNSIGNED"):
        assert int(re.search(r"#define OHGPU_IFF_%s\s+(\d+)u" % name, text).group(1)) == getattr(capi, "IFF_" + name)


def descs_of(*rows):
    d = np.zeros(len(rows), dtype=capi.IFF_STREAM_DESC)
    for x, (off, size, dst, frames, room) in zip(d, rows):
        x["src_offset"], x["src_bytes"], x["dst_offset"], x["dst_frame_capacity"], x["dst_bytes_capacity"], x["max_bit_depth"] = off, size, dst, frames, room, 24
    return d


def refused(descs, src_bytes, dst_bytes):
    with pytest.raises(capi.OhGpuError) as e:
        capi.iff_batch_check(descs, src_bytes, dst_bytes)
    return e.value.code


def test_the_refusals_and_their_codes():
    good = descs_of((3, 1000, 5, 10, 400), (1003, 500, 405, 100, 595), (1503, 0, 1000, 0, 0))
    capi.iff_batch_check(good, 1503, 1000)

    def broken(field, i, value, src_bytes=1503, dst_bytes=1000):
        d = good.copy()
        d[field][i] = value
        return refused(d, src_bytes, dst_bytes)

    assert broken("reserved", 1, 1) == capi.ERR_INVALID
    d = good.copy()
    d["reserved"][2][3] = 7
    assert refused(d, 1503, 1000) == capi.ERR_INVALID
    assert broken("flags", 0, 2) == capi.ERR_INVALID
    assert broken("flags", 0, 3) == capi.ERR_INVALID
    d = good.copy()
    d["flags"][0] = capi.IFF_FLAG_WAV8_UNSIGNED
    capi.iff_batch_check(d, 1503, 1000)
    for depth in (0, 16, 23, 25, 33):
        assert broken("max_bit_depth", 1, depth) == capi.ERR_INVALID
    d = good.copy()
    d["max_bit_depth"][1] = 32
    capi.iff_batch_check(d, 1503, 1000)
    assert broken("src_bytes", 0, 1 << 31) == capi.ERR_INVALID
    assert broken("dst_bytes_capacity", 0, 401) == capi.ERR_INVALID          # more than dst_frame_capacity x 40
    assert broken("dst_frame_capacity", 0, 9) == capi.ERR_INVALID
    assert broken("dst_offset", 1, 404) == capi.ERR_INVALID                  # destination ranges that overlap
    assert broken("dst_offset", 0, 6) == capi.ERR_INVALID
    assert broken("src_offset", 1, 1004) == capi.ERR_BOUNDS                  # a range outside the source arena
    assert refused(good, 1502, 1000) == capi.ERR_BOUNDS
    assert broken("src_offset", 2, 1504) == capi.ERR_BOUNDS                  # (an empty stream too lies inside the arena)
    assert broken("dst_offset", 1, 406) == capi.ERR_BOUNDS                   # ... or the destination arena
    assert refused(good, 1503, 999) == capi.ERR_BOUNDS
    assert broken("dst_offset", 2, 1001) == capi.ERR_BOUNDS
    capi.iff_batch_check(np.zeros(0, dtype=capi.IFF_STREAM_DESC), 0, 0)      # the empty batch is legal
    sources_may_overlap = descs_of((0, 1000, 0, 10, 400), (0, 1000, 400, 10, 400))
    capi.iff_batch_check(sources_may_overlap, 1000, 800)
