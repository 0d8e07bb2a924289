"""The protected MPEG-4 layer's C ABI on the host alone (no device): the two struct sizes, ohgpu_cenc_batch_check's codes -- the sibling's
rules for the fields the families share, flags that must be OHGPU_MP4F_GATHER, unknown key flags, reserved words -- and ohgpu_cenc_head
against the model (tests/cenc_textbook.py, head_only and without a key) for every named file, good and malformed."""
import numpy as np
import pytest

import cenc_cases as CC
import cenc_textbook as CX
from ohpipeline_amd import capi


def test_the_struct_sizes_and_the_new_status():
    assert capi.CENC_STREAM_DESC.itemsize == 112 and capi.CENC_STREAM_RESULT.itemsize == 208
    assert capi.CENC_STREAM_DESC.fields["key_flags"][1] == 64 and capi.CENC_STREAM_DESC.fields["kid"][1] == 80 and capi.CENC_STREAM_DESC.fields["key"][1] == 96
    assert [capi.CENC_STREAM_RESULT.fields[k][1] for k in ("entry", "scheme", "is_protected", "iv_size", "kid", "blocks")] == [168, 172, 176, 177, 184, 200]
    assert capi.CENC_NO_KEY == 7 == CX.NO_KEY and capi.CENC_HAVE_KEY == 1 and capi.CENC_SCHEME == CX.code(b"cenc")
    header = open(capi.__file__.replace("ohpipeline_amd/capi.py", "include/ohgpu_cenc.h")).read()
    assert "#define OHGPU_CENC_NO_KEY    7u" in header and "typedef struct ohgpu_cenc_stream_desc {   /* 112 bytes */" in header and "/* 208 bytes */" in header


def descs(n=2):
    d = np.zeros(n, dtype=capi.CENC_STREAM_DESC)
    for i in range(n):
        d[i]["src_offset"], d[i]["src_bytes"], d[i]["codecs"], d[i]["flags"] = 1000 * i, 900, 3, 1
        d[i]["packet_first"], d[i]["packet_capacity"], d[i]["run_first"], d[i]["run_capacity"] = 10 * i, 10, 4 * i, 4
        d[i]["dst_offset"], d[i]["dst_capacity"], d[i]["key_flags"] = 500 * i, 500, i
    return d


def refused(d, code, **kw):
    with pytest.raises(capi.OhGpuError) as e:
        capi.cenc_batch_check(d, **dict(dict(n_packets=20, n_runs=8, src_arena_bytes=2000, dst_arena_bytes=1000), **kw))
    assert e.value.code == code, e.value


def test_a_good_batch_and_the_empty_batch_pass():
    capi.cenc_batch_check(descs(), 20, 8, 2000, 1000)
    capi.cenc_batch_check(np.zeros(0, dtype=capi.CENC_STREAM_DESC), 0, 0, 0, 0)


@pytest.mark.parametrize("field,value", [("reserved", (0, 1)), ("reserved2", (0, 0, 1)), ("flags", 0), ("flags", 3), ("key_flags", 2), ("codecs", 0), ("codecs", 4),
                                         ("src_bytes", 1 << 31), ("packet_first", 5), ("packet_capacity", 11), ("run_first", 3), ("run_capacity", 5), ("dst_offset", 499)])
def test_invalid_descriptors(field, value):
    d = descs()
    d[1][field] = value
    refused(d, capi.ERR_INVALID, src_arena_bytes=1 << 33)


@pytest.mark.parametrize("field,value", [("src_offset", 1101), ("dst_offset", 501)])
def test_ranges_outside_their_arenas(field, value):
    d = descs()
    d[1][field] = value
    refused(d, capi.ERR_BOUNDS)


def assert_head(data):
    got, want = capi.cenc_head(data), CX.demux(data, 3, 0, 0, head_only=True)
    for k in CX.RESULT_FIELDS:
        assert int(got["mp4f"][k]) == want[k], (k, got["mp4f"][k], want[k])
    for k in CX.CONFIG_FIELDS:
        assert int(got["mp4f"]["config"][k]) == want["config"][k]
    for k in CX.FLAC_FIELDS:
        assert (bytes(got["mp4f"]["flac"][k]) if k == "md5" else int(got["mp4f"]["flac"][k])) == want["flac"][k]
    for k in CX.EXTRA_FIELDS:
        assert (bytes(got[k]) if k == "kid" else int(got[k])) == want[k], k
    assert not got["pad"].any() and int(got["reserved"]) == 0
    return want


def test_the_head_of_every_named_file_needs_no_key():
    for name, m in CC.named_good().items():
        want = assert_head(m.data)
        assert want["status"] == CX.OK and want["samples"] == 0 and want["codec"] == CX.code(m.codec) and want["is_protected"] == (1 if m.protected else 0), name
        assert want["kid"] == (m.kid if want["entry"] == CX.code(b"enca") else bytes(16)), name
    statuses = set()
    for name, (data, status, at, codecs, have_key, kid) in CC.named_malformed().items():
        want = assert_head(data)
        statuses.add(want["status"])
        assert want["status"] != CX.NO_KEY and (status != CX.NO_KEY or (want["status"], want["kid"], want["is_protected"]) == (CX.OK, CC.KID, 1)), name
    assert statuses >= {CX.OK, CX.INVALID, CX.NOT_CODEC, CX.UNSUPPORTED}


def test_the_head_of_a_file_cut_anywhere_in_its_protection_boxes():
    m = CC.named_good()["alac_iv16"]
    for data in CC.protection_cuts(m):
        if len(data) <= m.init_bytes + 1:
            assert_head(data)
    assert_head(b"")
    with pytest.raises(capi.OhGpuError):
        capi.check(capi.lib().ohgpu_cenc_head(None, 4, None))


def test_the_library_exports_what_the_header_declares():
    """tests/test_capi_loads.py's check, for include/ohgpu_cenc.h and capi.CENC_SYMBOLS; and ohgpu.h brings the header along"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ohgpu_cenc.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ohgpu_[a-z0-9_]+)\s*\(", text)))
    assert len(names) == 13 and sorted(capi.CENC_SYMBOLS) == names and not set(names) & set(capi.SYMBOLS)
    for n in names:
        assert hasattr(capi.lib(), n), n
    assert '#include "ohgpu_cenc.h"' in open(os.path.join(root, "include", "ohgpu.h")).read()
