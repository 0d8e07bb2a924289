"""The second protected MPEG-4 family's C ABI on the host alone (no device): the two struct sizes and their offsets, ohgpu_cbcs_batch_check's
codes -- the sibling's rules for the fields the families share, and the shares of the subsample table --, ohgpu_cbcs_head against the model
(tests/cbcs_textbook.py, head_only and without a key) for every named file, good and malformed, and the header against the exports."""
import os
import re

import numpy as np
import pytest

import cbcs_cases as BC
import cbcs_textbook as BX
from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_struct_sizes_and_offsets():
    assert capi.CBCS_STREAM_DESC.itemsize == 120 and capi.CBCS_STREAM_RESULT.itemsize == 232
    assert [capi.CBCS_STREAM_DESC.fields[k][1] for k in ("key_flags", "kid", "key", "subsample_first", "subsample_capacity")] == [64, 80, 96, 112, 116]
    assert [capi.CBCS_STREAM_RESULT.fields[k][1] for k in ("cenc", "crypt_blocks", "skip_blocks", "constant_iv_size", "pad", "subsamples", "constant_iv")] == [0, 208, 209, 210, 211, 212, 216]
    assert capi.CBCS_SCHEME_CENC == BX.code(b"cenc") and capi.CBCS_SCHEME_CBCS == BX.code(b"cbcs")
    header = open(os.path.join(ROOT, "include", "ohgpu_cbcs.h")).read()
    assert "typedef struct ohgpu_cbcs_stream_desc {   /* 120 bytes */" in header and "typedef struct ohgpu_cbcs_stream_result {   /* 232 bytes */" in header
    assert "#define OHGPU_CBCS_SCHEME_CBCS  0x63626373u" in header


def descs(n=2):
    d = np.zeros(n, dtype=capi.CBCS_STREAM_DESC)
    for i in range(n):
        d[i]["src_offset"], d[i]["src_bytes"], d[i]["codecs"], d[i]["flags"] = 1000 * i, 900, 3, 1
        d[i]["packet_first"], d[i]["packet_capacity"], d[i]["run_first"], d[i]["run_capacity"] = 10 * i, 10, 4 * i, 4
        d[i]["dst_offset"], d[i]["dst_capacity"], d[i]["key_flags"] = 500 * i, 500, i
        d[i]["subsample_first"], d[i]["subsample_capacity"] = 6 * i, 6
    return d


def refused(d, code, **kw):
    with pytest.raises(capi.OhGpuError) as e:
        capi.cbcs_batch_check(d, **dict(dict(n_packets=20, n_runs=8, n_subsamples=12, src_arena_bytes=2000, dst_arena_bytes=1000), **kw))
    assert e.value.code == code, e.value


def test_a_good_batch_and_the_empty_batch_pass():
    capi.cbcs_batch_check(descs(), 20, 8, 12, 2000, 1000)
    capi.cbcs_batch_check(np.zeros(0, dtype=capi.CBCS_STREAM_DESC), 0, 0, 0, 0, 0)
    d = descs()
    d[0]["subsample_capacity"] = d[1]["subsample_capacity"] = 0          # (a stream with no share may name any row of the table, its end included)
    d[1]["subsample_first"] = 12
    capi.cbcs_batch_check(d, 20, 8, 12, 2000, 1000)


@pytest.mark.parametrize("field,value", [("reserved", (0, 1)), ("reserved2", (0, 0, 1)), ("flags", 0), ("flags", 3), ("key_flags", 2), ("codecs", 0), ("codecs", 4),
                                         ("src_bytes", 1 << 31), ("packet_first", 5), ("packet_capacity", 11), ("run_first", 3), ("run_capacity", 5), ("dst_offset", 499),
                                         ("subsample_first", 5), ("subsample_first", 7), ("subsample_capacity", 7), ("subsample_first", 0xffffffff)])
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
    got, want = capi.cbcs_head(data), BX.demux(data, 3, 0, 0, head_only=True)
    for k in BX.RESULT_FIELDS:
        assert int(got["cenc"]["mp4f"][k]) == want[k], (k, got["cenc"]["mp4f"][k], want[k])
    for k in BX.CONFIG_FIELDS:
        assert int(got["cenc"]["mp4f"]["config"][k]) == want["config"][k]
    for k in BX.FLAC_FIELDS:
        assert (bytes(got["cenc"]["mp4f"]["flac"][k]) if k == "md5" else int(got["cenc"]["mp4f"]["flac"][k])) == want["flac"][k]
    for k in BX.EXTRA_FIELDS:
        assert (bytes(got["cenc"][k]) if k == "kid" else int(got["cenc"][k])) == want[k], k
    for k in BX.MORE_FIELDS:
        assert (bytes(got[k]) if k == "constant_iv" else int(got[k])) == want[k], k
    assert not got["cenc"]["pad"].any() and int(got["cenc"]["reserved"]) == 0 and int(got["pad"]) == 0
    return want


def test_the_head_of_every_named_file_needs_no_key():
    seen = set()
    for name, m in BC.named_good().items():
        want = assert_head(m.data)
        assert want["status"] == BX.OK and want["samples"] == 0 and want["subsamples"] == 0 and want["is_protected"] == (1 if m.protected else 0), name
        if m.protected:
            assert (want["crypt_blocks"], want["skip_blocks"]) == m.pattern and want["scheme"] == BX.code(m.scheme) and want["kid"] == m.kid, name
            seen.add((want["iv_size"], want["constant_iv_size"]))
    assert seen == {(8, 0), (16, 0), (0, 8), (0, 16)}
    statuses = set()
    for name, (data, status, at, codecs, have_key, kid) in BC.named_malformed().items():
        want = assert_head(data)
        statuses.add(want["status"])
        assert want["status"] != BX.NO_KEY, name
        if data.find(b"moof") < 0 and status != BX.NO_KEY:               # (an initialisation segment alone: the head is the whole answer)
            assert (want["status"], want["error_offset"]) == (status, at), name
    assert statuses == {BX.OK, BX.INVALID, BX.UNSUPPORTED}


def test_the_head_of_a_file_cut_anywhere_in_its_tenc():
    m = BC.named_good()["cbcs_1_9_constant_iv16_no_senc"]
    tenc = BC.at_of(m.data, b"tenc")
    for cut in range(tenc, tenc + 8 + 41 + 1):
        assert_head(m.data[:cut])
    assert_head(b"")
    with pytest.raises(capi.OhGpuError):
        capi.check(capi.lib().ohgpu_cbcs_head(None, 4, None))


def test_the_sibling_family_still_refuses_what_this_one_serves():
    """ohgpu_cenc_* answers as before: cbcs, tenc version 1 and a senc of entries stay UNSUPPORTED there"""
    good = BC.named_good()
    for name in ("cbcs_whole_samples_iv16", "cbcs_pattern_1_9", "cbcs_1_9_constant_iv16_no_senc"):
        got = capi.cenc_head(good[name].data)
        assert int(got["mp4f"]["status"]) == BX.UNSUPPORTED and int(got["mp4f"]["error_offset"]) == BC.at_of(good[name].data, b"schm"), name


def test_the_library_exports_what_the_header_declares():
    """tests/test_capi_loads.py's check, for include/ohgpu_cbcs.h and capi.CBCS_SYMBOLS; and ohgpu.h brings the header along"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ohgpu_cbcs.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ohgpu_[a-z0-9_]+)\s*\(", text)))
    assert len(names) == 13 and sorted(capi.CBCS_SYMBOLS) == names and not set(names) & (set(capi.SYMBOLS) | set(capi.CENC_SYMBOLS))
    assert [n.replace("ohgpu_cbcs_", "") for n in names] == [n.replace("ohgpu_cenc_", "") for n in sorted(capi.CENC_SYMBOLS)]      # the family mirrors the sibling one for one
    for n in names:
        assert hasattr(capi.lib(), n), n
    assert '#include "ohgpu_cbcs.h"' in open(os.path.join(ROOT, "include", "ohgpu.h")).read()
