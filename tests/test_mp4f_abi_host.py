"""ohgpu_mp4f_batch_check's codes and ohgpu_mp4f_head against the model, on the host alone (no device): reserved words, unknown flags
and codecs, src_bytes of 2^31, row / run / gather ranges that overlap or leave their tables or arenas; and the head of every named
file -- good, malformed, and cut inside its moov -- as tests/mp4f_textbook.py reads it with head_only."""
import numpy as np
import pytest

import mp4f_cases as FC
import mp4f_textbook as FX
from ohpipeline_amd import capi


def descs(n=2):
    d = np.zeros(n, dtype=capi.MP4F_STREAM_DESC)
    for i in range(n):
        d[i]["src_offset"], d[i]["src_bytes"], d[i]["codecs"], d[i]["flags"] = 1000 * i, 900, 3, 1
        d[i]["packet_first"], d[i]["packet_capacity"], d[i]["run_first"], d[i]["run_capacity"] = 10 * i, 10, 4 * i, 4
        d[i]["dst_offset"], d[i]["dst_capacity"] = 500 * i, 500
    return d


def check(d, n_packets=20, n_runs=8, src=2000, dst=1000):
    capi.mp4f_batch_check(d, n_packets, n_runs, src, dst)


def refused(d, code, **kw):
    with pytest.raises(capi.OhGpuError) as e:
        check(d, **kw)
    assert e.value.code == code, e.value


def test_a_good_batch_and_the_empty_batch_pass():
    check(descs())
    check(np.zeros(0, dtype=capi.MP4F_STREAM_DESC), 0, 0, 0, 0)


@pytest.mark.parametrize("field,value", [("reserved", (0, 1)), ("flags", 2), ("flags", 0x80000001), ("codecs", 0), ("codecs", 4), ("src_bytes", 1 << 31),
                                         ("packet_first", 5), ("packet_capacity", 11), ("run_first", 3), ("run_capacity", 5), ("dst_offset", 499)])
def test_invalid_descriptors(field, value):
    d = descs()
    d[1][field] = value
    refused(d, capi.ERR_INVALID, src=1 << 33)


@pytest.mark.parametrize("field,value", [("src_offset", 1101), ("dst_offset", 501)])
def test_ranges_outside_their_arenas(field, value):
    d = descs()
    d[1][field] = value
    refused(d, capi.ERR_BOUNDS)


def test_what_is_not_gathered_needs_no_room():
    d = descs()
    d["flags"] = 0
    d["dst_offset"] = 1 << 40
    check(d)
    d["packet_capacity"] = d["run_capacity"] = 0           # ... and a stream without rows has no range to overlap
    d["packet_first"] = d["run_first"] = 1 << 30
    check(d)


def model_head(data):
    return FX.demux(data, 3, 0, 0, head_only=True)


def assert_head(data):
    got, want = capi.mp4f_head(data), model_head(data)
    for k in FX.RESULT_FIELDS:
        assert int(got[k]) == want[k], (k, got[k], want[k])
    for k in FX.CONFIG_FIELDS:
        assert int(got["config"][k]) == want["config"][k]
    for k in FX.FLAC_FIELDS:
        assert (bytes(got["flac"][k]) if k == "md5" else int(got["flac"][k])) == want["flac"][k]
    return want


def test_the_head_of_every_named_file():
    for name, m in FC.named_good().items():
        want = assert_head(m.data)
        assert want["status"] == FX.OK and want["samples"] == 0 and want["codec"] == FX.code(m.codec), name
        assert_head(m.data[:m.init_bytes])
    statuses = set()
    for name, (data, status, at, codecs) in FC.named_malformed().items():
        statuses.add(assert_head(data)["status"])
    assert statuses >= {FX.OK, FX.NOT_MP4, FX.TRUNCATED, FX.INVALID, FX.NOT_CODEC, FX.UNSUPPORTED, FX.NOT_FRAGMENTED}


def test_the_head_of_a_file_cut_anywhere_in_its_moov():
    m = FC.flac_file("s16_stereo_44k1_b1152_l5")
    want = assert_head(m.data)
    assert want["flac"]["md5"] == m.fixture.data[26:42] and want["flac"]["total_samples"] == m.info["total_samples"] and want["duration"] == m.info["total_samples"]
    for data in FC.cuts(m):
        if len(data) <= m.init_bytes + 1:
            assert_head(data)
    assert_head(b"")
