"""The MPEG-4 container layer's host-only entry points: ohgpu_mp4_batch_check's refusals with their codes, and ohgpu_mp4_seek on a
hand-made sample table.  No device."""
import numpy as np
import pytest

from ohpipeline_amd import capi


def descs_of(*rows):
    d = np.zeros(len(rows), dtype=capi.MP4_STREAM_DESC)
    for x, (off, size, first, capacity) in zip(d, rows):
        x["src_offset"], x["src_bytes"], x["packet_first"], x["packet_capacity"] = off, size, first, capacity
    return d


def refused(descs, n_packets, src_bytes):
    with pytest.raises(capi.OhGpuError) as e:
        capi.mp4_batch_check(descs, n_packets, src_bytes)
    return e.value.code


def test_the_refusals_and_their_codes():
    good = descs_of((3, 1000, 0, 10), (1003, 500, 10, 5), (1503, 0, 15, 0))
    capi.mp4_batch_check(good, 15, 1503)

    def broken(field, i, value, n_packets=15, src_bytes=1503):
        d = good.copy()
        d[field][i] = value
        return refused(d, n_packets, src_bytes)

    assert broken("reserved", 1, 1) == capi.ERR_INVALID
    assert broken("flags", 0, 1) == capi.ERR_INVALID
    assert broken("src_bytes", 0, 1 << 31) == capi.ERR_INVALID
    assert broken("packet_first", 1, 9) == capi.ERR_INVALID                  # rows that overlap
    assert broken("packet_capacity", 1, 6) == capi.ERR_INVALID               # ... or run past the tables
    assert refused(good, 14, 1503) == capi.ERR_INVALID
    assert broken("src_offset", 1, 1004) == capi.ERR_BOUNDS                  # a range outside the source arena
    assert refused(good, 15, 1502) == capi.ERR_BOUNDS
    assert broken("src_offset", 2, 1504) == capi.ERR_BOUNDS                  # (an empty stream too lies inside the arena)
    capi.mp4_batch_check(np.zeros(0, dtype=capi.MP4_STREAM_DESC), 0, 0)      # the empty batch is legal


def test_the_seek_on_a_hand_made_table():
    table = np.zeros(5, dtype=capi.MP4_SAMPLE)
    table["first_frame"] = [0, 4096, 8192, 8192, 12288]
    table["frames"] = [4096, 4096, 0, 4096, 100]
    table["chunk"] = [0, 0, 1, 1, 2]
    assert capi.mp4_seek(table, 0) == (0, 0) and capi.mp4_seek(table, 4095) == (0, 0) and capi.mp4_seek(table, 4096) == (1, 4096)
    assert capi.mp4_seek(table, 8192) == (3, 8192)                           # not the row of no frames in front of it
    assert capi.mp4_seek(table, 12288 + 99) == (4, 12288)
    for frame in (12288 + 100, 1 << 40):
        with pytest.raises(capi.OhGpuError) as e:
            capi.mp4_seek(table, frame)
        assert e.value.code == capi.ERR_BOUNDS
    with pytest.raises(capi.OhGpuError) as e:
        capi.mp4_seek(np.zeros(0, dtype=capi.MP4_SAMPLE), 0)
    assert e.value.code == capi.ERR_BOUNDS
