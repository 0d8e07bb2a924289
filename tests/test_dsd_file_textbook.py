"""The model of the DSD file layer (tests/dsd_file_textbook.py) held to what the tests' own writer recorded: for every named file the
record (rate, sample count, chunk totals, where the audio lies) and the channels' streams, chunk by chunk in every format; for every
named malformed file the stated status and the chunk that gave it; the seek's rounding; and the conversion's arithmetic (rooms, seeks,
the 0x69 fill at the stream's end alone) on small files worked by hand.  No device, no library."""
import pytest

import dsd_file_cases as FC
import dsd_file_textbook as FX
import dsd_textbook as DT


@pytest.mark.parametrize("name", list(FC.named_good()))
def test_the_model_returns_the_writers_record_and_streams(name):
    w = FC.named_good()[name]
    for W, P in FC.FORMATS:
        m = FX.read(w.data, W, P)
        assert m["status"] == FX.OK and m["error_offset"] == 0, m
        got = {k: m[k] for k in ("kind", "channels", "sample_rate", "format_version", "channel_type", "sample_count", "chunks_total", "data_offset", "data_bytes",
                                 "metadata_offset")}
        assert got == dict(kind=w.kind, channels=2, sample_rate=w.rate, format_version=w.format_version, channel_type=w.channel_type, sample_count=w.sample_count,
                           chunks_total=w.chunks_total, data_offset=w.data_offset, data_bytes=w.data_bytes, metadata_offset=w.metadata), (got, name)
        present = min(w.chunks_total, len(w.left) // 2)
        assert m["chunks_available"] == present
        if present == w.chunks_total:
            assert m["chunks_written"] == present and m["blocks"] == w.blocks(W, P)
        else:                                               # the file is shorter than it says: whole blocks of what is there
            whole = present - present % (W - P)
            assert m["chunks_written"] == whole and m["blocks"] == w.blocks(W, P, 0, whole)
        assert m["bytes_written"] == len(m["blocks"]) and len(m["blocks"]) % (W * 4) == 0


def test_the_named_malformed_files_give_the_stated_status_and_chunk():
    bad = FC.named_malformed()
    for name, (data, status, at) in bad.items():
        m = FX.read(data, 2, 0)
        assert (m["status"], m["error_offset"]) == (status, at), (name, m["status"], m["error_offset"])
        assert all(m[k] == 0 for k in FX.FIELDS if k not in ("status", "error_offset")) and m["blocks"] == b"", name
    assert {status for _, status, _ in bad.values()} == {FX.NOT_DSD, FX.TRUNCATED, FX.INVALID, FX.UNSUPPORTED}
    assert FX.read(FC.named_good()["dsf_100"].data, 2, 0)["status"] == FX.OK          # ... and with it all five statuses occur


def test_worked_bytes():
    # the packer layer's own worked examples, through a file
    left, right = bytes.fromhex("00804020"), bytes.fromhex("01814121")
    assert FX.read(FX.dsf(left, right).data, 6, 2)["blocks"] == bytes.fromhex("000080000181" "004020004121") + bytes([DT.SILENCE] * 12)
    assert FX.read(FX.dff(left, right).data, 1, 0)["blocks"] == bytes.fromhex("00800181" "40204121")
    # the file stores DSF bytes least significant bit first: the left stream's first byte 0x80 lies in the file as 0x01
    w = FX.dsf(b"\x80\x00", b"\x00\x00")
    assert w.data[w.data_offset] == 0x01 and w.data[w.data_offset + FX.PLANE] == 0x00
    # DFF lies L R L R
    w = FX.dff(b"\x11\x33", b"\x22\x44")
    assert w.data[w.data_offset:w.data_offset + 4] == bytes.fromhex("11223344") and FX.read(w.data, 6, 2)["blocks"][:6] == bytes.fromhex("001133002244")


@pytest.mark.parametrize("kind", [FX.DSF, FX.DFF])
def test_rooms_seeks_and_the_fill(kind):
    w = FC.make(kind, 45, 9)
    W, P, cpb, block = 6, 2, 4, 24
    whole = 12 * block                                       # 45 chunks: eleven blocks and one chunk of a twelfth
    m = FX.read(w.data, W, P, dst_bytes_capacity=whole)
    assert (m["chunks_written"], m["bytes_written"]) == (45, whole) and m["blocks"][45 * 6:] == bytes([DT.SILENCE] * 18) and m["blocks"] == w.blocks(W, P)
    m = FX.read(w.data, W, P, dst_bytes_capacity=whole - 1)  # the last block does not fit: whole blocks, no fill
    assert (m["chunks_written"], m["bytes_written"]) == (44, 11 * block) and m["blocks"] == w.blocks(W, P, 0, 44)
    assert FX.read(w.data, W, P, dst_bytes_capacity=block - 1)["bytes_written"] == 0
    m = FX.read(w.data, W, P, chunk_first=7, dst_bytes_capacity=3 * block)
    assert (m["chunks_written"], m["bytes_written"]) == (12, 3 * block) and m["blocks"] == w.blocks(W, P, 7, 12)
    m = FX.read(w.data, W, P, chunk_first=42)                # three chunks to the end: one block, a chunk of fill
    assert (m["chunks_written"], m["bytes_written"]) == (3, block) and m["blocks"] == w.blocks(W, P, 42, 3)
    for first in (45, 46, 1 << 40):
        m = FX.read(w.data, W, P, chunk_first=first)
        assert m["status"] == FX.OK and (m["chunks_written"], m["bytes_written"], m["blocks"]) == (0, 0, b"")
    # a prefix: what is there plays, in whole blocks
    cut = w.data[:w.data_offset + (4 * 10 + 3 if kind == FX.DFF else FX.PLANE + 2 * 10 + 1)]
    m = FX.read(cut, W, P)
    assert (m["chunks_total"], m["chunks_available"], m["chunks_written"]) == (45, 10, 8) and m["blocks"] == w.blocks(W, P, 0, 8)


def test_the_seeks_rounding():
    assert [FX.seek(FX.DSF, s) for s in (0, 1, 32767, 32768, 2047, 2048)] == [(0, 0), (0, 0), (0, 0), (2048, 32768), (0, 0), (0, 0)]
    assert [FX.seek(FX.DFF, s) for s in (0, 1, 32767, 32768, 2047, 2048)] == [(0, 0), (0, 0), (1920, 30720), (2048, 32768), (0, 0), (128, 2048)]
