"""csrc/ohm_rx_core.h -- the text the Songcast receiver's three kernels run -- built for the CPU with AddressSanitizer and UBSan and
taken through parse, sequence and gather by tests/cpp/ohm_rx_core_driver.cpp, a stand-alone program: the committed sessions, the
alignment and length sweep of tests/test_gpu_ohm_rx_textbook.py (every audio length at every datagram offset mod 16 and every payload
residue mod 4, five interleaved streams), seeded window-bounded shuffles at the wrap, and a stream of every bad status.  The source
arena is allocated to the byte, the destination pre-filled with 0xA5 with guard bytes around every run; every record, every result
and the whole destination arena must be the model's (tests/ohm_rx_textbook.py), with no sanitizer report.  Then the malformed tables,
which ohgpu_ohm_rx_batch_check must refuse with the documented codes: this is where odd tables are explored; the device sees only
tables that passed that check."""
import os
import subprocess

import numpy as np
import pytest

import ohm_rx_cases as RC
import ohm_rx_textbook as RX
import ohm_textbook as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ohm_rx_core") / "ohm_rx_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "ohm_rx_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.ohm_rx_batch_check(job.d_streams, job.d_grams, len(job.src), len(job.dst0))   # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    a, b = job.want_records.nbytes, job.want_records.nbytes + job.want_results.nbytes
    assert len(raw) == b + len(job.dst0)
    recs = np.frombuffer(raw[:a], dtype=capi.OHM_RX_RECORD)
    results = np.frombuffer(raw[a:b], dtype=capi.OHM_RX_STREAM_RESULT)
    RC.assert_same(results, recs, raw[b:], job)
    return recs, results, raw[b:]


def test_the_committed_sessions(driver, tmp_path):
    job = RC.Job([RC.session_stream(s) for s in RC.load_sessions()])
    check(driver, job, tmp_path)
    assert job.want != job.dst0


def test_every_length_at_every_alignment(driver, tmp_path):
    job = RC.sweep_job()
    assert {(size - 58 - c, off % 16, c) for (off, size), c in zip(job.table, [c for c in RC.SWEEP_CODEC for _ in range(80)])} == \
        {(n, a, c) for n in RC.SWEEP_AUDIO for a in (0, 4, 8, 12) for c in RC.SWEEP_CODEC}
    assert {int(r["dst_offset"]) % 16 for r in job.want_records if r["audio_bytes"]} == set(range(16))
    assert all(r["disposition"] == RX.OUTPUT for r in job.want_records)
    _, _, arena = check(driver, job, tmp_path)
    assert arena[:RC.GUARD] == bytes([RC.FILL]) * RC.GUARD


def test_shuffled_streams_at_the_wrap(driver, tmp_path):
    rng = RC.Lcg(62)
    streams = []
    for first in (0, 5, 0xffffff00, 0xfffffffe):
        frames = RC.window_shuffle([(first + k) & 0xffffffff for k in range(300)], rng)
        grams = []
        for f in frames:
            grams.append(RC.audio_gram(f, rng.bytes(1 + rng.below(40)), depth=8, channels=1))
            if rng.below(10) == 0:
                grams.append(RC.audio_gram(f, rng.bytes(3), flags=OT.FLAG_LOSSLESS | OT.FLAG_RESENT, depth=8, channels=1))
        streams.append(RC.stream(grams))
    job = RC.Job(streams)
    assert all(res["n_output"] == 300 and res["n_pending"] == 0 and res["stop_reason"] == 0 for res in job.results)
    check(driver, job, tmp_path)


def test_every_bad_status_and_a_stream_that_ends_in_a_repair(driver, tmp_path):
    good = RC.audio_gram(3, bytes(range(40)), codec=b"abc")
    big = RC.audio_gram(4, bytes(5760), codec=b"x" * 29)
    over = big[:6] + (len(big) + 1).to_bytes(2, "big") + big[8:] + b"\0"            # 5761 audio bytes
    long_codec = good[:57] + bytes([30]) + good[58:]
    short = RC.audio_gram(5, b"", codec=b"abcdef")[:60]
    short = short[:6] + (60).to_bytes(2, "big") + short[8:]                           # the total says 60 where 58 + 6 are needed
    grams = [RC.audio_gram(2, b"\1\2"), good, b"", b"Ohm \1", over, long_codec, short, RC.other_gram(8), b"Ohm \2\3\0\10", big,
             RC.audio_gram(7, b"\5"), RC.audio_gram(30, b"\6\7"), RC.audio_gram(204, b"\10")]
    job = RC.Job([RC.stream(grams), RC.stream([]), RC.stream([RC.other_gram(0)])])
    assert [r["status"] for r in job.recs[:13]] == [RX.OK, RX.OK, RX.TRUNCATED, RX.TRUNCATED, RX.OVERSIZE, RX.BAD_HEADER, RX.TRUNCATED, RX.NOT_OHM,
                                                    RX.NOT_OHM, RX.OK, RX.OK, RX.OK, RX.OK]
    assert job.results[0]["n_pending"] == 3 and len(job.results[0]["resend"]) == 20
    check(driver, job, tmp_path)


def refused(streams, grams, src_bytes, dst_bytes):
    from ohpipeline_amd import capi
    with pytest.raises(capi.OhGpuError) as e:
        capi.ohm_rx_batch_check(streams, grams, src_bytes, dst_bytes)
    return e.value.code


def test_malformed_tables_are_refused_with_the_documented_codes():
    from ohpipeline_amd import capi
    job = RC.Job([RC.session_stream(s) for s in RC.load_sessions()[:3]])
    streams, grams = job.d_streams, job.d_grams
    sizes = (len(job.src), len(job.dst0))
    capi.ohm_rx_batch_check(streams, grams, *sizes)

    def broken(change):
        s, g = streams.copy(), grams.copy()
        change(s, g)
        return refused(s, g, *sizes)

    def put(array, i, field, value):
        array[field][i] = value

    assert broken(lambda s, g: put(g, 1, "src_offset", g["src_offset"][1] + 2)) == capi.ERR_INVALID          # a source offset that is no multiple of 4
    assert broken(lambda s, g: put(s, 1, "first_datagram", s["first_datagram"][1] - 1)) == capi.ERR_INVALID  # ranges that overlap in the table
    assert broken(lambda s, g: put(s, 1, "n_datagrams", s["n_datagrams"][1] - 1)) == capi.ERR_INVALID        # ... or leave part of it out
    assert refused(streams, grams[:-1], *sizes) == capi.ERR_INVALID
    assert broken(lambda s, g: put(g, 2, "reserved", 1)) == capi.ERR_INVALID                                 # non-zero reserved fields
    assert broken(lambda s, g: put(s, 0, "reserved", 1)) == capi.ERR_INVALID
    assert broken(lambda s, g: put(s, 2, "state_reserved", 7)) == capi.ERR_INVALID
    assert broken(lambda s, g: put(g, 2, "src_offset", (sizes[0] + 19) // 4 * 4)) == capi.ERR_BOUNDS         # a datagram outside the source arena
    assert broken(lambda s, g: put(g, 2, "bytes", sizes[0])) == capi.ERR_BOUNDS
    assert refused(streams, grams, sizes[0] - 1, sizes[1]) == capi.ERR_BOUNDS                                # (the last datagram ends where the arena ends)
    assert broken(lambda s, g: put(s, 2, "dst_offset", sizes[1] - 4)) == capi.ERR_BOUNDS                     # a run that ends outside the destination arena
    assert broken(lambda s, g: put(s, 0, "dst_capacity", sizes[1] + 1)) == capi.ERR_BOUNDS
    assert broken(lambda s, g: put(s, 1, "dst_capacity", s["dst_capacity"][1] - 1)) == capi.ERR_BOUNDS       # less room than the table's datagrams may carry
    capi.ohm_rx_batch_check(np.zeros(0, dtype=capi.OHM_RX_STREAM), np.zeros(0, dtype=capi.OHM_RX_DATAGRAM), 0, 0)   # the empty batch is legal
