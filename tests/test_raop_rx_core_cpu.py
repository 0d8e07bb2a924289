"""csrc/raop_rx_core.h -- the text the RAOP receiver's parse, plain sequencer and table kernels run -- built for the CPU with
AddressSanitizer and UBSan and taken through the three phases by tests/cpp/raop_rx_core_driver.cpp, a stand-alone program, once with
field_bytes.h's byte reader and once with the device's aligned dword reader: the committed sessions and the reference's suite, the
seeded lossy sessions, the shapes of tests/test_gpu_raop_rx_textbook.py, and every datagram length 0..20 and 1470..1474 of every kind at
the four source offsets mod 16.  The source arena is allocated to the byte; every record, every result and every packet row must be the
model's (tests/raop_rx_textbook.py), with no sanitizer report.  Then the malformed tables, which ohgpu_raop_rx_batch_check must refuse
with the documented codes: the device sees only tables that passed that check."""
import os
import subprocess

import numpy as np
import pytest

import raop_rx_cases as RC
import raop_rx_textbook as RX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["bytes", "aligned"])
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("raop_rx_core") / f"raop_rx_core_driver_{request.param}"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra"] +
                          (["-DOHGPU_ALIGNED_READS"] if request.param == "aligned" else []) +
                          [os.path.join(ROOT, "tests", "cpp", "raop_rx_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.raop_rx_batch_check(job.d_streams, job.d_grams, len(job.src))       # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    a, b = job.want_records.nbytes, job.want_records.nbytes + job.want_results.nbytes
    assert len(raw) == b + job.want_rows.nbytes
    RC.assert_same(np.frombuffer(raw[a:b], dtype=capi.RAOP_RX_STREAM_RESULT), np.frombuffer(raw[:a], dtype=capi.RAOP_RX_RECORD),
                   np.frombuffer(raw[b:], dtype=capi.ALAC_PACKET), job)


def suite_streams():
    """every batch of every case of the reference's suite, as the caller would hand it over: the pending datagrams in front, state_out as state_in"""
    out = []
    for case in RC.load_golden()["resend_suite"]:
        state = RX.new_state()
        for todo, _, res in RC.play(RC.suite_batches(case), case["max_frames"]):
            out.append(RC.stream(todo, state, case["max_frames"]))
            state = res["state_out"]       # (a drop changes it further; the stream that follows a drop is then not the caller's, which is no matter here)
    return out


def test_the_committed_sessions_and_the_reference_suite(driver, tmp_path):
    gold = RC.load_golden()
    sessions = [RC.stream(RC.golden_grams(s), s["state_in"], s["max_frames"]) for s in gold["sessions"]]
    grams = RC.stream([(bytes.fromhex(g["hex"]), g["port"]) for g in gold["datagrams"]])
    job = RC.Job(sessions + [grams] + suite_streams())
    assert {RX.STOP_BUFFER_FULL, RX.STOP_RESTARTED} <= {r["stop_reason"] for r in job.results} and any(r["n_pending"] for r in job.results)
    check(driver, job, tmp_path)


def test_the_seeded_sessions(driver, tmp_path):
    check(driver, RC.Job(RC.lossy_streams()), tmp_path)


def test_the_shapes_of_the_wave_kernel(driver, tmp_path):
    check(driver, RC.Job(RC.shape_streams() + RC.mixed_streams()), tmp_path)


def test_every_length_at_every_alignment(driver, tmp_path):
    job = RC.Job(RC.sweep_streams())
    assert {(size, off % 16) for off, size, _ in job.table} == {(n, a) for n in RC.SWEEP_LENGTHS for a in (0, 4, 8, 12)}
    statuses = {(size, port, int(r["status"])) for (_, size, port), r in zip(job.table, job.want_records)}
    assert {(11, 0, RX.TRUNCATED), (12, 0, RX.OK), (19, 1, RX.TRUNCATED), (20, 1, RX.OK), (1472, 0, RX.OK), (1473, 0, RX.OVERSIZE), (1473, 1, RX.OVERSIZE),
            (4, 1, RX.OTHER_TYPE), (15, 1, RX.TRUNCATED), (16, 1, RX.OK)} <= statuses
    check(driver, job, tmp_path)


def refused(streams, grams, src_bytes):
    from ohpipeline_amd import capi
    with pytest.raises(capi.OhGpuError) as e:
        capi.raop_rx_batch_check(streams, grams, src_bytes)
    return e.value.code


def test_malformed_tables_are_refused_with_the_documented_codes():
    from ohpipeline_amd import capi
    job = RC.Job(RC.lossy_streams()[:3])
    streams, grams, size = job.d_streams, job.d_grams, len(job.src)
    capi.raop_rx_batch_check(streams, grams, size)

    def broken(change):
        s, g = streams.copy(), grams.copy()
        change(s, g)
        return refused(s, g, size)

    def put(array, i, field, value):
        array[field][i] = value

    assert broken(lambda s, g: put(g, 1, "src_offset", g["src_offset"][1] + 2)) == capi.ERR_INVALID          # a source offset that is no multiple of 4
    assert broken(lambda s, g: put(g, 1, "port", 2)) == capi.ERR_INVALID                                     # a port that is neither
    assert broken(lambda s, g: put(s, 1, "first_datagram", s["first_datagram"][1] - 1)) == capi.ERR_INVALID  # ranges that overlap in the table
    assert broken(lambda s, g: put(s, 1, "n_datagrams", s["n_datagrams"][1] - 1)) == capi.ERR_INVALID        # ... or leave part of it out
    assert refused(streams, grams[:-1], size) == capi.ERR_INVALID
    assert broken(lambda s, g: put(s, 0, "max_frames", 0)) == capi.ERR_INVALID                               # max_frames outside 1..63
    assert broken(lambda s, g: put(s, 0, "max_frames", 64)) == capi.ERR_INVALID
    assert broken(lambda s, g: put(s, 2, "running", 2)) == capi.ERR_INVALID                                  # a flag that is no flag
    assert broken(lambda s, g: put(s, 2, "resume_pending", 2)) == capi.ERR_INVALID
    assert broken(lambda s, g: put(g, 2, "reserved", 1)) == capi.ERR_INVALID                                 # non-zero reserved fields
    assert broken(lambda s, g: put(s, 0, "reserved", 1)) == capi.ERR_INVALID
    assert broken(lambda s, g: put(s, 2, "state_reserved", 7)) == capi.ERR_INVALID
    assert broken(lambda s, g: put(g, 2, "src_offset", (size + 19) // 4 * 4)) == capi.ERR_BOUNDS             # a datagram outside the source arena
    assert broken(lambda s, g: put(g, 2, "bytes", size)) == capi.ERR_BOUNDS
    assert refused(streams, grams, size - 1) == capi.ERR_BOUNDS                                              # (the last datagram ends where the arena ends)
    capi.raop_rx_batch_check(np.zeros(0, dtype=capi.RAOP_RX_STREAM), np.zeros(0, dtype=capi.RAOP_RX_DATAGRAM), 0)   # the empty batch is legal
