"""csrc/iff_chunk_core.h -- the text both routes of the PCM file layer run -- built for the CPU with AddressSanitizer and UBSan and
taken through the walk and the conversion (by pieces as the device's workgroups take it, and byte by byte) by
tests/cpp/iff_core_driver.cpp, a stand-alone program.  Every file lies in a heap block that ends where it ends, the destination is
pre-filled with 0xA5 and has guard bytes round every run; every result and every destination byte, guards included, must be the
model's (tests/iff_textbook.py) on both routes, with no sanitizer report, and the driver's step counter holds the walk to its bound.
The driver is built twice: with the host's byte reads, and with the reader the device compiles (aligned words joined by shifts)."""
import os
import subprocess

import numpy as np
import pytest

import iff_cases as IC
import iff_textbook as IX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[[], ["-DOHGPU_ALIGNED_READS"]], ids=["byte_reads", "the_devices_aligned_reads"])
def driver(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("iff_core") / "iff_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", *request.param,
                           os.path.join(ROOT, "tests", "cpp", "iff_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.iff_batch_check(job.descs, job.src.size, job.dst_bytes)      # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    a = len(job.streams) * capi.IFF_STREAM_RESULT.itemsize
    assert len(raw) == 2 * (a + job.dst_bytes)
    for route, at in (("fused", 0), ("plain", a + job.dst_bytes)):
        results = np.frombuffer(raw[at:at + a], dtype=capi.IFF_STREAM_RESULT)
        IC.assert_same(results, np.frombuffer(raw[at + a:at + a + job.dst_bytes], dtype=np.uint8), job, route)
    return results


def test_every_named_file(driver, tmp_path):
    good, bad = IC.named_good(), IC.named_malformed()
    streams = [IC.stream(w, max_bit_depth=depth) for w in good.values() for depth in (24, 32)] + [IC.stream(data) for data, _, _ in bad.values()]
    job = IC.Job(streams)
    results = check(driver, job, tmp_path)
    assert {int(r["status"]) for r in results} == set(range(5))
    assert [(int(r["status"]), int(r["error_offset"])) for r in results[2 * len(good):]] == [(status, at) for _, status, at in bad.values()]
    assert all(int(r["frames_written"]) == w.frames for r, w in zip(results[0:2 * len(good):2], good.values()))


def test_every_file_cut_round_every_chunk_boundary(driver, tmp_path):
    streams = []
    for w in IC.named_good().values():
        streams += [IC.stream(data, frames=w.frames) for data in IC.cuts(w)]
    assert len(streams) > 500
    job = IC.Job(streams)
    assert {IX.OK, IX.TRUNCATED} <= {m["status"] for m in job.models}
    assert any(m["status"] == IX.OK and 0 < m["frames_available"] < m["frames_total"] for m in job.models)      # a prefix that ends inside the audio
    check(driver, job, tmp_path)


def test_five_thousand_damaged_headers(driver, tmp_path):
    job = IC.Job([IC.stream(data, frames=48) for data in IC.damaged(5000)])
    statuses = [m["status"] for m in job.models]
    assert set(statuses) == set(range(5)) and statuses.count(IX.OK) > 500 and statuses.count(IX.INVALID) > 100
    check(driver, job, tmp_path)


def test_the_shape_sweep(driver, tmp_path):
    check(driver, IC.Job(IC.shape_sweep()), tmp_path)
    for job in IC.alignment_sweep():
        check(driver, job, tmp_path)
