"""csrc/dsd_file_core.h -- the text both routes of the DSD file layer run -- built for the CPU with AddressSanitizer and UBSan and
taken through the walk and the conversion (by pieces as the device's workgroups take it, lane by lane, and byte by byte) by
tests/cpp/dsd_file_core_driver.cpp, a stand-alone program.  Every file lies in a heap block that ends where it ends, the destination
is pre-filled with 0xA5 and has guard bytes round every run; every result and every destination byte, guards included, must be the
model's (tests/dsd_file_textbook.py) on both routes, with no sanitizer report, and the driver's step counter holds the walk to its
bound.  The driver is built twice: with the host's byte reads, and with the reader the device compiles (aligned words joined by
shifts)."""
import os
import subprocess

import numpy as np
import pytest

import dsd_file_cases as FC
import dsd_file_textbook as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[[], ["-DOHGPU_ALIGNED_READS"]], ids=["byte_reads", "the_devices_aligned_reads"])
def driver(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("dsd_file_core") / "dsd_file_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", *request.param,
                           os.path.join(ROOT, "tests", "cpp", "dsd_file_core_driver.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def jobs():
    """The jobs, made once for both drivers."""
    good, bad = FC.named_good(), FC.named_malformed()
    named = FC.Job([FC.stream(w, W, P) for w in good.values() for W, P in FC.FORMATS] + [FC.stream(data) for data, _, _ in bad.values()])
    cut = []
    for k, w in enumerate(good.values()):
        cut += [FC.stream(data, *FC.FORMATS[(k + n) % 4], room=FC.stream(w, *FC.FORMATS[(k + n) % 4])["room"]) for n, data in enumerate(FC.cuts(w))]
    return dict(named=named, cut=FC.Job(cut), shapes=FC.Job(FC.shape_sweep()), phases=FC.phase_sweep(), good=good, bad=bad)


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.dsd_file_batch_check(job.descs, job.src.size, job.dst_bytes)      # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    a = len(job.streams) * capi.DSD_FILE_STREAM_RESULT.itemsize
    assert len(raw) == 2 * (a + job.dst_bytes)
    for route, at in (("fused", 0), ("plain", a + job.dst_bytes)):
        results = np.frombuffer(raw[at:at + a], dtype=capi.DSD_FILE_STREAM_RESULT)
        FC.assert_same(results, np.frombuffer(raw[at + a:at + a + job.dst_bytes], dtype=np.uint8), job, route)
    return results


def test_every_named_file(driver, jobs, tmp_path):
    good, bad = jobs["good"], jobs["bad"]
    results = check(driver, jobs["named"], tmp_path)
    assert {int(r["status"]) for r in results} == set(range(5))
    assert [(int(r["status"]), int(r["error_offset"])) for r in results[4 * len(good):]] == [(status, at) for _, status, at in bad.values()]
    assert all(int(r["chunks_written"]) == min(w.chunks_total, int(r["chunks_available"])) for r, w in zip(results[0:4 * len(good):4], good.values()))


def test_every_file_cut_at_every_byte_round_every_header_boundary(driver, jobs, tmp_path):
    job = jobs["cut"]
    assert len(job.streams) > 500
    assert {FX.OK, FX.TRUNCATED, FX.NOT_DSD} <= {m["status"] for m in job.models}
    assert any(m["status"] == FX.OK and 0 < m["chunks_available"] < m["chunks_total"] for m in job.models)      # a prefix that ends inside the audio
    check(driver, job, tmp_path)


def test_the_shape_sweep(driver, jobs, tmp_path):
    check(driver, jobs["shapes"], tmp_path)


def test_the_audio_at_every_address(driver, jobs, tmp_path):
    job = jobs["phases"]
    assert all(FC.has_wide_body(job, i) for i in range(len(job.streams)))
    check(driver, job, tmp_path)
