"""csrc/cbcs_core.h over csrc/cenc_core.h and csrc/mp4_frag_core.h -- the text both routes of the second protected MPEG-4 family run --
built for the CPU with AddressSanitizer and UBSan into tests/cpp/cbcs_core_driver.cpp, a stand-alone program (its own main, run as a
process, nothing preloaded), and taken through the phases in the device's order and through the serial text.  Every stream's bytes lie
in a heap block of their own size, its room in the destination in one of exactly dst_capacity, its records, rows and subsample rows in
blocks of exactly their capacities; the whole destination arena and all four tables must be the model's (tests/cbcs_textbook.py) on
both routes, with no sanitizer report.  The driver is built twice: with the host's byte reads, and with the reader the device compiles.

The driver's phases route restates the work-list arithmetic: the tiles' prefixes over work units, the three searches, and -- given a CU
count -- the persistent launch's chunk slots, its stride and its jumps, with every unit met exactly once.  Every job of
tests/test_gpu_cbcs_textbook.py passes here first."""
import os
import subprocess

import numpy as np
import pytest

import cbcs_cases as BC
import cbcs_jobs as BJ
import cbcs_textbook as BX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[[], ["-DOHGPU_ALIGNED_READS"]], ids=["byte_reads", "the_devices_aligned_reads"])
def driver(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("cbcs_core") / "cbcs_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", *request.param,
                           os.path.join(ROOT, "tests", "cpp", "cbcs_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path, cus=None):
    from ohpipeline_amd import capi
    capi.cbcs_batch_check(job.descs, job.n_packets, job.n_runs, job.n_subsamples, job.src.size, job.dst_bytes)     # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")] + ([str(cus)] if cus else []), capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    sizes = (len(job.streams) * capi.CBCS_STREAM_RESULT.itemsize, job.n_runs * 32, job.n_packets * 16, job.n_packets * 16, job.dst_bytes)
    assert len(raw) == 2 * sum(sizes)
    at = 0
    for route in ("phases", "plain"):
        parts = []
        for size, dtype in zip(sizes, (capi.CBCS_STREAM_RESULT, capi.MP4F_RUN, capi.ALAC_PACKET, capi.MP4_SAMPLE, np.uint8)):
            parts.append(np.frombuffer(raw[at:at + size], dtype=dtype))
            at += size
        BC.assert_same(*parts, job, route)
    return parts[0]


def test_every_named_file(driver, tmp_path):
    job = BJ.named_job()
    results = check(driver, job, tmp_path)
    BJ.assert_named(job, results)


def test_every_part_size_at_four_by_four_alignments(driver, tmp_path):
    job = BJ.alignment_job()
    BJ.assert_alignments(job)
    check(driver, job, tmp_path)


def test_capacities_prefixes_and_seek_rows(driver, tmp_path):
    job = BJ.capacity_job()
    BJ.assert_capacities(job)
    check(driver, job, tmp_path)


def test_streams_of_more_than_one_tile(driver, tmp_path):
    job = BJ.tile_job()
    BJ.assert_tiles(job)
    check(driver, job, tmp_path)


def test_the_interleaved_batch(driver, tmp_path):
    job = BJ.mixed_job()
    BJ.assert_mixed(job)
    check(driver, job, tmp_path)


def test_fixed_seed_damage(driver, tmp_path):
    job = BJ.damage_job()
    BJ.assert_damage(job)
    check(driver, job, tmp_path)


def test_more_chunk_slots_than_one_cu_has_waves(driver, tmp_path):
    """the one-CU build of the many-trip job, in the persistent launch's own order: slots, stride and jumps"""
    job, slots = BJ.many_trip_job(1)
    BJ.assert_trips(1, job, slots)
    check(driver, job, tmp_path, cus=1)
