"""csrc/mp4_frag_core.h -- the text both routes of the fragmented MPEG-4 layer run -- built for the CPU with AddressSanitizer and UBSan
and taken through the phases in the device's order, and through the serial text, by tests/cpp/mp4f_core_driver.cpp, a stand-alone
program.  Every stream's bytes lie in a heap block of their own size, its run records in one of exactly run_capacity; the three tables
and the destination arena are pre-filled with 0xA5 and have guards; every result, every row of the three tables, every gathered byte
and the guards must be the model's (tests/mp4f_textbook.py) on both routes, with no sanitizer report, and the driver's step counter
holds every loop to its bound.  The driver is built twice: with the host's byte reads, and with the reader the device compiles."""
import os
import subprocess

import numpy as np
import pytest

import mp4f_cases as FC
import mp4f_textbook as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[[], ["-DOHGPU_ALIGNED_READS"]], ids=["byte_reads", "the_devices_aligned_reads"])
def driver(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("mp4f_core") / "mp4f_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", *request.param,
                           os.path.join(ROOT, "tests", "cpp", "mp4f_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.mp4f_batch_check(job.descs, job.n_packets, job.n_runs, job.src.size, job.dst_bytes)      # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    sizes = (len(job.streams) * capi.MP4F_STREAM_RESULT.itemsize, job.n_runs * 32, job.n_packets * 16, job.n_packets * 16, job.dst_bytes)
    assert len(raw) == 2 * sum(sizes)
    at = 0
    for route in ("phases", "plain"):
        parts = []
        for size, dtype in zip(sizes, (capi.MP4F_STREAM_RESULT, capi.MP4F_RUN, capi.ALAC_PACKET, capi.MP4_SAMPLE, np.uint8)):
            parts.append(np.frombuffer(raw[at:at + size], dtype=dtype))
            at += size
        FC.assert_same(*parts, job, route)
    return parts[0]


def test_every_named_file(driver, tmp_path):
    good, bad, caps = FC.named_good(), FC.named_malformed(), FC.named_capacities()
    streams = [FC.stream(m, gather_first_row=k % 3) for k, m in enumerate(good.values())] + [FC.stream(data, codecs=codecs) for data, _, _, codecs in bad.values()]
    streams += [FC.stream(m, capacity=pc, run_capacity=rc) for m, rc, pc in caps.values()] + [FC.stream(m) for m, _ in FC.limit_edges().values()]
    job = FC.Job(streams)
    results = check(driver, job, tmp_path)
    assert {int(r["status"]) for r in results} == set(range(7))
    assert [(int(r["status"]), int(r["error_offset"])) for r in results[len(good):len(good) + len(bad)]] == [(status, at) for _, status, at, _ in bad.values()]
    assert sum(1 for m in job.models if m["bytes_gathered"]) >= len(good) - 3


def test_every_file_cut_round_every_box_boundary(driver, tmp_path):
    streams = []
    for name, m in FC.named_good().items():
        streams += [FC.stream(data, capacity=m.n, run_capacity=len(m.runs), dst_capacity=len(m.data)) for data in FC.cuts(m)]
    assert len(streams) > 1000
    job = FC.Job(streams)
    assert {FX.OK, FX.TRUNCATED} <= {m["status"] for m in job.models}
    assert any(m["status"] == FX.OK and m["samples_refused"] and m["bytes_gathered"] for m in job.models)       # a prefix that ends inside mdat
    big = [m for s, m in zip(streams, job.models) if len(s["data"]) > 60000]      # the files of more than a tile: refusals in a later tile, a gather that ends in one
    assert any(m["status"] == FX.OK and m["first_bad_sample"] > 1024 and m["first_bad_sample"] != FX.NO_SAMPLE and m["bytes_gathered"] for m in big)
    check(driver, job, tmp_path)


def test_two_thousand_damaged_files(driver, tmp_path):
    job = FC.Job([FC.stream(data, capacity=2100, run_capacity=8) for data in FC.damaged(2000)])
    statuses = [m["status"] for m in job.models]
    assert statuses.count(FX.OK) >= 500 and sum(1 for s in statuses if s != FX.OK) >= 500        # by the model alone: a quarter stays, a quarter is refused
    check(driver, job, tmp_path)


def test_gathers_from_every_row_into_every_room(driver, tmp_path):
    m = FC.named_good()["two_truns_without_data_offset"]
    total = sum(m.sizes)
    streams = [FC.stream(m, gather_first_row=row, dst_capacity=total) for row in (0, 1, 4, 5, 6, 70, 71, 73, 74, 75, 147, 148, 200)]
    streams += [FC.stream(m, dst_capacity=total - 1), FC.stream(m, dst_capacity=0), FC.stream(m, gather=False), FC.stream(m, capacity=72), FC.stream(m, run_capacity=2)]
    job = FC.Job(streams, align=lambda i: i % 16, dst_align=lambda i: (3 * i) % 16)
    assert [m_["bytes_gathered"] for m_ in job.models[13:16]] == [0, 0, 0] and job.models[0]["bytes_gathered"] == total and job.models[12]["bytes_gathered"] == 0
    check(driver, job, tmp_path)
