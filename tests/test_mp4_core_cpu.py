"""csrc/mp4_box_core.h -- the text both routes of the MPEG-4 container layer run -- built for the CPU with AddressSanitizer and UBSan and
taken through the walk, the tile sums, the carries and the expansion, and through the serial expansion, by
tests/cpp/mp4_core_driver.cpp, a stand-alone program.  Every stream's bytes lie in a heap block of their own size, both tables are
pre-filled with 0xA5 and have guard rows; every result, every row of both tables and the guards must be the model's
(tests/mp4_textbook.py) on both routes, with no sanitizer report, and the driver's step counter holds every loop to its bound.  The
driver is built twice: with the host's byte reads, and with the reader the device compiles (aligned words joined by shifts)."""
import os
import subprocess

import numpy as np
import pytest

import mp4_cases as MC
import mp4_textbook as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024                          # kMp4Tile (csrc/ohgpu_internal.h)


@pytest.fixture(scope="module", params=[[], ["-DOHGPU_ALIGNED_READS"]], ids=["byte_reads", "the_devices_aligned_reads"])
def driver(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("mp4_core") / "mp4_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", *request.param,
                           os.path.join(ROOT, "tests", "cpp", "mp4_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.mp4_batch_check(job.descs, job.n_packets, job.src.size)      # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    a, b = len(job.streams) * capi.MP4_STREAM_RESULT.itemsize, job.n_packets * 16
    assert len(raw) == 2 * (a + 2 * b)
    for route, at in (("fused", 0), ("plain", a + 2 * b)):
        results = np.frombuffer(raw[at:at + a], dtype=capi.MP4_STREAM_RESULT)
        packets = np.frombuffer(raw[at + a:at + a + b], dtype=capi.ALAC_PACKET)
        samples = np.frombuffer(raw[at + a + b:at + a + 2 * b], dtype=capi.MP4_SAMPLE)
        MC.assert_same(results, packets, samples, job, route)
    return results


def test_every_named_file(driver, tmp_path):
    good, bad = MC.named_good(), MC.named_malformed()
    job = MC.Job([MC.stream(m) for m in good.values()] + [MC.stream(data) for data, _, _ in bad.values()])
    results = check(driver, job, tmp_path)
    assert {int(r["status"]) for r in results} == set(range(6))
    assert [int(r["status"]) for r in results[len(good):]] == [status for _, status, _ in bad.values()]
    assert bytes(job.want_packets[:MC.GUARD_ROWS].tobytes()) == bytes([MC.FILL]) * 16 * MC.GUARD_ROWS


def test_every_file_cut_round_every_box_boundary(driver, tmp_path):
    streams = []
    for m in MC.named_good().values():
        streams += [MC.stream(data, capacity=m.n) for data in MC.cuts(m)]
    assert len(streams) > 1000
    job = MC.Job(streams)
    assert {MX.OK, MX.TRUNCATED, MX.NOT_ALAC} <= {m["status"] for m in job.models}
    assert any(m["status"] == MX.OK and m["samples_refused"] for m in job.models)       # a prefix that ends inside mdat
    check(driver, job, tmp_path)


def test_five_thousand_damaged_moovs(driver, tmp_path):
    job = MC.Job([MC.stream(data) for data in MC.damaged(5000)])
    statuses = [m["status"] for m in job.models]
    assert statuses.count(MX.OK) > 500 and statuses.count(MX.INVALID) > 500 and MX.UNSUPPORTED in statuses and MX.NOT_ALAC in statuses
    assert sum(1 for m in job.models if m["samples_refused"]) > 50
    check(driver, job, tmp_path)


def test_tile_edges_chunkings_and_capacities(driver, tmp_path):
    streams = []
    for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        packets = MC.pattern_packets(n, seed=n)
        frames = [1 + (k * 5) % 7 for k in range(n)]
        for per_chunk in ([1 << 20], [1], [7], [3, 5, 2, 9, 4], [TILE - 3, 700, TILE + 5]):
            m = MC.mux(packets, MC.PATTERN_COOKIE, per_chunk=per_chunk, frames=frames, entry_per_chunk=len(per_chunk) > 1, co64=n % 2 == 1, gap=n % 4)
            streams.append(MC.stream(m))
            if n == 2 * TILE + 1:
                streams += [MC.stream(m, capacity=0), MC.stream(m, capacity=n - 1), MC.stream(m, capacity=TILE)]
    job = MC.Job(streams)
    assert all(m["status"] == MX.OK and m["samples_refused"] == 0 for m in job.models)
    check(driver, job, tmp_path)
