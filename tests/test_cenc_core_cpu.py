"""csrc/cenc_core.h over csrc/mp4_frag_core.h -- the text both routes of the protected MPEG-4 layer run -- built for the CPU with
AddressSanitizer and UBSan into tests/cpp/cenc_core_driver.cpp, a stand-alone program (its own main, run as a process, nothing preloaded),
and taken through the phases in the device's order and through the serial text.  Every stream's bytes lie in a heap block of their own
size, its room in the destination in one of exactly dst_capacity, its records and rows in blocks of exactly their capacities; the whole
destination arena and all four tables must be the model's (tests/cenc_textbook.py) on both routes, with no sanitizer report.  The driver
is built twice: with the host's byte reads, and with the reader the device compiles.

Every job of more than one tile (tests/cenc_cases.py's multi_tile_jobs) and the one-CU build of the job with more chunk slots than a
launch has waves (many_trip_job) pass here, in both builds, before tests/test_gpu_cenc_textbook.py takes them to the device.  The
driver's phases route is a serial restatement -- it has the tiles' prefixes and both searches, and no waves and no stride -- so what
it shows is that the model, the serial text and the per-tile arithmetic agree on these shapes and that no index leaves a stream's
blocks.  With `s0 = ta * kTile` replaced by `s0 = 0` in the driver's restatement (a scratch copy, never committed) both multi-tile
jobs fail here ("stream 13: block 3048 found row 1023, which does not hold it"), while the named files, the seek rows of the
142-sample file and the one-CU work list, whose streams all fit one tile, still pass."""
import os
import subprocess

import numpy as np
import pytest

import cenc_cases as CC
import cenc_textbook as CX
import mp4f_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = list(range(0, 97)) + list(range(1008, 1041)) + [2048, 2049]


@pytest.fixture(scope="module", params=[[], ["-DOHGPU_ALIGNED_READS"]], ids=["byte_reads", "the_devices_aligned_reads"])
def driver(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("cenc_core") / "cenc_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", *request.param,
                           os.path.join(ROOT, "tests", "cpp", "cenc_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.cenc_batch_check(job.descs, job.n_packets, job.n_runs, job.src.size, job.dst_bytes)      # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    sizes = (len(job.streams) * capi.CENC_STREAM_RESULT.itemsize, job.n_runs * 32, job.n_packets * 16, job.n_packets * 16, job.dst_bytes)
    assert len(raw) == 2 * sum(sizes)
    at = 0
    for route in ("phases", "plain"):
        parts = []
        for size, dtype in zip(sizes, (capi.CENC_STREAM_RESULT, capi.MP4F_RUN, capi.ALAC_PACKET, capi.MP4_SAMPLE, np.uint8)):
            parts.append(np.frombuffer(raw[at:at + size], dtype=dtype))
            at += size
        CC.assert_same(*parts, job, route)
    return parts[0]


def test_every_named_file(driver, tmp_path):
    good, bad = CC.named_good(), CC.named_malformed()
    streams = [CC.stream(m, gather_first_row=k % 3) for k, m in enumerate(good.values())]
    streams += [CC.stream(data, codecs=codecs, have_key=have_key, kid=kid) for data, _, _, codecs, have_key, kid in bad.values()]
    job = CC.Job(streams)
    results = check(driver, job, tmp_path)
    assert {int(r["mp4f"]["status"]) for r in results} >= {CX.OK, CX.INVALID, CX.NOT_CODEC, CX.UNSUPPORTED, CX.NO_KEY}
    assert [(int(r["mp4f"]["status"]), int(r["mp4f"]["error_offset"])) for r in results[len(good):]] == [(status, at) for _, status, at, _, _, _ in bad.values()]
    assert sum(1 for m in job.models if m["blocks"]) >= 12


def test_every_size_at_every_pair_of_alignments_under_twenty_keys(driver, tmp_path):
    """a file of every sample size, one stream a (source alignment, destination alignment) pair on the diagonals that meet every residue
    of both, each under one of twenty keys and either IV size"""
    files = [CC.simple([len(SIZES)], sizes=SIZES, iv_size=(8, 16)[k % 2], key=CC.key_of(k), kid=CC.kid_of(k), seed=k,
                       init=dict(info=FC.streaminfo(max_block=4096))) for k in range(20)]
    streams = [CC.stream(files[i % 20]) for i in range(32)]
    job = CC.Job(streams, align=lambda i: i % 16, dst_align=lambda i: (3 * i + i // 16) % 16)
    assert {int(d["src_offset"]) % 16 for d in job.descs} == set(range(16)) == {int(d["dst_offset"]) % 16 for d in job.descs}
    assert all(m["samples_available"] == len(SIZES) and m["blocks"] == sum((s + 15) // 16 for s in SIZES) for m in job.models)
    check(driver, job, tmp_path)


def test_both_iv_sizes_the_wrap_and_a_seek_row(driver, tmp_path):
    good = CC.named_good()
    wrap, two = good["wrap_inside_three_blocks"], good["two_truns_under_one_senc_behind"]
    streams = [CC.stream(wrap), CC.stream(wrap, gather_first_row=1), CC.stream(good["flac_iv8"]), CC.stream(good["alac_iv16"])]
    streams += [CC.stream(two, gather_first_row=row) for row in (0, 3, 5, 6, 70, 71, 100, 141, 142)]
    streams += [CC.stream(two, capacity=40, run_capacity=2), CC.stream(two, dst_capacity=sum(two.sizes) - 1), CC.stream(two, dst_capacity=0), CC.stream(two, capacity=0, run_capacity=0)]
    streams += [CC.stream(two.data[:cut], capacity=two.n, run_capacity=len(two.runs), key=two.key, kid=two.kid) for cut in (two.segment_ends[0] + 30, two.segment_ends[0] - 9)]   # prefixes
    job = CC.Job(streams)
    assert job.models[0]["gathered"][:48] == wrap.clear[0] and job.models[1]["clear_rows"][:2] == [(0, 0), (0, 7)]
    assert job.models[-1]["samples_refused"] and job.models[-1]["bytes_gathered"]
    check(driver, job, tmp_path)


def test_fixed_seed_damage_and_a_cut_at_every_byte_of_the_protection_boxes(driver, tmp_path):
    """tests/cenc_cases.damage_job, the job tests/test_gpu_cenc_textbook.py later gives the device"""
    job = CC.damage_job()
    assert len(job.streams) == 608
    statuses = [model["status"] for model in job.models]
    assert statuses.count(CX.OK) >= 100 and sum(1 for s in statuses if s not in (CX.OK, CX.TRUNCATED)) >= 50 and CX.TRUNCATED in statuses
    check(driver, job, tmp_path)


@pytest.mark.parametrize("name", ["every_count", "descriptors"])
def test_streams_of_more_than_one_tile(driver, tmp_path, name):
    """255 to 3077 samples; a tile without blocks between two that hold some; runs that end and begin inside tiles 1 and 2; two truns
    under one senc across row 1024; gather_first_row up to 2048; capacities that cut the rows at TILE + 1 and rooms too small"""
    job = CC.multi_tile_jobs()[name]
    CC.assert_reaches(name, job)
    check(driver, job, tmp_path)


def test_more_chunk_slots_than_one_cu_has_waves(driver, tmp_path):
    """the one-CU build of the job whose work list is longer than the persistent launch (the full-size one is the device's alone: here
    every stream has heap blocks of its own)"""
    job, slots, per_slot = CC.many_trip_job(1)
    CC.assert_trips(1, job, slots, per_slot)
    check(driver, job, tmp_path)
