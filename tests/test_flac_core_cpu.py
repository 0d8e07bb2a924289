"""csrc/flac_frame_core.h -- the text the device kernels run -- built for the CPU with AddressSanitizer and UBSan and taken through
scan, probe, chain and restore (both routes) by tests/cpp/flac_core_driver.cpp: over every fixture, over the malformed cases that
later run on the device (tests/flac_cases.device_cases), and over a fixed-seed set of more than 2 000 mutated streams.  Every case must
end in a status -- the model's (tests/flac_textbook.py) status, counts and whole destination arena -- with no sanitizer report.
This is where malformed input is explored first: the device takes the named handful (tests/test_gpu_flac_textbook.py) and then the
whole mutation set in one batch (tests/flac_cases.device_mutations, tests/test_gpu_flac_damage.py), and nothing that has not
passed here."""
import os
import struct
import subprocess

import numpy as np
import pytest

import flac_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULT = struct.Struct("<IIQQQIIQ")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("flac_core") / "flac_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "ohpipeline_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "flac_core_driver.cpp"),
                           "-o", str(exe)])
    return exe


def run_cases(driver, cases, tmp_path):
    blob = [struct.pack("<I", len(cases))]
    for c in cases:
        blob.append(struct.pack("<8IQ", c.src_bytes, c.channels, c.bits, c.rate, c.blocksize, c.max_blocksize, c.max_samples, c.flags, c.first_sample))
        blob.append(c.data[c.offset:c.offset + c.src_bytes])
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    out, at = [], 0
    for _ in cases:
        r = RESULT.unpack_from(raw, at)
        (nb,) = struct.unpack_from("<I", raw, at + RESULT.size)
        at += RESULT.size + 4
        out.append((r[:7], np.frombuffer(raw, dtype=np.uint8, count=nb, offset=at)))
        at += nb
    assert at == len(raw)
    return out


def check(driver, cases, tmp_path):
    got = run_cases(driver, cases, tmp_path)
    statuses = set()
    for c, (res, arena) in zip(cases, got):
        want, want_arena = FC.model(c)
        assert res == FC.result_tuple(want), (c.label, res, FC.result_tuple(want))
        assert np.array_equal(arena, want_arena), c.label
        statuses.add(res[0])
    return statuses


def test_every_fixture_planes_and_packed(driver, tmp_path):
    cases = [FC.whole(fx, packed) for fx in FC.fixtures() for packed in (False, True)]
    assert check(driver, cases, tmp_path) == {0}
    for fx in FC.fixtures():
        res, _ = FC.model(FC.whole(fx))
        assert res.samples == fx.samples and res.bytes_consumed == len(fx.data) - fx.audio


def test_the_cases_that_go_to_the_device(driver, tmp_path):
    cases = FC.device_cases()
    assert check(driver, cases, tmp_path) == {0, 1, 3}
    by = {c.label: FC.model(c)[0] for c in cases}
    assert by["false_candidate"].candidates_rejected >= 1 and by["false_candidate"].status == 0
    assert by["mid_stream"].first_sample_decoded == 48 and len(by["mid_stream"].frames) == 3
    assert by["mid_stream_false_candidate"].candidates_rejected >= 1 and len(by["mid_stream_false_candidate"].frames) == 1
    assert by["cut_in_last_frame"].status == 0 and len(by["cut_in_last_frame"].frames) == 5
    assert by["flipped_bit"].status == 1 and len(by["flipped_bit"].frames) == 3
    assert by["overflow"].status == 3 and len(by["overflow"].frames) == 3


def test_the_mixed_batch_that_goes_to_the_device(driver, tmp_path):
    cases = FC.mixed_cases()
    assert len(cases) == 64 and check(driver, cases, tmp_path) == {0}
    assert all(len(FC.model(c)[0].frames) > 0 for c in cases)


def test_mutations_end_in_the_models_status(driver, tmp_path):
    cases = FC.mutations()
    assert len(cases) >= 2000
    statuses = check(driver, cases, tmp_path)
    assert {0, 1, 3} <= statuses                   # the set reaches the outcomes it is there for
    # and is not a set of streams that all die at their first byte: a good share still delivers frames
    assert sum(1 for c in cases if len(FC.model(c)[0].frames) > 0) > len(cases) // 3


def test_what_goes_to_the_device_of_them_is_all_of_them_and_outgrows_the_first_list():
    """the device's set is the set above case for case (this driver takes cases one by one, so that test has covered them), and by
    the model alone its candidates do not fit the list the device's scan sizes first: the device run scans twice"""
    cases = FC.device_mutations()
    assert list(cases) == FC.mutations() and len(cases) == 2142
    candidates = sum(FC.model(c)[0].candidates for c in cases)
    assert candidates > FC.first_list(FC.damage_layout().src.size), (candidates, FC.damage_layout().src.size)
