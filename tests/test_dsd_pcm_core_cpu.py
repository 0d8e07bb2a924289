"""csrc/dsd_pcm_core.h -- the text the plain DSD -> PCM kernel runs per thread -- built for the CPU with AddressSanitizer and UBSan and
taken by tests/cpp/dsd_pcm_core_driver.cpp over every batch that later runs on the device (tests/dsd_pcm_cases.every_case): each
whole destination arena must equal the model's (tests/dsd_pcm_textbook.py), with no sanitizer report.  The arenas are allocated to
the byte: a bit fetched from outside a message's window, or a value stored outside its frames, is a report."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dsd_pcm_cases as DC
import pcm_textbook as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dsd_pcm_core") / "dsd_pcm_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "ohpipeline_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "dsd_pcm_core_driver.cpp"),
                           "-o", str(exe)])
    return exe


def run_cases(driver, cases, tmp_path):
    blob = [np.array(PT.ramp_table(), dtype="<u2").tobytes(), struct.pack("<I", len(cases))]
    for c in cases:
        D, T = c.key
        blob.append(struct.pack("<4I2Q", D, T, c.descs.size, DC.FILL, c.src.size, c.dst_bytes))
        blob.append(DC.coef(c.key).astype("<i4").tobytes())
        blob.append(c.descs.tobytes())
        blob.append(c.src.tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw, at, out = (tmp_path / "out.bin").read_bytes(), 0, []
    for c in cases:
        out.append(np.frombuffer(raw, dtype=np.uint8, count=c.dst_bytes, offset=at))
        at += c.dst_bytes
    assert at == len(raw)
    return out


def test_every_case_that_goes_to_the_device(driver, tmp_path):
    cases = DC.every_case()
    assert len(cases) == 9
    for c, got in zip(cases, run_cases(driver, cases, tmp_path)):
        bad = np.nonzero(got != c.want())[0]
        assert bad.size == 0, f"{c.label}: {bad.size} differing bytes, first at {bad[:6].tolist()}"


def test_far_positions_and_their_near_twins(driver, tmp_path):
    """tests/dsd_pcm_cases.positions: out_frame0 up to 2^40, the stream's bit, byte and chunk index past 2^32 -- and the same frames
    entered near the stream's start.  The core gives the model's bytes for both, and the two are the same bytes."""
    cases = DC.every_far_case()
    assert len(cases) == 8 and max(int(c.descs["out_frame0"].max()) for c in cases) == 1 << 40
    for c, got in zip(cases, run_cases(driver, cases, tmp_path)):
        bad = np.nonzero(got != c.want())[0]
        assert bad.size == 0, f"{c.label}: {bad.size} differing bytes, first at {bad[:6].tolist()}"
    for key in DC.DESIGNS:
        assert np.array_equal(DC.positions(key, True).want(), DC.positions(key, False).want()), key


def test_the_cases_reach_what_they_are_there_for():
    """All ones clamp to 2^23 - 1, all zeros give -2^23, a stream start reads the idle pattern (it differs from the same bits read
    mid-stream), and the fill between the messages is there to be compared."""
    import dsd_pcm_textbook as DP
    for key in DC.DESIGNS:
        D, T = key
        co = DC.coef(key)
        ones = np.ones((2, 16 * 300), dtype=np.uint8)
        assert (DP.frames(co, D, ones, 0, T + 2, 3) == (1 << 23) - 1).all()
        assert (DP.frames(co, D, 1 - ones, 0, T + 2, 3) == -(1 << 23)).all()
        assert not (DP.frames(co, D, ones, 0, 0, 1) == (1 << 23) - 1).all()          # (idle history pulls the first frame down)
        want = DC.shapes(key).want()
        assert (want == DC.FILL).sum() >= 24 and (want != DC.FILL).sum() > 6 * 3000
