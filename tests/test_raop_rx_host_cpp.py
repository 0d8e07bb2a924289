"""Builds and runs tests/cpp/test_raop_rx.cpp: the RAOP receiver in the host adapter (RaopReceiver).  Without a GPU: the
element with a mock clock, sink and observer, csrc/raop_rx_core.h on the CPU standing in for the device between Collect and Apply -- the
8-byte wire packet, the 10 / 30 ms resend schedule, the requeue of what waits, DropAudio, SendFlush, a stop.  With one: a lane fed a
committed session's packets as damaged datagrams over four ticks (one of them with nothing new: the resend request goes out there), one
fused device call a tick; the bytes that reach ProcessorPcmBufTest must be the packed big-endian form of the PCM the packets were encoded
from."""
import os
import subprocess

import pytest

import raop_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_raop_rx")


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_raop_rx.cpp")
    lib_dir = os.path.join(ROOT, "ohpipeline_amd", "lib")
    deps = [src, os.path.join(lib_dir, "libohhost.so"), os.path.join(lib_dir, "libohgpu.so"), os.path.join(ROOT, "ohpipeline_amd", "csrc", "raop_rx_core.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE,
                           "-L", lib_dir, "-lohhost", "-lohgpu", f"-Wl,-rpath,{lib_dir}", "-lpthread"])
    return EXE


def run(*args):
    exe = build_test_binary()
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        lines = out.stdout.splitlines()
        raise AssertionError("\n".join(sorted(set(lines), key=lines.index)[:60]) + out.stderr[-2000:])
    return out.stdout


def test_the_element_with_a_mock_clock_sink_and_observer():
    out = run("cpu")
    assert "cpu:" in out and " 0 failures" in out


@pytest.mark.gpu
def test_a_lane_from_damaged_datagrams_to_the_processor_through_the_gpu(tmp_path):
    import test_gpu_raop_rx_to_pcm as TP
    s = AC.sessions()[0]
    (first, second, third), _ = TP.ticks_of(0, s, 90)
    ticks = [first, [], second, third]
    grams = [g for t in ticks for g in t]
    size = s["fx"]["meta"]["bits"] // 8
    want = b"".join(s["fx"]["pcm"][i:i + size][::-1] for i in range(0, len(s["fx"]["pcm"]), size))
    stem = tmp_path / "lane"
    (tmp_path / "lane.fmtp").write_text(s["fmtp"])
    (tmp_path / "lane.secret").write_bytes(s["key"] + s["iv"])
    (tmp_path / "lane.datagrams").write_bytes(b"".join(g for g, _ in grams))
    (tmp_path / "lane.sizes").write_text(" ".join(str(len(g)) for g, _ in grams) + "\n")
    (tmp_path / "lane.ports").write_text(" ".join(str(p) for _, p in grams) + "\n")
    (tmp_path / "lane.ticks").write_text(" ".join(str(len(t)) for t in ticks) + "\n")
    (tmp_path / "lane.want").write_bytes(want)
    out = run("gpu", str(stem))
    assert " 0 failures" in out and "byte-exact" in out, out
