"""Builds and runs tests/cpp/test_dsd_pcm.cpp: the DSD -> PCM element of the host adapter (host/DsdPcmConverter.{h,cpp}; DESIGN.md 4c,
5.11).  Without a GPU: the design, a lane's bookkeeping, the history it keeps, the announced stream and the 9216-byte pieces.  With
one: five lanes over several ticks into ProcessorPcmBufTest, one joining mid-run, byte for byte a single-shot conversion of each
whole stream."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_dsd_pcm")


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_dsd_pcm.cpp")
    lib_dir = os.path.join(ROOT, "ohpipeline_amd", "lib")
    deps = [src, os.path.join(lib_dir, "libohhost.so"), os.path.join(lib_dir, "libohgpu.so")]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE,
                           "-L", lib_dir, "-lohhost", "-lohgpu", f"-Wl,-rpath,{lib_dir}", "-lpthread"])
    return EXE


def run(mode):
    exe = build_test_binary()
    out = subprocess.run([exe, mode], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        lines = out.stdout.splitlines()
        raise AssertionError("\n".join(sorted(set(lines), key=lines.index)[:60]) + out.stderr[-2000:])
    return out.stdout


def test_dsd_pcm_lanes_on_the_control_plane():
    out = run("cpu")
    assert "cpu:" in out and " 0 failures" in out


@pytest.mark.gpu
def test_dsd_pcm_from_chunks_to_processor_through_the_gpu():
    out = run("gpu")
    assert " 0 failures" in out and "byte-exact" in out, out
