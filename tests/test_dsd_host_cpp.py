"""Builds and runs tests/cpp/test_dsd.cpp: DSD in the host adapter (MsgAudioDsd, DSD silence and playables, IDsdProcessor,
CodecController::OutputAudioDsd, DsdPacker).  Without a GPU: the reference's DSD message suite restated on the control
plane and the packer's bookkeeping.  With one: the parts of that suite that read audio, and five lanes over several ticks from
packer to ProcessorDsdBufTest, byte for byte."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_dsd")


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_dsd.cpp")
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


def test_dsd_messages_on_the_control_plane():
    out = run("cpu")
    assert "cpu:" in out and " 0 failures" in out


@pytest.mark.gpu
def test_dsd_from_packer_to_processor_through_the_gpu():
    out = run("gpu")
    assert " 0 failures" in out and "byte-exact" in out, out
