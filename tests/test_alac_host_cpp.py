"""Builds and runs tests/cpp/test_alac.cpp: Apple Lossless in the host adapter (AlacBatchDecoder).  Without a GPU:
the configuration with and without its atoms, the packet queue's bookkeeping, the seek, the refusals (more than two channels, a
frame length above 4096), the rule a packet is cut into messages by.  With one: five lanes, two packets pushed per tick, one Flush
per tick; the bytes that reach ProcessorPcmBufTest must be the packed big-endian form of the PCM the packets were encoded from, the
message sizes Decode's (pieces of DecodedAudio::kMaxBytes, restarting with every packet), one device call per tick, and the lane
with a damaged packet mid-stream delivers the packets before it and then throws."""
import os
import subprocess

import numpy as np
import pytest

import alac_cases as AC
import alac_textbook as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_alac")
MAX_PIECE = 9216


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_alac.cpp")
    lib_dir = os.path.join(ROOT, "ohpipeline_amd", "lib")
    deps = [src, os.path.join(lib_dir, "libohhost.so"), os.path.join(lib_dir, "libohgpu.so")]
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


def test_alac_decoder_bookkeeping_without_a_device():
    out = run("cpu")
    assert "cpu:" in out and " 0 failures" in out


def expectations(cfg, packets):
    """(bytes that must reach the processor, message sizes, packets delivered): the model's packets up to the first that fails, packed
    big-endian (the pipeline's byte order: the little-endian pieces are swapped on their way in) and cut as Decode cuts them"""
    want, sizes, good = bytearray(), [], 0
    for packet in packets:
        status, n, chans = AC.decode_cached(cfg, packet)
        if status != T.OK:
            break
        good += 1
        body = T.pack(cfg, chans, n, T.PACKED_BE)
        want += body
        sizes += [min(MAX_PIECE, len(body) - at) for at in range(0, len(body), MAX_PIECE)]
    return bytes(want), sizes, good


@pytest.mark.gpu
def test_five_lanes_from_packets_to_processor_through_the_gpu(tmp_path):
    lanes = []
    for name in ("mono16_fl256", "stereo16_fl4096", "stereo24_fl1024", "stereo32_fl256"):
        fx = AC.load_fixture(name)
        want, sizes, good = expectations(fx["cfg"], fx["packets"])
        assert good == len(fx["packets"])
        # losslessness: what must arrive is the PCM that was encoded
        be = b"".join(fx["pcm"][i:i + fx["meta"]["bits"] // 8][::-1] for i in range(0, len(fx["pcm"]), fx["meta"]["bits"] // 8))
        assert want == be
        lanes.append((name, fx["cookie"], fx["packets"], fx["meta"]["rate"], want, sizes, False))
    assert any(s == MAX_PIECE for lane in lanes for s in lane[5])                      # a packet of more than one piece among them
    fx = AC.load_fixture("stereo16_fl1024")
    damaged = list(fx["packets"])
    damaged[2] = damaged[2][:len(damaged[2]) // 2]                                      # (cuts go through the sanitised CPU build first)
    want, sizes, good = expectations(fx["cfg"], damaged)
    assert good == 2
    lanes.append(("damaged", fx["cookie"], damaged, fx["meta"]["rate"], want, sizes, True))
    manifest = []
    for name, cookie, packets, rate, want, sizes, throws in lanes:
        stem = tmp_path / name
        (tmp_path / f"{name}.cookie").write_bytes(cookie)
        (tmp_path / f"{name}.packets").write_bytes(b"".join(packets))
        (tmp_path / f"{name}.sizes").write_text(" ".join(str(len(p)) for p in packets) + "\n")
        (tmp_path / f"{name}.want").write_bytes(want)
        (tmp_path / f"{name}.pieces").write_text(" ".join(str(s) for s in sizes) + "\n")
        manifest.append(f"{stem} {rate} {int(throws)}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")
    out = run("gpu", str(tmp_path / "manifest.txt"))
    assert " 0 failures" in out and "byte-exact" in out, out
