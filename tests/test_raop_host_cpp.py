"""Builds and runs tests/cpp/test_raop.cpp: RAOP audio in the host adapter (RaopBatchDecoder).  Without a GPU: the
fmtp string and its refusals, datagram parsing and every InvalidRaopPacket case, the 1472-byte limit, the queue's bookkeeping, the
key-length asserts.  With one: three lanes under three keys fed the committed datagrams (tests/golden/raop_textbook.json), two
datagrams a tick, one Flush a tick; the bytes that reach ProcessorPcmBufTest must be the packed big-endian form of the PCM the packets
were encoded from, one device call per tick; and a fourth lane, fed a datagram encrypted under another key mid-stream, delivers
what precedes it and then throws."""
import os
import subprocess

import pytest

import alac_cases as AC
import alac_textbook as T
import raop_cases as RC
import raop_textbook as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_raop")
MAX_PIECE = 9216


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_raop.cpp")
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


def test_raop_decoder_bookkeeping_without_a_device():
    out = run("cpu")
    assert "cpu:" in out and " 0 failures" in out


def expectations(cfg, key, iv, payloads):
    """(bytes that must reach the processor, message sizes, packets delivered): the model chain's packets up to the first that fails,
    packed big-endian (the pipeline's byte order) and cut as Decode cuts them"""
    want, sizes, good = bytearray(), [], 0
    for payload in payloads:
        status, n, chans = AC.decode_cached(cfg, RC.decrypt_cached(key, iv, payload))
        if status != T.OK:
            break
        good += 1
        body = T.pack(cfg, chans, n, T.PACKED_BE)
        want += body
        sizes += [min(MAX_PIECE, len(body) - at) for at in range(0, len(body), MAX_PIECE)]
    return bytes(want), sizes, good


@pytest.mark.gpu
def test_lanes_from_datagrams_to_processor_through_the_gpu(tmp_path):
    lanes = []
    for s in RC.sessions()[:3]:
        want, sizes, good = expectations(s["cfg"], s["key"], s["iv"], s["payloads"])
        assert good == len(s["payloads"])
        size = s["fx"]["meta"]["bits"] // 8
        assert want == b"".join(s["fx"]["pcm"][i:i + size][::-1] for i in range(0, len(s["fx"]["pcm"]), size))       # losslessness through the cipher
        lanes.append((s["fixture"], s["fmtp"], s["key"], s["iv"], s["datagrams"], want, sizes, False))
    assert len({lane[2] for lane in lanes}) == 3
    # a lane whose third datagram was encrypted under another key (its bytes go through the sanitised CPU builds first:
    # tests/test_raop_core_cpu.py)
    s = RC.sessions()[3]
    other = RC.sessions()[0]["key"]
    head = R.parse_datagram(s["datagrams"][2])
    foreign = R.make_datagram(head["seq"], head["timestamp"], head["ssrc"], R.encrypt_packet(other, s["iv"], s["fx"]["packets"][2]))
    datagrams = s["datagrams"][:2] + [foreign] + s["datagrams"][3:]
    want, sizes, good = expectations(s["cfg"], s["key"], s["iv"], [R.parse_datagram(d)["payload"] for d in datagrams])
    assert good == 2
    lanes.append(("foreign_key", s["fmtp"], s["key"], s["iv"], datagrams, want, sizes, True))
    manifest = []
    for name, fmtp, key, iv, datagrams, want, sizes, throws in lanes:
        (tmp_path / f"{name}.fmtp").write_text(fmtp)
        (tmp_path / f"{name}.secret").write_bytes(key + iv)
        (tmp_path / f"{name}.datagrams").write_bytes(b"".join(datagrams))
        (tmp_path / f"{name}.sizes").write_text(" ".join(str(len(d)) for d in datagrams) + "\n")
        (tmp_path / f"{name}.want").write_bytes(want)
        (tmp_path / f"{name}.pieces").write_text(" ".join(str(n) for n in sizes) + "\n")
        manifest.append(f"{tmp_path / name} {int(throws)}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")
    out = run("gpu", str(tmp_path / "manifest.txt"))
    assert " 0 failures" in out and "byte-exact" in out, out
