"""Builds and runs tests/cpp/test_mpeg4_alac_decoder.cpp: Apple Lossless in an MPEG-4 file in the host adapter (Mpeg4Recognise,
Mpeg4AlacBatchDecoder).  Without a GPU: the `ftyp` rule, the top-level peek over ragged pushes of a moov-first and a
moov-last file (the head is whole exactly when the byte the muxer's record names has arrived), the refusals.  With one: five lanes --
fixtures of tests/golden/alac wrapped by the tests' muxer -- pushed in 1 000-byte pieces over several ticks, one Flush per tick: a
moov-first file, a moov-last file, a 24-bit file, a lane that seeks to a frame inside its third packet as soon as its head has been
read and must resume at that packet's first frame, and a lane with an mp4a entry that throws after every lane was served.  The bytes
that reach ProcessorPcmBufTest must be the packed big-endian form of the PCM the packets were encoded from, the message sizes
Decode's (AlacAppleBase.cpp:94-111), with one call for the heads of a tick and one decode call per tick."""
import os
import subprocess

import pytest

import alac_cases as AC
import mp4_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_mpeg4_alac_decoder")
MAX_PIECE = 9216                     # DecodedAudio::kMaxBytes


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_mpeg4_alac_decoder.cpp")
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


def peek_files(tmp_path):
    """a moov-first and a moov-last file, and the byte count at which each one's head is whole by the muxer's own record: the end of
    the mdat header behind moov, and the end of moov"""
    fx = AC.load_fixture("stereo16_fl1024")
    first, last = MC.fixture_file(fx, per_chunk=[2]), MC.fixture_file(fx, per_chunk=[3], moov_last=True)
    (tmp_path / "first.m4a").write_bytes(first.data)
    (tmp_path / "last.m4a").write_bytes(last.data)
    assert first.find("mdat")[0] == first.find("moov")[2] and last.find("moov")[2] == len(last.data)
    return [str(tmp_path / "first.m4a"), str(first.find("mdat")[1]), str(tmp_path / "last.m4a"), str(len(last.data))]


def test_recognition_the_peek_and_the_refusals_without_a_device(tmp_path):
    out = run("cpu", *peek_files(tmp_path))
    assert "cpu:" in out and " 0 failures" in out


def expectations(fx, first_packet=0):
    """the PCM the fixture was encoded from, from a packet on, packed big-endian, and the sizes Decode cuts each packet's bytes into"""
    width, unit = fx["meta"]["bits"] // 8, fx["cfg"]["channels"] * (fx["meta"]["bits"] // 8)
    fl, want, sizes = fx["cfg"]["frame_length"], bytearray(), []
    for k in range(first_packet, len(fx["packets"])):
        body = fx["pcm"][k * fl * unit:(k + 1) * fl * unit]
        want += b"".join(body[i:i + width][::-1] for i in range(0, len(body), width))
        sizes += [min(MAX_PIECE, len(body) - at) for at in range(0, len(body), MAX_PIECE)]
    return bytes(want), sizes


@pytest.mark.gpu
def test_five_lanes_from_file_bytes_to_processor_through_the_gpu(tmp_path):
    a, b, c = AC.load_fixture("stereo16_fl4096"), AC.load_fixture("stereo16_fl1024"), AC.load_fixture("stereo24_fl1024")
    seeker = MC.fixture_file(b, per_chunk=[3])
    assert seeker.find("mdat")[1] < 1000 < seeker.offsets[0] + seeker.sizes[0]        # its head is whole in the first tick, its first packet is not
    frame = 2 * 1024 + 17
    assert seeker.first_frames[2] <= frame < seeker.first_frames[3]
    lanes = [("first", MC.fixture_file(a, per_chunk=[1]).data, expectations(a), 0, -1, 0),
             ("last", MC.fixture_file(b, per_chunk=[2], moov_last=True, co64=True).data, expectations(b), 0, -1, 0),
             ("deep", MC.fixture_file(c, per_chunk=[3]).data, expectations(c), 0, -1, 0),
             ("seeker", seeker.data, expectations(b, first_packet=2), 0, frame, seeker.first_frames[2]),
             ("mp4a", MC.fixture_file(b, entry_kind=b"mp4a").data, (b"", []), 2, -1, 0)]
    assert any(s == MAX_PIECE for lane in lanes for s in lane[2][1])                  # a packet of more than one piece among them
    manifest = []
    for name, data, (want, sizes), throws, seek, first in lanes:
        stem = tmp_path / f"lane_{name}"
        (tmp_path / f"lane_{name}.m4a").write_bytes(data)
        (tmp_path / f"lane_{name}.want").write_bytes(want)
        (tmp_path / f"lane_{name}.pieces").write_text(" ".join(str(s) for s in sizes) + "\n")
        manifest.append(f"{stem}.m4a {stem}.want {stem}.pieces {throws} {seek} {first}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")
    out = run("gpu", *peek_files(tmp_path), str(tmp_path / "manifest.txt"))
    assert " 0 failures" in out and "byte-exact" in out, out
