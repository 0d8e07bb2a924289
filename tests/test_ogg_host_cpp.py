"""Builds and runs tests/cpp/test_ogg_flac_decoder.cpp: Ogg FLAC in the host adapter (FlacRecognise, OggFlacBatchDecoder; DESIGN.md
5.15).  Without a GPU: CodecFlac::Recognise's rule on "fLaC", on "OggS" with and without "fLaC" at 37 and on 41 bytes, the byte queue's
bookkeeping, the head split over ragged pushes, the refusals.  With one: five lanes -- fixtures of tests/golden/flac wrapped in pages by
the tests' muxer -- pushed in 1 000-byte pieces over several ticks, one Flush per tick; the bytes that reach ProcessorPcmBufTest must
be the packed big-endian form of the PCM the plain-Python FLAC model decodes from the native stream, the message sizes
CallbackWrite's, one device call per tick, and the lane with a flipped bit in a page delivers the frames of the pages in front of it
and throws after every lane was served."""
import os
import subprocess

import pytest

import flac_cases as FC
import flac_textbook as T
import ogg_cases as GC
import ogg_textbook as OX
import test_flac_host_cpp as FH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_ogg_flac_decoder")
TINY = "tiny_s16_stereo_44k1_b16"


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_ogg_flac_decoder.cpp")
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


def tiny_files(tmp_path):
    fx = FC.fixture(TINY)
    data, _, _ = GC.ogg_flac(fx, max_segments=2)
    (tmp_path / "tiny.ogg").write_bytes(data)
    return str(tmp_path / "tiny.ogg"), os.path.join(FC.NEW_DIR, TINY + ".flac")


def test_recognise_and_the_decoders_bookkeeping_without_a_device(tmp_path):
    out = run("cpu", *tiny_files(tmp_path))
    assert "cpu:" in out and " 0 failures" in out


@pytest.mark.gpu
def test_five_lanes_from_file_bytes_to_processor_through_the_gpu(tmp_path):
    lanes = []
    for name, segs in (("s16_stereo_44k1_b1152_l5", 5), ("s24_stereo_44k1_b576_l0", 255), ("s8_mono_8k_b256_l2", 1), ("escape_wasted_s24_stereo_44k1_b576", 17)):
        # (streams at rates the pipeline carries: Jiffies::IsValidSampleRate refuses the fixtures' 44 056 and 11 000 Hz)
        fx = FC.fixture(name)
        lanes.append((name, GC.ogg_flac(fx, max_segments=segs)[0], fx.data, False))
    fx = FC.fixture("s16_stereo_44k1_b1152_l5")
    data, audio_page, audio_seq = GC.ogg_flac(fx, max_segments=4)
    broken = bytearray(data)
    broken[audio_page + (len(data) - audio_page) * 2 // 3] ^= 0x08                    # one bit, two thirds into the audio pages
    seen = OX.demux(bytes(broken[audio_page:]), serial=0x464C, expect_seq=audio_seq, flags=OX.FLAC_MAPPING)
    assert seen["status"] == OX.LOST_SYNC and 0 < len(seen["run"]) < len(fx.data) - fx.audio
    lanes.append(("flipped", bytes(broken), fx.data[:fx.audio] + seen["run"], True))  # what precedes the break, as a native stream
    manifest = []
    for name, ogg, native, throws in lanes:
        res, want, sizes = FH.expectations(native, T.streaminfo(native))
        assert res.status == T.OK and len(res.frames) > 0
        if not throws:
            assert res.samples == T.streaminfo(native)[0]["total_samples"]
        (tmp_path / f"{name}.ogg").write_bytes(ogg)
        want.tofile(tmp_path / f"{name}.want")
        (tmp_path / f"{name}.pieces").write_text(" ".join(str(s) for s in sizes) + "\n")
        manifest.append(f"{tmp_path / (name + '.ogg')} {tmp_path / (name + '.want')} {tmp_path / (name + '.pieces')} {int(throws)}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")
    out = run("gpu", *tiny_files(tmp_path), str(tmp_path / "manifest.txt"))
    assert " 0 failures" in out and "byte-exact" in out, out
