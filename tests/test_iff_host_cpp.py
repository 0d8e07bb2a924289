"""Builds and runs tests/cpp/test_pcm_file_decoder.cpp: PCM files in the host adapter (WavRecognise, AiffRecognise, AifcRecognise,
PcmFileBatchDecoder).  Without a GPU: the three recognition rules and a decoder before its first tick.  With one: five
lanes -- 16-bit WAV, 32-bit WAV under a 24-bit limit, AIFF, AIFC `sowt` with a seek as soon as its stream has been announced, and a
file that is none of them, which throws after every lane was served -- pushed in 20 000-byte pieces over several ticks, one Flush per
tick.  The MsgDecodedStream fields, the messages' sizes and track offsets, and the bytes that reach ProcessorPcmBufTest must be what
the tests' own writer recorded."""
import os
import subprocess

import pytest

import iff_cases as IC
import iff_textbook as IX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_pcm_file_decoder")
MAX_PIECE = 9216                     # DecodedAudio::kMaxBytes
PUSH = 20000                         # kPush
JIFFIES_PER_SECOND = 56448000


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_pcm_file_decoder.cpp")
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


def test_recognition_and_a_decoder_before_its_first_tick_without_a_device():
    out = run("cpu")
    assert "cpu:" in out and " 0 failures" in out


def expectations(w, max_bit_depth, seek):
    """The bytes the lane must deliver and its messages' sizes: what has arrived by each tick, from the frame the lane stands at (a
    seek moves it once, behind the tick that announced the stream), cut into pieces of whole frames within MAX_PIECE."""
    out_bytes = min(w.sample_bytes, max_bit_depth // 8)
    frame_in, frame_out = w.channels * w.sample_bytes, w.channels * out_bytes
    piece = MAX_PIECE // frame_out * frame_out
    want, sizes, at, sought = bytearray(), [], 0, False
    for tick in range(-(-len(w.data) // PUSH)):
        arrived = min(len(w.data), PUSH * (tick + 1))
        frames = max(0, min(arrived - w.data_offset, w.frames * frame_in) // frame_in - at)
        body = w.pcm(out_bytes, first=at, frames=frames)
        want += body
        sizes += [min(piece, len(body) - k) for k in range(0, len(body), piece)]
        at += frames
        if seek >= 0 and not sought:
            at, sought = seek, True
    return bytes(want), sizes


@pytest.mark.gpu
def test_five_lanes_from_file_bytes_to_processor_through_the_gpu(tmp_path):
    s = IC.samples
    lanes = [("wav16", IC.wav(s(11000, 2, 2, 81), 2, between=[IC.junk(b"LIST", 26)]), 24, -1, "WAV"),
             ("wav32_under_24", IC.wav(s(5500, 2, 4, 82), 2, rate=48000), 24, -1, "WAV"),
             ("aiff", IC.aiff(s(9000, 2, 3, 83), 2, rate=48000, ssnd_offset=2), 24, -1, "AIFF"),
             ("aifc_sowt", IC.aiff(s(12000, 2, 2, 84), 2, compression=b"sowt"), 32, 7001, "AIFF"),
             ("none_of_them", None, 24, -1, "-")]
    manifest = []
    for name, w, depth, seek, codec in lanes:
        stem = tmp_path / f"lane_{name}"
        if w is None:
            data, want, sizes, fields = b"\0\0\0\x20ftypM4A " + bytes(5000), b"", [], "0 0 0 0 - 0"
        else:
            assert len(w.data) > 2 * PUSH and w.data_offset < PUSH                     # several ticks, the stream announced in the first
            data = w.data
            want, sizes = expectations(w, depth, seek)
            model = IX.read(w.data, max_bit_depth=depth)
            IC.check_against_record(model, w)
            fields = f"{w.bit_rate} {min(w.depth, depth)} {w.rate} {w.channels} {codec} {w.frames * (JIFFIES_PER_SECOND // w.rate)}"
            assert MAX_PIECE // (w.channels * min(w.sample_bytes, depth // 8)) * (w.channels * min(w.sample_bytes, depth // 8)) in sizes
        (tmp_path / f"lane_{name}.bin").write_bytes(data)
        (tmp_path / f"lane_{name}.want").write_bytes(want)
        (tmp_path / f"lane_{name}.pieces").write_text(" ".join(str(x) for x in sizes) + "\n")
        manifest.append(f"{stem}.bin {stem}.want {stem}.pieces {1 if w is None else 0} {depth} {seek} {fields}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")
    out = run("gpu", str(tmp_path / "manifest.txt"))
    assert " 0 failures" in out and "byte-exact" in out, out
