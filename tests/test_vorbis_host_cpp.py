"""Builds and runs tests/cpp/test_vorbis_decoder.cpp: Ogg Vorbis in the host adapter (VorbisRecognise, OggVorbisBatchDecoder; DESIGN.md
5.23).  Without a GPU: the recognition rule, the head split over ragged pushes, the refusals, and the element's ticks with the device
stood in for between Collect and Apply from a truth file the model writes -- the priming packet sent again, the trim at the last page's
granule position (set 37 samples short of what the packets decode to), whole-sample pieces within DecodedAudio::kMaxBytes.  With one: the
same lane through Tick(), one fused call a tick, every sample within 1 LSB of the model's."""
import os
import subprocess

import pytest

import vorbis_cases as VC
import vorbis_frames as VF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_vorbis_decoder")
NAME = "stereo_256_2048"
TRIM = 37


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_vorbis_decoder.cpp")
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


def files(tmp_path):
    """The stream as an Ogg file whose last page's granule is TRIM short, the truth about its audio packets, the model's PCM."""
    st, (recs, _, pcm) = VC.stream(NAME), VC.expected(NAME)
    granules = VC.granules(NAME)
    granules[-1] -= TRIM
    data = VF.ogg_file(st, granules, max_segments=17)
    where, at, index, seq = [], 0, 0, 0               # per packet: (page offset, segment, page number, the byte at which it is whole)
    start = None
    while at < len(data):
        nseg = data[at + 26]
        body = sum(data[at + 27:at + 27 + nseg])
        end = at + 27 + nseg + body
        for s in range(nseg):
            if start is None:
                start = (at, s, seq)
            if data[at + 27 + s] < 255:
                where.append(start + (end,))
                start = None
        at, seq = end, seq + 1
    audio = where[3:]
    assert len(audio) == len(recs) and audio[0][1] == 0
    lines = [f"{len(audio)} {st.model.channels} {granules[-1]} {audio[0][0]}"]
    lines += [f"{w[0]} {w[1]} {w[2]} {w[3]} {r[3]} {r[4]}" for w, r in zip(audio, recs)]
    (tmp_path / "stream.ogg").write_bytes(data)
    (tmp_path / "truth.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "pcm.s16be").write_bytes(VC.pcm_s16be(pcm))
    return str(tmp_path / "stream.ogg"), str(tmp_path / "truth.txt"), str(tmp_path / "pcm.s16be")


def test_recognise_head_and_the_ticks_with_a_stand_in_for_the_device(tmp_path):
    out = run("cpu", *files(tmp_path))
    assert "stand-in:" in out and " 0 failures" in out, out


@pytest.mark.gpu
def test_a_lane_from_file_bytes_to_the_processor_through_the_gpu(tmp_path):
    out = run("gpu", *files(tmp_path))
    assert "device:" in out and " 0 failures" in out, out
