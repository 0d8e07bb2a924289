"""Builds and runs tests/cpp/test_mpeg4_cenc_decoder.cpp: protected fragmented MPEG-4 in the host adapter (Mpeg4CencRecognise,
Mpeg4CencBatchDecoder, ICencKeyProvider), in the shape of tests/test_mp4f_host_cpp.py.  Without a GPU: the recognition
over the prefixes of a protected fLaC and a protected alac stream and of a plain .m4a, the peek over ragged pushes (the head is read,
and the provider asked once by the head's kid, exactly when the byte the muxer's record names has arrived), a provider that lacks the
key, the refusals.  With one: seven lanes -- fixtures of tests/golden/flac and tests/golden/alac cut into fragments and encrypted by the
tests' muxer (tests/cenc_cases.py), each under its own key and kid, IVs of 8 and 16 bytes -- pushed in 3000-byte pieces over several
ticks, one Flush per tick: two fLaC streams, an alac stream, a fLaC and an alac lane that each seek back to a frame inside the third
fragment's last sample once that fragment has arrived whole, a protected lane whose key the provider lacks (it throws
CodecStreamFeatureUnsupported after every lane was served and delivers nothing), and a clear alac stream.  The bytes that reach
ProcessorPcmBufTest must be the packed big-endian form of the PCM the samples were encoded from."""
import os
import subprocess

import pytest

import alac_cases as AC
import flac_cases as FLC
import mp4_cases as MC
import cenc_cases as CC
import mp4f_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_mpeg4_cenc_decoder")
PIECE = 3000


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_mpeg4_cenc_decoder.cpp")
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


def head_files(tmp_path):
    """a protected fLaC and a protected alac stream with the byte count at which each one's moov is whole by the muxer's own record, a
    plain .m4a, and the kid and key both streams are under"""
    flac, alac = CC.flac_file("s8_mono_8k_b256_l2", per_fragment=4), CC.alac_file("stereo16_fl1024", per_fragment=3)
    plain = MC.fixture_file(AC.load_fixture("stereo16_fl1024"), per_chunk=[2])
    for name, data in (("flac.mp4", flac.data), ("alac.mp4", alac.data), ("plain.m4a", plain.data)):
        (tmp_path / name).write_bytes(data)
    assert flac.init_bytes == flac.find("moov")[2] and alac.init_bytes == alac.find("moov")[2]
    return [str(tmp_path / "flac.mp4"), str(flac.init_bytes), str(tmp_path / "alac.mp4"), str(alac.init_bytes), str(tmp_path / "plain.m4a"), CC.KID.hex(), CC.KEY.hex()]


def test_recognition_the_peek_and_the_refusals_without_a_device(tmp_path):
    out = run("cpu", *head_files(tmp_path))
    assert "cpu:" in out and " 0 failures" in out


def flac_pcm(m):
    """the packed big-endian PCM of the fixture behind a fragmented file, by the FLAC model, and its bytes a frame"""
    fx = m.fixture
    res, arena = FLC.model(FLC.whole(fx, packed=True))
    unit = fx.info["channels"] * (fx.info["bits"] // 8)
    return arena[:fx.samples * unit].tobytes(), unit


def alac_pcm(m):
    fx = m.fixture
    width, unit = fx["meta"]["bits"] // 8, fx["cfg"]["channels"] * (fx["meta"]["bits"] // 8)
    return b"".join(fx["pcm"][i:i + width][::-1] for i in range(0, len(fx["pcm"]), width)), unit


def seek_plan(m):
    """a seek back into the third fragment, made at the end of the tick in which that fragment has arrived whole: (frame, the first
    frame it must report, its row, the extent from which on it is made, the frames delivered by then)"""
    row = max(s for s in range(m.n) if m.run_of[s] == 2)                         # the third fragment's last sample
    frame = m.first_frames[row] + m.frames[row] // 2
    ends = sorted(mark[3] for mark in m.marks if "/" not in mark[0])                 # the ends of the top-level boxes
    pushed = 0
    while True:
        pushed = min(len(m.data), pushed + PIECE)
        whole = max([e for e in ends if e <= pushed], default=0)
        if whole >= m.segment_ends[2]:
            break
    delivered = sum(f for f, r in zip(m.frames, m.run_of) if m.segment_ends[r] <= whole)
    assert m.first_frames[row] < delivered                                            # a seek backwards: the sample was delivered before
    return frame, m.first_frames[row], row, m.segment_ends[2], delivered


@pytest.mark.gpu
def test_seven_lanes_from_stream_bytes_to_processor_through_the_gpu(tmp_path):
    def flac(name, per, k, iv):
        return CC.flac_file(name, per_fragment=per, key=CC.key_of(k), kid=CC.kid_of(k), iv_size=iv)

    def alac(name, per, k, iv):
        return CC.alac_file(name, per_fragment=per, key=CC.key_of(k), kid=CC.kid_of(k), iv_size=iv)

    a, b = flac("s16_stereo_44k1_b1152_l5", 2, 1, 8), flac("s24_stereo_44k1_b576_l0", 3, 2, 16)
    c = alac("stereo16_fl1024", 1, 3, 16)
    d, e = flac("s16_stereo_44k1_b1152_l5", 2, 4, 16), alac("stereo16_fl1024", 1, 5, 8)
    assert len(a.runs) > 3 and len(c.runs) > 3 and all(len(m.runs) == len(m.segment_ends) for m in (a, c, d, e))
    assert all(m.protected and m.data.count(b"senc") == len(m.runs) for m in (a, b, c, d, e))
    lanes = []
    for name, m, pcm_of, seeks in (("flac16", a, flac_pcm, False), ("flac24", b, flac_pcm, False), ("alac", c, alac_pcm, False),
                                   ("flac_seeker", d, flac_pcm, True), ("alac_seeker", e, alac_pcm, True)):
        pcm, unit = pcm_of(m)
        if seeks:
            frame, first, row, whole, delivered = seek_plan(m)
            lanes.append((name, m.data, pcm[:delivered * unit] + pcm[first * unit:], 0, frame, first, row, whole, m.kid.hex(), m.key.hex()))
        else:
            lanes.append((name, m.data, pcm, 0, -1, 0, 0, 0, m.kid.hex(), m.key.hex()))
    keyless = flac("s8_mono_8k_b256_l2", 4, 6, 8)
    lanes.append(("keyless", keyless.data, b"", 2, -1, 0, 0, 0, keyless.kid.hex(), "-"))          # the provider has no key for this kid
    clear = FC.alac_file("stereo16_fl1024", per_fragment=2)
    lanes.append(("clear_alac", clear.data, alac_pcm(clear)[0], 0, -1, 0, 0, 0, bytes(16).hex(), "-"))
    manifest = []
    for name, data, want, throws, frame, first, row, whole, kid, key in lanes:
        stem = tmp_path / f"lane_{name}"
        (tmp_path / f"lane_{name}.mp4").write_bytes(data)
        (tmp_path / f"lane_{name}.want").write_bytes(want)
        manifest.append(f"{stem}.mp4 {stem}.want {throws} {frame} {first} {row} {whole} {kid} {key}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")
    out = run("gpu", *head_files(tmp_path), str(tmp_path / "manifest.txt"))
    assert " 0 failures" in out and "byte-exact" in out, out
