"""Builds and runs tests/cpp/test_mpeg4_cbcs_decoder.cpp: the host element's all-schemes option (Mpeg4CencBatchDecoder made with
aAllSchemes, served by ohgpu_cbcs_*), in the shape of tests/test_cenc_host_cpp.py -- whose suite runs untouched and holds
the element without the option to what it did.  Without a GPU: a `cbcs` stream is Other to the element as it was and Flac with the
option, the head is read and the provider asked once when the byte the muxer's record names has arrived, the wide head has the pattern
and the constant IV.  With one: seven lanes pushed in 3000-byte pieces, one Flush per tick -- `cbcs` 1:9 fLaC under a constant IV, `cbcs`
fLaC and alac with subsample entries, `cenc` fLaC with entries, a whole-sample `cenc` lane WITHOUT the option beside them (both families
in one tick), a lane whose key the provider lacks and a `cbcs` stream in a lane without the option (both throw
CodecStreamFeatureUnsupported after every lane was served and deliver nothing).  The bytes that reach ProcessorPcmBufTest must be the
packed big-endian form of the PCM the samples were encoded from."""
import os
import subprocess

import pytest

import cbcs_cases as BC
import cenc_cases as CC
from test_cenc_host_cpp import alac_pcm, flac_pcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_mpeg4_cbcs_decoder")
CONSTANT = dict(pattern=(1, 9), constant_iv=bytes(range(0x70, 0x80)), senc=None)
ENTRIES = dict(iv_size=8, pattern=(1, 1), layout=lambda i, size: [(min(size, 9), max(size - 13, 0)), (min(max(size - 9, 0), 4), 0)])
CTR = dict(scheme=BC.CENC, iv_size=16, layout=lambda i, size: [(min(size, 4), (size - min(size, 4)) // 2), (0, size - min(size, 4) - (size - min(size, 4)) // 2)])


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_mpeg4_cbcs_decoder.cpp")
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


def head_args(tmp_path):
    m, _ = BC.flac_file("s8_mono_8k_b256_l2", 4, 0, **CONSTANT)
    (tmp_path / "cbcs.mp4").write_bytes(m.data)
    assert m.init_bytes == m.find("moov")[2]
    return [str(tmp_path / "cbcs.mp4"), str(m.init_bytes), m.kid.hex(), m.key.hex(), "1", "9", "16"]


def test_recognition_and_the_head_without_a_device(tmp_path):
    out = run("cpu", *head_args(tmp_path))
    assert "cpu:" in out and " 0 failures" in out


@pytest.mark.gpu
def test_seven_lanes_of_both_families_through_the_gpu(tmp_path):
    a, _ = BC.flac_file("s16_stereo_44k1_b1152_l5", 2, 1, **CONSTANT)
    b, _ = BC.flac_file("s24_stereo_44k1_b576_l0", 3, 2, **ENTRIES)
    c = BC.alac_file("stereo16_fl1024", 1, 3, **ENTRIES)
    d, _ = BC.flac_file("s16_stereo_44k1_b1152_l5", 2, 4, **CTR)
    e = CC.flac_file("s8_mono_8k_b256_l2", per_fragment=4, key=CC.key_of(5), kid=CC.kid_of(5), iv_size=8)
    keyless, _ = BC.flac_file("s8_mono_8k_b256_l2", 4, 6, **ENTRIES)
    narrow, _ = BC.flac_file("s8_mono_8k_b256_l2", 4, 7, **CONSTANT)
    assert b.subsamples == 2 * b.n and c.subsamples == 2 * c.n and d.subsamples == 2 * d.n and a.subsamples == 0
    lanes = [("cbcs_1_9", a, flac_pcm(a)[0], 0, 1, a.key.hex()), ("cbcs_entries", b, flac_pcm(b)[0], 0, 1, b.key.hex()), ("cbcs_alac", c, alac_pcm(c)[0], 0, 1, c.key.hex()),
             ("cenc_entries", d, flac_pcm(d)[0], 0, 1, d.key.hex()), ("cenc_whole_without_the_option", e, flac_pcm(e)[0], 0, 0, e.key.hex()),
             ("keyless", keyless, b"", 2, 1, "-"), ("cbcs_without_the_option", narrow, b"", 2, 0, narrow.key.hex())]
    manifest = []
    for name, m, want, throws, wide, key in lanes:
        stem = tmp_path / f"lane_{name}"
        (tmp_path / f"lane_{name}.mp4").write_bytes(m.data)
        (tmp_path / f"lane_{name}.want").write_bytes(want)
        manifest.append(f"{stem}.mp4 {stem}.want {throws} {wide} {m.kid.hex()} {key}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")
    out = run("gpu", *head_args(tmp_path), str(tmp_path / "manifest.txt"))
    assert " 0 failures" in out and "byte-exact" in out, out
