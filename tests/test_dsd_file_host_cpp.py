"""Builds and runs tests/cpp/test_dsd_file_decoder.cpp: DSD files in the host adapter (DsfRecognise, DffRecognise,
DsdFileBatchDecoder, CodecController::OutputDecodedStreamDsd).  Without a GPU: the two recognition rules, a decoder
before its first tick, the seek's two grids, and the host-side walk over every lane's file as it arrives.  With one: five lanes -- a
DSF file that ends inside a sample block, with a seek as soon as its stream has been announced; a DFF file with a seek; a DSF file
whose bytes are MSB first, which throws CodecStreamFeatureUnsupported; a DFF file whose PROP claims more than the file holds, which
throws CodecStreamCorrupt once its stream has ended; and a file that is no DSD file, which is dropped as not recognised and throws
nothing -- pushed in 20 000-byte pieces over several ticks, one Flush per tick.  The MsgDecodedStream fields, the messages' sizes
(whole sample blocks) and track offsets, the 0x69 fill at the stream's end alone, the track offsets of both seek formulas and the bytes
that reach ProcessorDsdBufTest must be what the model and the tests' own writer say."""
import os
import struct
import subprocess

import pytest

import dsd_file_cases as FC
import dsd_file_textbook as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_dsd_file_decoder")
MAX_PIECE = 9216                     # DecodedAudio::kMaxBytes
PUSH = 20000                         # kPush


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_dsd_file_decoder.cpp")
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


def expectations(data, W, P, seek):
    """The bytes the lane must deliver and its messages' sizes: at every tick the model over what has arrived, from the chunk the
    lane stands at and with the room the element gives it (a seek moves the lane once, behind the tick that announced the stream), cut
    into pieces of whole sample blocks within MAX_PIECE."""
    piece = MAX_PIECE - MAX_PIECE % (W * 4)
    want, sizes, at, sought, fills = bytearray(), [], 0, False, 0
    for tick in range(-(-len(data) // PUSH)):
        arrived = min(len(data), PUSH * (tick + 1))
        m = FX.read(data[:arrived], W, P, chunk_first=at, dst_bytes_capacity=(arrived // 4 // (W - P) + 1) * W * 4)
        if m["status"] != FX.OK:
            assert m["status"] == FX.TRUNCATED and arrived < len(data)
            continue
        body = m["blocks"]
        fills += m["bytes_written"] > m["chunks_written"] * (4 + P)
        assert at + m["chunks_written"] == m["chunks_total"] or m["bytes_written"] == m["chunks_written"] * (4 + P)     # the fill at the stream's end alone
        want += body
        sizes += [min(piece, len(body) - k) for k in range(0, len(body), piece)]
        at += m["chunks_written"]
        if seek >= 0 and not sought:
            at, sought = FX.seek(m["kind"], seek)[0], True
    return bytes(want), sizes, fills


def lanes():
    dsf = FC.make(FX.DSF, 5 * 2048 + 1001, 81)                                  # 11241 chunks = 4 x 2810 + 1: ends inside a block of (6, 2)
    dff = FC.make(FX.DFF, 12000 + 2, 82, rate=5644800, locals_before=[FC.junk(b"ABSS", 7)])
    msb = FC.make(FX.DSF, 3000, 83, bits=8)
    good = FC.make(FX.DFF, 8000, 84)
    prop = good.marks["PROP"]
    cut = FC.patched(good, prop + 4, struct.pack(">Q", 1 << 20))              # its PROP claims more than the file holds
    return [("dsf", dsf, dsf.data, 6, 2, 40000, 0), ("dff", dff, dff.data, 2, 0, 50000, 0), ("msb_first", msb, msb.data, 8, 4, -1, 2),
            ("prop_cut", good, cut, 6, 2, -1, 1), ("none_of_them", None, b"RIFF\x24\0\0\0WAVEfmt " + bytes(30000), 1, 0, -1, 3)]


def write_manifest(tmp_path):
    manifest = []
    for name, w, data, W, P, seek, fate in lanes():
        stem = tmp_path / f"lane_{name}"
        if fate == 0:
            assert len(data) > 2 * PUSH and w.data_offset < PUSH                       # several ticks, the stream announced in the first
            want, sizes, fills = expectations(data, W, P, seek)
            assert (W - P == 1 or w.chunks_total % (W - P) == 0 or fills == 1) and MAX_PIECE - MAX_PIECE % (W * 4) in sizes
            assert want[-W * 4:] == w.blocks(W, P)[-W * 4:]                            # the stream's last block, fill and all
            fields = f"{w.kind} {w.rate} {w.sample_count} {w.chunks_total} {w.data_offset}"
        else:
            want, sizes, fields = b"", [], "0 0 0 0 0"
            assert fate != 1 or len(data) > PUSH                                       # corrupt only once the stream has ended, a tick later
        (tmp_path / f"lane_{name}.bin").write_bytes(data)
        (tmp_path / f"lane_{name}.want").write_bytes(want)
        (tmp_path / f"lane_{name}.pieces").write_text(" ".join(str(x) for x in sizes) + "\n")
        manifest.append(f"{stem}.bin {stem}.want {stem}.pieces {fate} {W} {P} {seek} {fields}")
    (tmp_path / "manifest.txt").write_text("\n".join(manifest) + "\n")
    return str(tmp_path / "manifest.txt")


def test_recognition_the_head_and_a_decoder_before_its_first_tick_without_a_device(tmp_path):
    out = run("cpu", write_manifest(tmp_path))
    assert "cpu:" in out and " 0 failures" in out


@pytest.mark.gpu
def test_five_lanes_from_file_bytes_to_processor_through_the_gpu(tmp_path):
    out = run("gpu", write_manifest(tmp_path))
    assert " 0 failures" in out and "byte-exact" in out, out
