"""Builds and runs tests/cpp/test_mpegts_demuxer.cpp: the transport stream element of the host adapter (MpegTsAdtsBatchDemuxer,
MpegTsRecognise, AdtsRecognise, Id3v2Skip).  Without a GPU: the recognisers, and three lanes -- an HLS-like segment, one
with every PES packet a frame and a counter jump, one that ends in a corrupt packet -- pushed in ragged pieces over many ticks with
csrc/ts_packet_core.h on the CPU standing in for the device between Collect and Apply.  With one: the same lanes through
MpegTsAdtsBatchDemuxer::Tick, one fused device call a tick.  Either way the frames that reach the sink must be the ones the model
(tests/ts_textbook.py) finds in the whole stream at once: their offsets in the elementary stream, their bytes, and the PTS of the PES
packet that holds their first byte; and the state carried at the end must be the model's."""
import os
import subprocess

import pytest

import ts_cases as TC
import ts_textbook as TX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_mpegts_demuxer")


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_mpegts_demuxer.cpp")
    lib_dir = os.path.join(ROOT, "ohpipeline_amd", "lib")
    deps = [src, os.path.join(lib_dir, "libohhost.so"), os.path.join(lib_dir, "libohgpu.so"), os.path.join(ROOT, "ohpipeline_amd", "csrc", "ts_packet_core.h")]
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


def lane(tmp_path, name, data, piece_sizes):
    """The files of one lane: what the model says of the whole stream at once is what the element must deliver piece by piece."""
    m = TX.demux(data)
    a = TX.adts_chain(m["run"], TX.RECOGNISE)
    assert a["status"] == TX.ADTS_OK and len(a["frames"]) > 20
    stamps = [(r["es_offset"], r["pts"]) for r in m["pes"]]
    lines = []
    for f in a["frames"]:
        pts = [p for at, p in stamps if at <= f["offset"]]
        lines.append(f"{f['offset']} {f['bytes']} {pts[-1] if pts and pts[-1] != TX.NO_PTS else -1}")
    pieces, at, k = [], 0, 0
    while at < len(data):
        n = min(piece_sizes[k % len(piece_sizes)], len(data) - at)
        pieces.append(n)
        at += n
        k += 1
    stem = tmp_path / name
    (tmp_path / f"{name}.ts").write_bytes(data)
    (tmp_path / f"{name}.es").write_bytes(m["run"])
    (tmp_path / f"{name}.want").write_text("\n".join(lines) + "\n")
    (tmp_path / f"{name}.pieces").write_text(" ".join(str(n) for n in pieces) + "\n")
    (tmp_path / f"{name}.state").write_text(f"{m['pmt_pid']} {m['audio_pid']} {m['pes_open_bytes']} {len(m['run']) - a['bytes_consumed']} {int(m['status'] == TX.CORRUPT)}\n")
    return str(stem)


def lanes(tmp_path):
    rng = TC.Lcg(31)
    packets, _ = TC.segment(rng, 90, frames_per_pes=5)
    first = lane(tmp_path, "segment", b"".join(packets), [1000, 333, 4000, 188, 7])
    packets, _ = TC.segment(rng, 60, frames_per_pes=1, tables_every=7)
    jumped = packets[:40] + packets[41:]                                 # a packet lost: a counter jump, and a frame cut short
    second = lane(tmp_path, "lossy", b"".join(jumped)[:-50], [2500, 61])
    packets, _ = TC.segment(rng, 50, frames_per_pes=2)
    third = lane(tmp_path, "corrupt", b"".join(packets[:45] + [TC.packet(TC.OTHER_PID, b"", adaptation=184)] + packets[45:]), [188 * 9, 188 * 2])
    return first, second, third


def test_the_recognisers_and_the_element_with_the_core_standing_in_for_the_device(tmp_path):
    out = run("cpu", *lanes(tmp_path))
    assert "cpu:" in out and " 0 failures" in out and out.count("byte-exact") == 3, out


@pytest.mark.gpu
def test_three_lanes_from_transport_bytes_to_the_frame_sink_through_the_gpu(tmp_path):
    out = run("gpu", *lanes(tmp_path))
    assert " 0 failures" in out and out.count("byte-exact") == 3, out
