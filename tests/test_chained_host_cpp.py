"""Builds and runs tests/cpp/test_chained_decoder.cpp: a chained Ogg stream through the host element (OggVorbisBatchDecoder across
links; DESIGN.md 5.23's addendum), held to what a player must put out of every link (tests/chained_cases.played, which
tests/test_chained_tremor.py holds to Tremor).  Without a GPU the device is stood in for between CollectLinks and ApplyLinks from a
truth file the models write, and the committed chains are pushed in small and in large steps.  Asserted on the events the sink and the
comment observer got: at a link the old link's PCM, a decoded-stream message only where channels or rate change, the comment packet,
the new link's PCM; every link's sample count with its trims (the last page's granule, a first granule of 1 000 000, a negative one);
and that the element waits at a link whose head is open.  With a GPU: a two-link lane and a plain lane in the same
Tick(), one fused call a tick, every link's samples within 1 LSB of the model's."""
import os
import subprocess

import numpy as np
import pytest

import chained_cases as KC
import vorbis_cases as VC
import vorbis_frames as VF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
EXE = os.path.join(BUILD, "test_chained_decoder")
COMMENT_BYTES = len(VF.COMMENT)


def build_test_binary():
    from ohpipeline_amd import build as product_build
    product_build.build()
    product_build.build_host()
    os.makedirs(BUILD, exist_ok=True)
    src = os.path.join(ROOT, "tests", "cpp", "test_chained_decoder.cpp")
    lib_dir = os.path.join(ROOT, "ohpipeline_amd", "lib")
    deps = [src, os.path.join(lib_dir, "libohhost.so"), os.path.join(lib_dir, "libohgpu.so")]
    if os.path.exists(EXE) and all(os.path.getmtime(d) <= os.path.getmtime(EXE) for d in deps):
        return EXE
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE,
                           "-L", lib_dir, "-lohhost", "-lohgpu", f"-Wl,-rpath,{lib_dir}", "-lpthread"])
    return EXE


def run(*args):
    exe = build_test_binary()
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        lines = out.stdout.splitlines()
        raise AssertionError("\n".join(sorted(set(lines), key=lines.index)[:60]) + out.stderr[-2000:])
    return out.stdout


def expected_events(chain):
    """S<channels>:<rate> only where either changes, M<comment bytes>, A<samples a channel> per link"""
    words, said = [], None
    for channels, rate, pcm in KC.played(chain):
        if said != (channels, rate):
            words.append(f"S{channels}:{rate}")
            said = (channels, rate)
        words += [f"M{COMMENT_BYTES}", f"A{pcm.shape[1]}"]
    return " ".join(words)


def truth(chain, tmp_path):
    data = KC.ogg(chain)
    links, m = KC.links_of(data)
    where, at, start = [], 0, None                        # per packet: (page offset, segment, page number, the byte at which it is whole)
    while at < len(data):
        nseg, seq = data[at + 26], int.from_bytes(data[at + 18:at + 22], "little")
        end = at + 27 + nseg + sum(data[at + 27:at + 27 + nseg])
        for s in range(nseg):
            if start is None:
                start = (at, s, seq)
            if data[at + 27 + s] < 255:
                where.append(start + (end,))
                start = None
        at = end
    assert len(where) == len(m["packets"])
    lines, rows = [], []
    for j, (serial, page, first, packets) in enumerate(links):
        setup, recs, _ = KC.decode_link(packets)
        lines.append(f"{page} {serial} {setup.channels} {setup.rate} {setup.bs[0]} {setup.bs[1]}")
        for k, (pk, r) in enumerate(zip(packets, recs)):
            w = where[first + k]
            assert (w[0], w[1], w[2]) == (pk["page_offset"], pk["segment"], pk["page_seq"])
            rows.append(f"{j} {w[0]} {w[1]} {w[2]} {w[3]} {pk['granule']} {pk['flags'] & 2} {r[3]} {1 if k >= 3 else 0}")
    (tmp_path / "chain.ogg").write_bytes(data)
    (tmp_path / "truth.txt").write_text("\n".join([f"{len(rows)} {len(links)}"] + lines + rows) + "\n")
    return str(tmp_path / "chain.ogg"), str(tmp_path / "truth.txt")


@pytest.mark.parametrize("step", [61, 700, 100000])
@pytest.mark.parametrize("chain", sorted(KC.CHAINS))
def test_the_messages_at_a_link_with_a_stand_in_for_the_device(tmp_path, chain, step):
    out = run("cpu", *truth(chain, tmp_path), step)
    assert " 0 failures" in out, out
    events = next(l for l in out.splitlines() if l.startswith("events: "))[8:].strip()
    assert events == expected_events(chain), out
    waited = int(next(l for l in out.splitlines() if l.startswith("open: ")).split()[1])
    if step == 100000:
        assert waited == 0 and " ticks: 1 " in out, out               # the whole chain in one tick


@pytest.mark.parametrize("chain", sorted(KC.CHAINS))
def test_the_wait_at_a_link_whose_head_is_open(tmp_path, chain):
    """The first push ends inside the second link's setup packet, its first page whole: the call answers HEAD_OPEN for that link, the
    element puts out the first link, cuts its queue at the link's first page and waits; the rest comes with the second push."""
    second = KC.links_of(KC.ogg(chain))[0][1]
    first_push = second[1] + second[3][1]["page_offset"] - second[3][0]["page_offset"] + 100
    out = run("cpu", *truth(chain, tmp_path), 100000, first_push)
    assert " 0 failures" in out and "open: 1 ticks: 2 " in out, out
    assert next(l for l in out.splitlines() if l.startswith("events: "))[8:].strip() == expected_events(chain), out


def test_the_expected_events_say_what_the_chains_were_built_for():
    assert expected_events("chain_mono_stereo") == f"S1:44100 M{COMMENT_BYTES} A288 S2:44100 M{COMMENT_BYTES} A3840"
    assert expected_events("chain_negative_g0") == f"S1:44100 M{COMMENT_BYTES} A240 M{COMMENT_BYTES} A348"          # no second decoded-stream message
    assert expected_events("chain_trimmed").split()[2] == "A507" and expected_events("chain_million").split()[-1] == "A480"


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["chain_mono_stereo", "chain_negative_g0", "chain_mono_eight"])
def test_a_two_link_lane_and_a_plain_lane_in_the_same_tick(tmp_path, chain):
    plain = "stereo_clips"
    (tmp_path / "chain.ogg").write_bytes(KC.ogg(chain))
    (tmp_path / "plain.ogg").write_bytes(VC.ogg(plain))
    out = run("gpu", tmp_path / "chain.ogg", tmp_path / "plain.ogg", 900, tmp_path / "chain.pcm", tmp_path / "plain.pcm")
    assert " 0 failures" in out, out
    lanes = [l.split("events: ")[1].strip() for l in out.splitlines() if l.startswith("lane ")]
    pcm = VC.expected(plain)[2]
    assert lanes == [expected_events(chain), f"S{pcm.shape[0]}:44100 M{COMMENT_BYTES} A{pcm.shape[1]}"], out
    got = np.fromfile(str(tmp_path / "chain.pcm"), dtype=">i2").astype(np.int64)
    want = np.concatenate([p.T.reshape(-1) for _, _, p in KC.played(chain)])
    assert got.size == want.size and int(np.abs(got - want).max()) <= 1
    got = np.fromfile(str(tmp_path / "plain.pcm"), dtype=">i2").astype(np.int64)
    assert got.size == pcm.size and int(np.abs(got - pcm.T.reshape(-1)).max()) <= 1
