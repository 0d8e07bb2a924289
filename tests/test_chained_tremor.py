"""What a player puts out of a chained Ogg Vorbis file (tests/chained_cases.played: the links of tests/ogg_links_textbook.py, each
decoded by tests/vorbis_textbook.py and trimmed by its own granule positions) held to Tremor's vorbisfile.c, the code through which
the reference follows a chain (Codec/Vorbis.cpp:398-438).  Where /root/reference exists, and skipped elsewhere as
tests/test_vorbis_tremor.py is, Tremor WITH vorbisfile.c and its libogg are compiled with tests/cpp/tremor_chain_driver.c into
pytest's temporary directory, never into the tree; the driver reads through callbacks that cannot seek, ov_read until 0, and logs the
bitstream index, ov_info and the byte count of every read.  The files are the four chains built from vorbis_cases.TREMOR_SHAPES: mono
into stereo with other block sizes, a link whose granules begin at 1 000 000, a link trimmed at its last page, a link with a negative
first granule (the specification's start trim -- what Tremor does there decides what the model does).  Asserted: the same number of
links, the same channels and rate a link, the same sample count a link, and PCM within the 2 LSB tests/test_vorbis_tremor.py asserts,
for its stated reason (measured there: 1 LSB)."""
import glob
import os
import subprocess

import numpy as np
import pytest

import chained_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/thirdparty"
MEASURED_LSB = 1
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "Tremor", "vorbisfile.c")), reason="the reference tree only exists in the build container")


@pytest.fixture(scope="module")
def tremor(tmp_path_factory):
    out = tmp_path_factory.mktemp("tremor_chain") / "driver"
    parts = ("block", "codebook", "floor0", "floor1", "info", "mapping0", "mdct", "registry", "res012", "sharedbook", "synthesis", "window", "vorbisfile")
    subprocess.run(["gcc", "-O1", "-w", "-I", os.path.join(REF, "libogg", "include"), "-I", os.path.join(REF, "Tremor")] +
                   [os.path.join(REF, "Tremor", p + ".c") for p in parts] + sorted(glob.glob(os.path.join(REF, "libogg", "src", "*.c"))) +
                   [os.path.join(ROOT, "tests", "cpp", "tremor_chain_driver.c"), "-o", str(out)], check=True, timeout=300)
    return out


@pytest.mark.parametrize("chain", KC.TREMOR_CHAINS)
def test_the_links_a_player_puts_out_are_tremors(tremor, tmp_path, chain):
    (tmp_path / "chain.ogg").write_bytes(KC.ogg(chain))
    r = subprocess.run([str(tremor), str(tmp_path / "chain.ogg"), str(tmp_path / "pcm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1].startswith("OK"), (r.stdout[-500:], r.stderr[-1000:])
    reads = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()[:-1]]
    raw = np.fromfile(str(tmp_path / "pcm"), dtype="<i2").astype(np.int32)
    got, at = [], 0                                       # per link: (channels, rate, samples [channels][n]); a link is a run of reads of one index
    for k, (index, channels, rate, nbytes) in enumerate(reads):
        if k == 0 or index != reads[k - 1][0]:
            got.append([channels, rate, []])
        assert (channels, rate) == tuple(got[-1][:2])
        got[-1][2].append(raw[at:at + nbytes // 2])
        at += nbytes // 2
    assert at == raw.size
    want = KC.played(chain)
    print(chain, "Tremor's links:", [(c, r_, sum(x.size for x in parts) // c) for c, r_, parts in got], "the model's:", [(c, r_, pcm.shape[1]) for c, r_, pcm in want])
    assert len(got) == len(want)
    worst = 0
    for (channels, rate, parts), (ch, rt, pcm) in zip(got, want):
        mine = np.concatenate(parts).reshape(-1, channels).T
        assert (channels, rate, mine.shape[1]) == (ch, rt, pcm.shape[1])
        worst = max(worst, int(np.abs(mine - pcm).max()))
    print(f"{chain}: largest difference from Tremor {worst} LSB")
    assert worst <= 2 * MEASURED_LSB
