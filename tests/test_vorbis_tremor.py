"""The model (tests/vorbis_textbook.py) held to Tremor, the decoder the reference plays Vorbis through: where /root/reference exists, and
skipped elsewhere, Tremor and its libogg are compiled with tests/cpp/vorbis_tremor_driver.c into pytest's temporary directory, never into
the tree, and decode the minimal encoder's stream and the streams of tests/vorbis_cases.TREMOR_SHAPES (which says where those keep to
what an encoder writes, and why).  Tremor computes in fixed point; its error is not known beforehand.  Measured on these streams
(profiles/vorbis_summary.md): the largest difference from the model's PCM is 1 LSB.  Asserted: twice that, because the streams sample
few block sizes and levels.  A mis-read specification differs by the signal itself, thousands of LSB: the margin hides nothing -- while
this test was written it told apart, at once, a class word taken modulo and a floor's tail, both of which Tremor reads otherwise."""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import vorbis_cases as VC
import vorbis_frames as VF
import vorbis_textbook as TB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/thirdparty"
MEASURED_LSB = 1
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "Tremor", "synthesis.c")), reason="the reference tree only exists in the build container")


@pytest.fixture(scope="module")
def tremor(tmp_path_factory):
    out = tmp_path_factory.mktemp("tremor") / "driver"
    parts = ("block", "codebook", "floor0", "floor1", "info", "mapping0", "mdct", "registry", "res012", "sharedbook", "synthesis", "window")
    subprocess.run(["gcc", "-O1", "-w", "-I", os.path.join(REF, "libogg", "include"), "-I", os.path.join(REF, "Tremor")] +
                   [os.path.join(REF, "Tremor", p + ".c") for p in parts] + sorted(glob.glob(os.path.join(REF, "libogg", "src", "*.c"))) +
                   [os.path.join(ROOT, "tests", "cpp", "vorbis_tremor_driver.c"), "-o", str(out)], check=True, timeout=300)
    return out


def decode(tremor, tmp_path, st):
    case = struct.pack("<I", len(st.ident)) + st.ident + struct.pack("<I", len(st.setup)) + st.setup + struct.pack("<I", len(st.packets))
    for p in st.packets:
        case += struct.pack("<I", len(p)) + p
    (tmp_path / "case").write_bytes(case)
    r = subprocess.run([str(tremor), str(tmp_path / "case"), str(tmp_path / "pcm")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stderr[-1000:]
    return np.fromfile(str(tmp_path / "pcm"), dtype="<i2").astype(np.int32).reshape(-1, st.model.channels).T


@pytest.mark.parametrize("name", ["minimal_encoder"] + sorted(VC.TREMOR_SHAPES))
def test_the_model_is_tremor_within_its_fixed_point_error(tremor, tmp_path, name):
    if name == "minimal_encoder":
        t = np.arange(256 * 24)
        st = VF.encode(0.5 * np.sin(2 * np.pi * (0.01 + 0.00002 * t) * t))
        pcm = TB.decode_stream(st.model, st.packets)[2]
    else:
        st, pcm = VC.stream(name), VC.expected(name)[2]
    got = decode(tremor, tmp_path, st)
    assert got.shape == pcm.shape and np.abs(pcm).max() > 8000
    worst = int(np.abs(got - pcm).max())
    print(f"{name}: {pcm.shape[1]} samples a channel, peak {int(np.abs(pcm).max())}, largest difference from Tremor {worst} LSB, {int((got != pcm).sum())} samples differ")
    assert worst <= 2 * MEASURED_LSB
