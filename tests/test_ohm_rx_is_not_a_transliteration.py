"""The Songcast receiver's files against the reference files whose behaviour they answer to, the way
tests/test_alac_is_not_a_transliteration.py holds the Apple Lossless family: normalised line overlap (tools/overlap.py) must stay
below 20 %.  The core, the kernels, the API file, the CPU driver, the model and host/Receiver.* all answer to
OpenHome/Av/Songcast/{ProtocolOhBase, ProtocolOhm, ProtocolOhu, OhmMsg, Ohm}.*, none of whose text may be restated.  Runs where the
reference tree exists, skipped elsewhere."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "OpenHome")), reason="the reference tree only exists in the build container")

SONGCAST = ["OpenHome/Av/Songcast/ProtocolOhBase.*", "OpenHome/Av/Songcast/ProtocolOhm.*", "OpenHome/Av/Songcast/ProtocolOhu.*",
            "OpenHome/Av/Songcast/OhmMsg.*", "OpenHome/Av/Songcast/Ohm.*"]
MINE = ["ohpipeline_amd/csrc/ohm_rx_core.h", "ohpipeline_amd/csrc/ohm_rx_kernel.hip", "ohpipeline_amd/csrc/api_ohm_rx.hip", "tests/cpp/ohm_rx_core_driver.cpp",
        "tests/ohm_rx_textbook.py", "tests/ohm_rx_cases.py", "ohpipeline_amd/host/Receiver.cpp", "ohpipeline_amd/host/Receiver.h", "tests/cpp/test_receiver.cpp"]


@pytest.mark.parametrize("mine", MINE)
def test_overlap_with_the_reference_stays_low(mine):
    import overlap
    own = overlap.significant(os.path.join(ROOT, mine))
    ref = set()
    for pattern in SONGCAST:
        files = glob.glob(os.path.join(REF, pattern))
        assert files, pattern
        for f in files:
            ref.update(overlap.significant(f))
    share = sum(1 for l in own if l in ref) / max(1, len(own))
    assert share < 0.20, f"{mine}: {100 * share:.1f} % of its significant lines are in {SONGCAST}"
