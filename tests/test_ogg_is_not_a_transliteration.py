"""The Ogg page layer's files against the reference files whose behaviour they answer to, the way
tests/test_ohm_rx_is_not_a_transliteration.py holds the Songcast receiver: normalised line overlap (tools/overlap.py) must stay below
20 %.  The core, the kernels, the API file, the CPU driver, the model, the tests' muxer, the fixture generator and the host element all answer to
thirdparty/libogg/src/framing.c and thirdparty/flac-1.2.1/src/libFLAC/ogg_decoder_aspect.c, none of whose text may be restated.  Runs
where the reference tree exists, skipped elsewhere."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "thirdparty", "libogg")), reason="the reference tree only exists in the build container")

THEIRS = ["thirdparty/libogg/src/framing.c", "thirdparty/flac-1.2.1/src/libFLAC/ogg_decoder_aspect.c"]
MINE = ["ohpipeline_amd/csrc/ogg_page_core.h", "ohpipeline_amd/csrc/ogg_page_kernel.hip", "ohpipeline_amd/csrc/api_ogg.hip", "tests/cpp/ogg_core_driver.cpp",
        "tests/ogg_textbook.py", "tests/ogg_cases.py", "tools/gen_ogg_golden.c", "tools/ogg_host_cpu.cpp", "ohpipeline_amd/host/OggFlacDecoder.cpp",
        "ohpipeline_amd/host/OggFlacDecoder.h", "tests/cpp/test_ogg_flac_decoder.cpp"]


@pytest.mark.parametrize("mine", MINE)
def test_overlap_with_the_reference_stays_low(mine):
    import overlap
    own = overlap.significant(os.path.join(ROOT, mine))
    ref = set()
    for name in THEIRS:
        assert os.path.isfile(os.path.join(REF, name)), name
        ref.update(overlap.significant(os.path.join(REF, name)))
    share = sum(1 for l in own if l in ref) / max(1, len(own))
    assert share < 0.20, f"{mine}: {100 * share:.1f} % of its significant lines are in {THEIRS}"
