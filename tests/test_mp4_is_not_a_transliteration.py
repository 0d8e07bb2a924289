"""The MPEG-4 container layer's files against the reference files whose behaviour they answer to, the way
tests/test_ogg_is_not_a_transliteration.py holds the Ogg layer: normalised line overlap (tools/overlap.py) must stay below 20 %.
Every new product, test and tool file answers to OpenHome/Media/Codec/Mpeg4.cpp, Mpeg4.h and AlacApple.cpp, none of whose text may be
restated.  Runs where the reference tree exists, skipped elsewhere."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "OpenHome", "Media", "Codec", "Mpeg4.cpp")), reason="the reference tree only exists in the build container")

THEIRS = ["OpenHome/Media/Codec/Mpeg4.cpp", "OpenHome/Media/Codec/Mpeg4.h", "OpenHome/Media/Codec/AlacApple.cpp"]
MINE = ["ohpipeline_amd/csrc/mp4_box_core.h", "ohpipeline_amd/csrc/mp4_table_kernel.hip", "ohpipeline_amd/csrc/api_mp4.hip", "tests/cpp/mp4_core_driver.cpp",
        "tests/mp4_textbook.py", "tests/mp4_cases.py", "tests/test_mp4_textbook.py", "tests/test_mp4_core_cpu.py", "tests/test_mp4_abi_host.py",
        "tests/test_gpu_mp4_textbook.py", "tests/test_gpu_mp4_alac_to_pcm.py", "tools/bench_mp4_alac.py", "ohpipeline_amd/host/Mpeg4AlacDecoder.h", "ohpipeline_amd/host/Mpeg4AlacDecoder.cpp",
        "tests/cpp/test_mpeg4_alac_decoder.cpp", "tests/test_mp4_host_cpp.py", "ohpipeline_amd/csrc/field_bytes.h"]


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
