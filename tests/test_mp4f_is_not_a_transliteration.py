"""The fragmented MPEG-4 layer's files against the reference files whose behaviour they answer to, the way
tests/test_mp4_is_not_a_transliteration.py holds the MPEG-4 layer: normalised line overlap (tools/overlap.py) must stay below 20 %.
Every new product and test file answers to OpenHome/Media/Codec/Mpeg4.cpp, Mpeg4.h and Flac.cpp, none of whose text may be restated.
Runs where the reference tree exists, skipped elsewhere."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "OpenHome", "Media", "Codec", "Mpeg4.cpp")), reason="the reference tree only exists in the build container")

THEIRS = ["OpenHome/Media/Codec/Mpeg4.cpp", "OpenHome/Media/Codec/Mpeg4.h", "OpenHome/Media/Codec/Flac.cpp"]
MINE = ["ohpipeline_amd/csrc/mp4_frag_core.h", "ohpipeline_amd/csrc/mp4_frag_kernel.hip", "ohpipeline_amd/csrc/api_mp4f.hip", "tests/cpp/mp4f_core_driver.cpp",
        "tests/mp4f_textbook.py", "tests/mp4f_cases.py", "tests/test_mp4f_textbook.py", "tests/test_mp4f_core_cpu.py", "tests/test_mp4f_abi_host.py",
        "tests/test_gpu_mp4f_textbook.py", "tests/test_gpu_mp4f_to_pcm.py", "tools/bench_mp4f.py", "tools/mp4f_serial.cpp", "ohpipeline_amd/host/Mpeg4FragmentDecoder.h", "ohpipeline_amd/host/Mpeg4FragmentDecoder.cpp",
        "tests/cpp/test_mpeg4_fragment_decoder.cpp", "tests/test_mp4f_host_cpp.py", "ohpipeline_amd/csrc/field_bytes.h"]


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
