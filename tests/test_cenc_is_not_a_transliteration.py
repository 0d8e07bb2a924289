"""The protected MPEG-4 layer's files against the reference files whose behaviour they answer to, the way
tests/test_mp4f_is_not_a_transliteration.py holds the fragmented layer: normalised line overlap (tools/overlap.py) must stay below 20 %.
Every new product and test file answers to OpenHome/Media/Codec/Mpeg4.cpp and Mpeg4.h, none of whose text may be restated.  Runs where
the reference tree exists, skipped elsewhere."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "OpenHome", "Media", "Codec", "Mpeg4.cpp")), reason="the reference tree only exists in the build container")

THEIRS = ["OpenHome/Media/Codec/Mpeg4.cpp", "OpenHome/Media/Codec/Mpeg4.h"]
MINE = ["ohpipeline_amd/csrc/cenc_core.h", "ohpipeline_amd/csrc/cenc_kernel.hip", "ohpipeline_amd/csrc/api_cenc.hip", "tests/cpp/cenc_core_driver.cpp",
        "tests/cenc_textbook.py", "tests/cenc_cases.py", "tests/far_cenc_cases.py", "tests/test_far_cenc_cases.py", "tests/test_cenc_textbook.py", "tests/test_cenc_cases.py", "tests/test_cenc_core_cpu.py", "tests/test_cenc_abi_host.py",
        "tests/test_gpu_cenc_textbook.py", "tests/test_gpu_cenc_to_pcm.py", "tests/test_gpu_cenc_far_offsets.py", "tests/golden/make_cenc_fixtures.py", "tools/bench_cenc.py", "ohpipeline_amd/host/Mpeg4CencDecoder.h", "ohpipeline_amd/host/Mpeg4CencDecoder.cpp",
        "tests/cpp/test_mpeg4_cenc_decoder.cpp", "tests/test_cenc_host_cpp.py"]


def test_the_list_holds_every_new_file():
    listed = {os.path.basename(m) for m in MINE}
    for folder in ("ohpipeline_amd/csrc", "ohpipeline_amd/host", "tests", "tests/cpp", "tools"):
        for name in os.listdir(os.path.join(ROOT, folder)):
            if "cenc" in name.lower() and name.endswith((".h", ".hip", ".cpp", ".py")) and name != os.path.basename(__file__):
                assert name in listed, name


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
