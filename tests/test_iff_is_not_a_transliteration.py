"""The PCM file layer's files against the reference files whose behaviour they answer to, the way
tests/test_mp4_is_not_a_transliteration.py holds the MPEG-4 layer: normalised line overlap (tools/overlap.py) must stay below 20 %.
Every new product, test and tool file answers to OpenHome/Media/Codec/Wav.cpp, AiffBase.h, AiffBase.cpp, Aiff.cpp and Aifc.cpp, none
of whose text may be restated.  Runs where the reference tree exists, skipped elsewhere."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "OpenHome", "Media", "Codec", "Wav.cpp")), reason="the reference tree only exists in the build container")

THEIRS = ["OpenHome/Media/Codec/Wav.cpp", "OpenHome/Media/Codec/AiffBase.h", "OpenHome/Media/Codec/AiffBase.cpp", "OpenHome/Media/Codec/Aiff.cpp",
          "OpenHome/Media/Codec/Aifc.cpp"]
MINE = ["ohpipeline_amd/csrc/iff_chunk_core.h", "ohpipeline_amd/csrc/iff_pcm_kernel.hip", "ohpipeline_amd/csrc/api_iff.hip", "tests/cpp/iff_core_driver.cpp",
        "tests/iff_textbook.py", "tests/iff_cases.py", "tests/test_iff_textbook.py", "tests/test_iff_core_cpu.py", "tests/test_iff_abi_host.py",
        "tests/test_gpu_iff_textbook.py", "tests/test_gpu_iff_to_pcm.py", "tools/bench_iff.py", "ohpipeline_amd/host/PcmFileDecoder.h", "ohpipeline_amd/host/PcmFileDecoder.cpp",
        "tests/cpp/test_pcm_file_decoder.cpp", "tests/test_iff_host_cpp.py", "ohpipeline_amd/csrc/field_bytes.h", "ohpipeline_amd/csrc/api_file.h"]


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
