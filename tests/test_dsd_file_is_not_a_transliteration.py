"""The DSD file layer's files against the reference files whose behaviour they answer to, the way
tests/test_iff_is_not_a_transliteration.py holds the PCM file layer: normalised line overlap (tools/overlap.py) must stay below 20 %.
Every new product, test and tool file answers to OpenHome/Media/Codec/DsdDsf.cpp and DsdDff.cpp, none of whose text may be restated.
Runs where the reference tree exists, skipped elsewhere."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "OpenHome", "Media", "Codec", "DsdDsf.cpp")), reason="the reference tree only exists in the build container")

THEIRS = ["OpenHome/Media/Codec/DsdDsf.cpp", "OpenHome/Media/Codec/DsdDff.cpp"]
MINE = ["ohpipeline_amd/csrc/dsd_file_core.h", "ohpipeline_amd/csrc/dsd_perm.h", "ohpipeline_amd/csrc/dsd_file_kernel.hip", "ohpipeline_amd/csrc/api_dsd_file.hip",
        "ohpipeline_amd/host/DsdFileDecoder.h", "ohpipeline_amd/host/DsdFileDecoder.cpp", "tests/cpp/dsd_file_core_driver.cpp", "tests/cpp/test_dsd_file_decoder.cpp",
        "tests/dsd_file_textbook.py", "tests/dsd_file_cases.py", "tests/test_dsd_file_textbook.py", "tests/test_dsd_file_core_cpu.py", "tests/test_dsd_file_abi_host.py",
        "tests/test_dsd_file_host_cpp.py", "tests/test_gpu_dsd_file_textbook.py", "tools/bench_dsd_file.py", "ohpipeline_amd/csrc/field_bytes.h", "ohpipeline_amd/csrc/api_file.h"]


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
