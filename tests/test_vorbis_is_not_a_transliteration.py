"""The Vorbis decoder's files against the reference files whose behaviour they answer to, the way
tests/test_ts_is_not_a_transliteration.py holds the transport stream layer: normalised line overlap (tools/overlap.py) must stay below
20 %.  Every new product, test and tool file answers to OpenHome/Media/Codec/Vorbis.cpp and to the .c files of the reference's Tremor,
none of whose text may be restated.  Runs where the reference tree exists, skipped elsewhere."""
import glob
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "OpenHome", "Media", "Codec", "Vorbis.cpp")), reason="the reference tree only exists in the build container")

MINE = ["include/ohgpu_vorbis.h", "ohpipeline_amd/csrc/vorbis_core.h", "ohpipeline_amd/csrc/vorbis_kernel.hip", "ohpipeline_amd/csrc/api_vorbis.hip",
        "tests/cpp/vorbis_core_driver.cpp", "tests/vorbis_textbook.py", "tests/vorbis_frames.py", "tests/vorbis_cases.py", "tests/test_vorbis_core_cpu.py",
        "tests/test_gpu_vorbis_textbook.py", "tests/test_gpu_vorbis_far_offsets.py", "tests/test_vorbis_tremor.py", "tests/test_gpu_vorbis_ogg.py", "tests/test_vorbis_host_cpp.py", "tests/cpp/test_vorbis_decoder.cpp", "ohpipeline_amd/host/VorbisDecoder.h", "ohpipeline_amd/host/VorbisDecoder.cpp", "tests/test_vorbis_fixtures.py", "tests/golden/make_vorbis_fixtures.py", "tests/cpp/vorbis_tremor_driver.c", "tools/bench_vorbis.py", "tools/vorbis_host_cpu.cpp",
        "tests/vorbis_device.py", "tests/test_gpu_vorbis_damage.py"]
NAME = re.compile(r"vorbis", re.I)


def theirs():
    return [os.path.join(REF, "OpenHome", "Media", "Codec", "Vorbis.cpp")] + sorted(glob.glob(os.path.join(REF, "thirdparty", "Tremor", "*.c")))


def test_the_list_holds_every_new_file():
    listed = {os.path.basename(m) for m in MINE}
    for folder in ("include", "ohpipeline_amd/csrc", "ohpipeline_amd/host", "tests", "tests/cpp", "tests/golden", "tools"):
        for name in os.listdir(os.path.join(ROOT, folder)):
            if NAME.search(name) and name.endswith((".h", ".hip", ".cpp", ".c", ".py")) and name != os.path.basename(__file__):
                assert name in listed, name
    for m in MINE:
        assert os.path.isfile(os.path.join(ROOT, m)), m
    assert len(theirs()) > 10


@pytest.mark.parametrize("mine", MINE)
def test_overlap_with_the_reference_stays_low(mine):
    import overlap
    own = overlap.significant(os.path.join(ROOT, mine))
    ref = set()
    for name in theirs():
        ref.update(overlap.significant(name))
    share = sum(1 for l in own if l in ref) / max(1, len(own))
    assert share < 0.20, f"{mine}: {100 * share:.1f} % of its significant lines are in the reference's Vorbis.cpp and Tremor"
