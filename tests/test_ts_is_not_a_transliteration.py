"""The transport stream and ADTS layer's files against the reference files whose behaviour they answer to, the way
tests/test_cenc_is_not_a_transliteration.py holds the protected MPEG-4 layer: normalised line overlap (tools/overlap.py) must stay below
20 %.  Every new product, test and tool file answers to OpenHome/Media/Codec/MpegTs.cpp, MpegTs.h, AacFdkAdts.cpp and Id3v2.cpp, none of
whose text may be restated.  Runs where the reference tree exists, skipped elsewhere."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "OpenHome", "Media", "Codec", "MpegTs.cpp")), reason="the reference tree only exists in the build container")

THEIRS = ["OpenHome/Media/Codec/MpegTs.cpp", "OpenHome/Media/Codec/MpegTs.h", "OpenHome/Media/Codec/AacFdkAdts.cpp", "OpenHome/Media/Codec/Id3v2.cpp"]
MINE = ["include/ohgpu_ts.h", "ohpipeline_amd/csrc/ts_packet_core.h", "ohpipeline_amd/csrc/ts_packet_kernel.hip", "ohpipeline_amd/csrc/api_ts.hip",
        "ohpipeline_amd/host/MpegTsDemuxer.h", "ohpipeline_amd/host/MpegTsDemuxer.cpp", "tests/cpp/ts_core_driver.cpp", "tests/cpp/test_mpegts_demuxer.cpp",
        "tests/ts_textbook.py", "tests/ts_cases.py", "tests/test_ts_textbook.py", "tests/test_ts_core_cpu.py", "tests/test_ts_abi_host.py", "tests/test_ts_host_cpp.py",
        "tests/test_gpu_ts_textbook.py", "tests/test_gpu_ts_lifecycle.py", "tests/test_gpu_ts_far_offsets.py", "tests/golden/make_ts_fixtures.py", "tools/bench_ts.py",
        "tools/ts_host_cpu.cpp"]
NAME = re.compile(r"(?:^|_)ts[_.]|mpegts|adts", re.I)


def test_the_list_holds_every_new_file():
    listed = {os.path.basename(m) for m in MINE}
    for folder in ("include", "ohpipeline_amd/csrc", "ohpipeline_amd/host", "tests", "tests/cpp", "tests/golden", "tools"):
        for name in os.listdir(os.path.join(ROOT, folder)):
            if NAME.search(name) and name.endswith((".h", ".hip", ".cpp", ".py")) and name != os.path.basename(__file__):
                assert name in listed, name
    for m in MINE:
        assert os.path.isfile(os.path.join(ROOT, m)), m


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
