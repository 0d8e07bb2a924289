"""The Apple Lossless decoder's files against the reference files whose behaviour they answer to, the way
tests/test_flac_is_not_a_transliteration.py holds the FLAC family: normalised line overlap (tools/overlap.py) must stay below 20 %.
host/AlacDecoder.* answers to Codec/AlacApple*.cpp; the format core, the kernels, the drivers and the tests' model and writer answer
to the reference's vendored Apple codec, none of whose text may be restated.  Runs where the reference tree exists, skipped
elsewhere."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "OpenHome")), reason="the reference tree only exists in the build container")

CODEC = ["thirdparty/apple_alac/codec/*.c", "thirdparty/apple_alac/codec/*.cpp", "thirdparty/apple_alac/codec/*.h"]
GLUE = ["OpenHome/Media/Codec/AlacApple*.cpp", "OpenHome/Media/Codec/AlacApple*.h"]
CASES = [
    ("ohpipeline_amd/csrc/alac_packet_core.h", CODEC),
    ("ohpipeline_amd/csrc/alac_packet_kernel.hip", CODEC),
    ("ohpipeline_amd/csrc/api_alac.hip", CODEC),
    ("tests/cpp/alac_core_driver.cpp", CODEC),
    ("tests/golden/alac_encode_driver.cpp", CODEC),
    ("tools/alac_core_cpu.cpp", CODEC),
    ("tests/alac_textbook.py", CODEC),
    ("tests/alac_frames.py", CODEC),
    ("ohpipeline_amd/host/AlacDecoder.cpp", GLUE),
    ("ohpipeline_amd/host/AlacDecoder.h", GLUE),
]


@pytest.mark.parametrize("mine,theirs", CASES, ids=[m for m, _ in CASES])
def test_overlap_with_the_reference_stays_low(mine, theirs):
    import overlap
    own = overlap.significant(os.path.join(ROOT, mine))
    ref = set()
    for pattern in theirs:
        files = glob.glob(os.path.join(REF, pattern))
        assert files, pattern
        for f in files:
            ref.update(overlap.significant(f))
    share = sum(1 for l in own if l in ref) / max(1, len(own))
    assert share < 0.20, f"{mine}: {100 * share:.1f} % of its significant lines are in {theirs}"
