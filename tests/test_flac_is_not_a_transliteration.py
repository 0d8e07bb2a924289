"""The FLAC decoder's files against the reference files whose behaviour they answer to, the way
tests/test_host_is_not_a_transliteration.py holds the host adapter: normalised line overlap (tools/overlap.py) must stay below
20 %.  host/FlacDecoder.cpp answers to Codec/Flac.cpp; the format core, the kernels and the tests' model and writer answer to the
reference's vendored libFLAC, none of whose text may be restated.  Runs where the reference tree exists, skipped elsewhere."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "OpenHome")), reason="the reference tree only exists in the build container")

LIBFLAC = "thirdparty/flac-1.2.1/src/libFLAC"
CASES = [
    ("ohpipeline_amd/host/FlacDecoder.cpp", ["OpenHome/Media/Codec/Flac.cpp"]),
    ("ohpipeline_amd/host/FlacDecoder.h", ["OpenHome/Media/Codec/Flac.cpp"]),
    ("ohpipeline_amd/csrc/flac_frame_core.h", [LIBFLAC + "/*.c", LIBFLAC + "/include/private/*.h"]),
    ("ohpipeline_amd/csrc/flac_frame_kernel.hip", [LIBFLAC + "/*.c"]),
    ("tests/cpp/flac_core_driver.cpp", [LIBFLAC + "/*.c"]),
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
