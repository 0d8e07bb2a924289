"""The chained-stream files against the reference files whose behaviour they answer to, the way
tests/test_vorbis_is_not_a_transliteration.py holds the Vorbis decoder: normalised line overlap (tools/overlap.py) must stay below
20 %.  The new files answer to OpenHome/Media/Codec/Vorbis.cpp, to the .c files of the reference's Tremor -- vorbisfile.c, which
follows a chain, above all -- and to its libogg, none of whose text may be restated.  (They keep "vorbis" out of their names: the
Vorbis test's list of files is closed.)  Runs where the reference tree exists, skipped elsewhere."""
import glob
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "thirdparty", "Tremor", "vorbisfile.c")), reason="the reference tree only exists in the build container")

MINE = ["tests/ogg_links_textbook.py", "tests/ogg_links_cases.py", "tests/cpp/ogg_links_driver.cpp", "tests/test_ogg_links_textbook.py", "tests/test_ogg_links_core_cpu.py",
        "tests/test_gpu_ogg_links.py", "tests/chained_cases.py", "tests/test_chained_fixtures.py", "tests/test_chained_tremor.py", "tests/test_gpu_chained_to_pcm.py",
        "tests/cpp/tremor_chain_driver.c", "tests/golden/make_chained_fixtures.py", "ohpipeline_amd/csrc/ogg_page_core.h", "ohpipeline_amd/csrc/api_ogg.hip",
        "ohpipeline_amd/csrc/api_vorbis.hip", "include/ohgpu_vorbis.h", "tools/bench_ogg.py", "tests/cpp/test_chained_decoder.cpp", "tests/test_chained_host_cpp.py",
        "ohpipeline_amd/host/VorbisDecoder.h", "ohpipeline_amd/host/VorbisDecoder.cpp"]
NAME = re.compile(r"chain|links", re.I)


def theirs():
    return [os.path.join(REF, "OpenHome", "Media", "Codec", "Vorbis.cpp")] + sorted(glob.glob(os.path.join(REF, "thirdparty", "Tremor", "*.c"))) + \
        sorted(glob.glob(os.path.join(REF, "thirdparty", "libogg", "src", "*.c")))


def test_the_files_are_there():
    listed = {os.path.basename(m) for m in MINE}
    for folder in ("include", "ohpipeline_amd/csrc", "ohpipeline_amd/host", "tests", "tests/cpp", "tests/golden", "tools"):      # a later file of this family is listed too
        for name in os.listdir(os.path.join(ROOT, folder)):
            if NAME.search(name) and name.endswith((".h", ".hip", ".cpp", ".c", ".py")) and name != os.path.basename(__file__):
                assert name in listed, name
    for m in MINE:
        assert os.path.isfile(os.path.join(ROOT, m)), m
    assert any(t.endswith("vorbisfile.c") for t in theirs()) and any(t.endswith("framing.c") for t in theirs())


@pytest.mark.parametrize("mine", MINE)
def test_overlap_with_the_reference_stays_low(mine):
    import overlap
    own = overlap.significant(os.path.join(ROOT, mine))
    ref = set()
    for name in theirs():
        ref.update(overlap.significant(name))
    share = sum(1 for l in own if l in ref) / max(1, len(own))
    assert share < 0.20, f"{mine}: {100 * share:.1f} % of its significant lines are in the reference's Vorbis.cpp, Tremor and libogg"
