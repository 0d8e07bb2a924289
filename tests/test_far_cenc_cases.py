"""tests/far_cenc_cases.py checked without a device, the way tests/test_far_cases.py checks tests/far_cases.py: every
ohgpu_*_batch_create of include/ohgpu_cenc.h has a relocator, an alignment and a far test of its name; relocate changes the listed
fields alone; every 64-bit field of the header's result structs is classified."""
import os
import re

import numpy as np

import far_cenc_cases as FARC
from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ohgpu_cenc.h")).read()


def test_every_batch_family_of_the_header_has_a_relocator_and_a_far_test():
    families = set(re.findall(r"\bint\s+ohgpu_(\w+?)_batch_create\s*\(", HEADER))
    assert families == {"cenc"} == set(FARC.RELOCATE) == set(FARC.ALIGN)
    text = open(os.path.join(ROOT, "tests", "test_gpu_cenc_far_offsets.py")).read()
    assert set(re.findall(r"^def test_(\w+)\(", text, re.M)) == families
    body = text[text.index("def test_cenc("):]
    assert '"cenc"' in body and "FAR.SPAN" in body and "FAR.Twin(" in body


def test_relocate_moves_the_listed_fields_and_nothing_else():
    dtype = capi.CENC_STREAM_DESC
    raw = np.random.default_rng(4).integers(0, 256, size=3 * dtype.itemsize, dtype=np.uint8)
    t = raw.view(dtype).copy()
    for f in ("src_offset", "dst_offset", "dst_capacity"):
        t[f] >>= np.uint64(24)
    src_shift, dst_shift = (1 << 32) + 48, (1 << 31) + 16
    moved = FARC.relocate("cenc", {"descs": t}, src_shift, dst_shift)["descs"]
    assert moved is not t and moved.dtype == t.dtype
    for f in dtype.names:
        shift = src_shift if f == "src_offset" else dst_shift if f == "dst_offset" else 0
        assert np.array_equal(moved[f], t[f] + np.uint64(shift) if shift else t[f]), f
    assert {f for f in dtype.names if f.endswith("_offset")} == {"src_offset", "dst_offset"}


def test_every_64_bit_field_of_the_result_structs_is_classified():
    for struct, lists in FARC.RESULTS.items():
        body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}\s*" + struct + ";", HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in re.findall(r"\bu?int64_t\s+([^;]+);", body):
            fields += [f.strip() for f in decl.split(",")]
        listed = [f for k in ("src", "dst", "same") for f in lists.get(k, ())]
        assert sorted(listed) == sorted(fields), (struct, sorted(fields))
    structs = set(re.findall(r"typedef struct (ohgpu_\w*(?:result|record|run|frame|sample|packet))\s*\{", HEADER))
    assert structs == set(FARC.RESULTS)
