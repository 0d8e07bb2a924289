"""tests/far_raop_rx_cases.py checked without a device, the way tests/test_far_cenc_cases.py checks tests/far_cenc_cases.py: every
ohgpu_*_batch_create of include/ohgpu_raop_rx.h has a relocator, an alignment and a far test of its name; relocate changes the listed
fields alone; every 64-bit field of the header's result structs is classified."""
import os
import re

import numpy as np

import far_raop_rx_cases as FARR
from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ohgpu_raop_rx.h")).read()


def test_every_batch_family_of_the_header_has_a_relocator_and_a_far_test():
    families = set(re.findall(r"\bint\s+ohgpu_(\w+?)_batch_create\s*\(", HEADER))
    assert families == {"raop_rx"} == set(FARR.RELOCATE) == set(FARR.ALIGN)
    text = open(os.path.join(ROOT, "tests", "test_gpu_raop_rx_far_offsets.py")).read()
    assert set(re.findall(r"^def test_(\w+)\(", text, re.M)) == families
    body = text[text.index("def test_raop_rx("):]
    assert '"raop_rx"' in body and "FAR.SPAN" in body and "FAR.Twin(" in body


def test_relocate_moves_the_listed_fields_and_nothing_else():
    dtype = capi.RAOP_RX_DATAGRAM
    raw = np.random.default_rng(4).integers(0, 256, size=3 * dtype.itemsize, dtype=np.uint8)
    t = raw.view(dtype).copy()
    t["src_offset"] >>= np.uint64(24)
    src_shift, dst_shift = (1 << 32) + 48, (1 << 31) + 16
    moved = FARR.relocate("raop_rx", {"datagrams": t}, src_shift, dst_shift)["datagrams"]
    assert moved is not t and moved.dtype == t.dtype
    for f in dtype.names:
        assert np.array_equal(moved[f], t[f] + np.uint64(src_shift) if f == "src_offset" else t[f]), f
    assert {f for d in (capi.RAOP_RX_DATAGRAM, capi.RAOP_RX_STREAM) for f in d.names if f.endswith("_offset")} == {"src_offset"}
    assert FARR.ALIGN["raop_rx"][0] == 4 and "a multiple of 4" in HEADER


def test_every_64_bit_field_of_the_result_structs_is_classified():
    for struct, lists in FARR.RESULTS.items():
        body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}\s*" + struct + ";", HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in re.findall(r"\bu?int64_t\s+([^;]+);", body):
            fields += [f.strip() for f in decl.split(",")]
        listed = [f for k in ("src", "dst", "same") for f in lists.get(k, ())]
        assert sorted(listed) == sorted(fields), (struct, sorted(fields))
    structs = set(re.findall(r"typedef struct (ohgpu_\w*(?:result|record|run|frame|sample|packet))\s*\{", HEADER))
    assert structs == set(FARR.RESULTS)
