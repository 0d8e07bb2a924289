"""The RAOP receiver's counterpart of tests/far_cases.py's tables, for the family whose ABI text is include/ohgpu_raop_rx.h: which table
fields are arena offsets, the alignment its header text asks of them, and its result structs' 64-bit fields (it has none: the packet
rows it hands over are ohgpu.h's ohgpu_alac_packet, whose src_offset moves with the source).  tests/test_far_raop_rx_cases.py holds them
to that header without a device; tests/test_gpu_raop_rx_far_offsets.py runs the family past 2^31 and 2^32.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

RELOCATE = {"raop_rx": {"datagrams": (("src_offset",), ())}}
ALIGN = {"raop_rx": (4, 1)}
RESULTS = {"ohgpu_raop_rx_record": {}, "ohgpu_raop_rx_stream_result": {}}


def relocate(family, tables, src_shift, dst_shift):
    """tests/far_cases.py's relocate() over this file's RELOCATE"""
    out = {}
    for name, (src_fields, dst_fields) in RELOCATE[family].items():
        t = tables[name].copy()
        for f in src_fields:
            t[f] += np.uint64(src_shift)
        for f in dst_fields:
            t[f] += np.uint64(dst_shift)
        out[name] = t
    return out
