"""The protected MPEG-4 family's counterpart of tests/far_cases.py's tables, for the family whose ABI text is include/ohgpu_cenc.h: which
descriptor fields are arena offsets, the alignment its header text asks of them, and its result struct's 64-bit fields.
tests/test_far_cenc_cases.py holds them to that header without a device; tests/test_gpu_cenc_far_offsets.py runs the family past 2^31
and 2^32.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

RELOCATE = {"cenc": {"descs": (("src_offset",), ("dst_offset",))}}
ALIGN = {"cenc": (1, 1)}
# (ohgpu_cenc_stream_result begins with an ohgpu_mp4f_stream_result, whose fields tests/far_cases.py classifies under that name)
RESULTS = {"ohgpu_cenc_stream_result": {"same": ("blocks",)}}


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
