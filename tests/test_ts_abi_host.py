"""The transport stream and ADTS ABI without a device: the size of every struct of include/ohgpu_ts.h and the offset of every field, from a
compiled offsetof program that includes ohgpu.h alone, against ohpipeline_amd.capi's dtypes; the constants; the symbols; the checks'
codes and texts."""
import os
import re
import subprocess

import numpy as np
import pytest

from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {
    "ohgpu_ts_stream_desc": (capi.TS_STREAM_DESC, 64),
    "ohgpu_ts_stream_result": (capi.TS_STREAM_RESULT, 64),
    "ohgpu_ts_pes": (capi.TS_PES, 32),
    "ohgpu_adts_stream_desc": (capi.ADTS_STREAM_DESC, 32),
    "ohgpu_adts_stream_result": (capi.ADTS_STREAM_RESULT, 64),
    "ohgpu_adts_frame": (capi.ADTS_FRAME, 32),
}
NAMES = ("TS_PACKET_BYTES", "TS_NONE", "TS_OK", "TS_NO_PAT", "TS_NO_PMT", "TS_NO_AUDIO", "TS_CORRUPT", "TS_PES_OPEN", "TS_PES_CONTINUATION", "TS_PES_EXCESS",
         "TS_PES_TRUNCATED", "TS_PES_CC_JUMP", "ADTS_OK", "ADTS_NOT_ADTS", "ADTS_RECOGNISE", "ADTS_INTERRUPTED", "ADTS_RECOGNISE_LAST_START", "ADTS_RECOGNISE_FRAMES")
CONSTANTS = {"OHGPU_" + k: getattr(capi, k) for k in NAMES}


def test_struct_sizes_and_every_field_offset_match_the_header(tmp_path):
    items = [(name, None, "sizeof(%s)" % name) for name in STRUCTS]
    for name, (dtype, _) in STRUCTS.items():
        items += [(name, field, "offsetof(%s, %s)" % (name, field)) for field in dtype.names]
    items += [(None, c, "(size_t)%s" % c) for c in CONSTANTS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\nint main(){\n' +        # (ohgpu.h brings the header along)
                   "".join('printf("%%zu\\n", %s);\n' % expr for _, _, expr in items) +
                   'printf("%d\\n", OHGPU_TS_NO_PTS == 0xffffffffffffffffull && OHGPU_ABI_VERSION == 1);\nreturn 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert len(out) == len(items) + 1 and out[-1] == 1 and capi.TS_NO_PTS == 0xFFFFFFFFFFFFFFFF
    for (name, field, expr), got in zip(items, out):
        if name is None:
            assert got == CONSTANTS[field], expr
        elif field is None:
            assert got == STRUCTS[name][0].itemsize == STRUCTS[name][1], expr
        else:
            assert got == STRUCTS[name][0].fields[field][1], expr
    for name, (dtype, size) in STRUCTS.items():              # every byte of every struct is a named field
        assert sum(dtype.fields[f][0].itemsize for f in dtype.names) == size, name


def test_the_header_stands_alone_and_every_symbol_is_declared_bound_and_exported(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "ohgpu_ts.h"\nint main(void){ return sizeof(ohgpu_ts_pes) == 32 && sizeof(ohgpu_adts_frame) == 32 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone")])
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ohgpu_ts.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ohgpu_(?:ts|adts|id3v2)_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.TS_SYMBOLS) and len(declared) == 20
    for name in declared:
        assert hasattr(capi.lib(), name), name
    for name in ("ohgpu_ts_batch_check", "ohgpu_ts_batch_create", "ohgpu_ts_batch_run", "ohgpu_ts_batch_results", "ohgpu_ts_batch_pes", "ohgpu_ts_batch_phase_ms",
                 "ohgpu_ts_process_host", "ohgpu_ts_crc", "ohgpu_adts_batch_check", "ohgpu_adts_batch_create", "ohgpu_adts_batch_run", "ohgpu_adts_batch_results",
                 "ohgpu_adts_batch_frames", "ohgpu_adts_batch_phase_ms", "ohgpu_adts_process_host", "ohgpu_adts_header", "ohgpu_id3v2_skip", "ohgpu_ts_adts_process_host"):
        assert name in declared, name
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ohgpu.h")).read(), flags=re.S)
    assert '#include "ohgpu_ts.h"' in main and "ohgpu_ts_batch_create" not in main
    assert capi.lib().ohgpu_abi_version() == 1
    from ohpipeline_amd import build
    assert os.path.join(ROOT, "include", "ohgpu_ts.h") in build.HEADERS


def test_the_checks_run_without_a_device_and_name_what_they_refuse():
    d = np.zeros(2, dtype=capi.TS_STREAM_DESC)
    d["src_offset"], d["src_bytes"], d["dst_offset"], d["dst_capacity"] = (0, 400), (376 + 5, 188), (0, 400), (368, 184)
    d["pes_first"], d["pes_capacity"] = (0, 3), (3, 2)
    capi.ts_batch_check(d, 5, 588, 584)
    for change, code, text in ((lambda: d["dst_capacity"].__setitem__(0, 367), capi.ERR_BOUNDS, "2 packets can deliver 368 bytes"),
                               (lambda: d["flags"].__setitem__(1, 4), capi.ERR_INVALID, "unknown flags 0x4"),
                               (lambda: d["audio_pid"].__setitem__(1, 0x2000), capi.ERR_INVALID, "a PID has 13 bits"),
                               (lambda: d["pes_first"].__setitem__(1, 2), capi.ERR_INVALID, "the PES ranges [0, +3) and [2, +2) overlap"),
                               (lambda: d["pes_capacity"].__setitem__(1, 3), capi.ERR_INVALID, "PES records [3, +3) of a table of 5"),
                               (lambda: d["src_bytes"].__setitem__(1, 189), capi.ERR_BOUNDS, "beyond the 588-byte source arena"),
                               (lambda: d["reserved"].__setitem__(0, (0, 0, 1)), capi.ERR_INVALID, "reserved words must be zero")):
        keep = d.copy()
        change()
        with pytest.raises(capi.OhGpuError) as e:
            capi.ts_batch_check(d, 5, 588, 584)
        assert e.value.code == code and text in str(e.value), str(e.value)
        d[:] = keep
    a = np.zeros(1, dtype=capi.ADTS_STREAM_DESC)
    a["src_offset"], a["src_bytes"], a["frame_capacity"] = 10, 90, 4
    capi.adts_batch_check(a, 4, 100)
    for change, code, text in ((lambda: a["src_bytes"].__setitem__(0, 91), capi.ERR_BOUNDS, "beyond the 100-byte source arena"),
                               (lambda: a["frame_capacity"].__setitem__(0, 5), capi.ERR_INVALID, "frames [0, +5) of a table of 4"),
                               (lambda: a["flags"].__setitem__(0, 3), capi.ERR_INVALID, "unknown flags 0x3")):
        keep = a.copy()
        change()
        with pytest.raises(capi.OhGpuError) as e:
            capi.adts_batch_check(a, 4, 100)
        assert e.value.code == code and text in str(e.value), str(e.value)
        a[:] = keep
