"""The RAOP receiver's ABI without a device: the size of every struct of include/ohgpu_raop_rx.h and the offset of every field, from a
compiled offsetof program that includes ohgpu.h alone, against ohpipeline_amd.capi's dtypes; the constants; the symbols; the check's
codes and texts."""
import os
import re
import subprocess

import numpy as np
import pytest

from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {
    "ohgpu_raop_rx_datagram": (capi.RAOP_RX_DATAGRAM, 16, {}),
    "ohgpu_raop_rx_stream": (capi.RAOP_RX_STREAM, 48, {"state_reserved": "state_in.reserved", **{k: "state_in." + k for k in capi.RAOP_RX_STATE_FIELDS}}),
    "ohgpu_raop_rx_record": (capi.RAOP_RX_RECORD, 48, {}),
    "ohgpu_raop_rx_stream_result": (capi.RAOP_RX_STREAM_RESULT, 296, {"state_reserved": "state_out.reserved", **{k: "state_out." + k for k in capi.RAOP_RX_STATE_FIELDS}}),
}
NAMES = ("MAX_PACKET_BYTES", "MAX_FRAMES", "MAX_RANGES", "PORT_AUDIO", "PORT_CONTROL", "OK", "TRUNCATED", "OVERSIZE", "OTHER_TYPE", "OUTPUT", "DUPLICATE", "PENDING",
         "DROPPED_BY_RESET", "FLUSHED", "WRONG_SESSION", "SYNC", "IGNORED", "NOT_REACHED", "EVENT_NEW_STREAM", "EVENT_DELAY", "STOP_NONE", "STOP_BUFFER_FULL", "STOP_RESTARTED")
CONSTANTS = {"OHGPU_RAOP_RX_" + k: getattr(capi, "RAOP_RX_" + k) for k in NAMES}


def test_struct_sizes_and_every_field_offset_match_the_header(tmp_path):
    items = [(name, None, "sizeof(%s)" % name) for name in STRUCTS]
    for name, (dtype, _, renamed) in STRUCTS.items():
        items += [(name, field, "offsetof(%s, %s)" % (name, renamed.get(field, field))) for field in dtype.names]
    items += [(None, c, "(size_t)%s" % c) for c in CONSTANTS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\nint main(){\n' +        # (ohgpu.h brings the header along)
                   "".join('printf("%%zu\\n", %s);\n' % expr for _, _, expr in items) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert len(out) == len(items)
    for (name, field, expr), got in zip(items, out):
        if name is None:
            assert got == CONSTANTS[field], expr
        elif field is None:
            assert got == STRUCTS[name][0].itemsize == STRUCTS[name][1], expr
        else:
            assert got == STRUCTS[name][0].fields[field][1], expr
    for name, (dtype, size, _) in STRUCTS.items():           # every byte of every struct is a named field
        assert sum(dtype.fields[f][0].itemsize for f in dtype.names) == size, name


def test_the_header_stands_alone_and_every_symbol_is_declared_bound_and_exported(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include "ohgpu_raop_rx.h"\nint main(void){ return sizeof(ohgpu_raop_rx_record) == 48 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "alone")])
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ohgpu_raop_rx.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ohgpu_raop_rx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.RAOP_RX_SYMBOLS) and len(declared) == 8
    for name in declared:
        assert hasattr(capi.lib(), name), name
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ohgpu.h")).read(), flags=re.S)
    assert '#include "ohgpu_raop_rx.h"' in main and "ohgpu_raop_rx_batch_create" not in main
    from ohpipeline_amd import build
    assert os.path.join(ROOT, "include", "ohgpu_raop_rx.h") in build.HEADERS


def test_the_check_runs_without_a_device_and_names_what_it_refuses():
    s, g = np.zeros(1, dtype=capi.RAOP_RX_STREAM), np.zeros(2, dtype=capi.RAOP_RX_DATAGRAM)
    s["n_datagrams"], s["max_frames"] = 2, 50
    g["src_offset"], g["bytes"], g["port"] = (0, 100), (100, 108), (0, 1)
    capi.raop_rx_batch_check(s, g, 208)
    for change, code, text in ((lambda: g["src_offset"].__setitem__(1, 98), capi.ERR_INVALID, "no multiple of 4"),
                               (lambda: g["port"].__setitem__(0, 2), capi.ERR_INVALID, "neither audio nor control"),
                               (lambda: s["max_frames"].__setitem__(0, 64), capi.ERR_INVALID, "outside 1..63"),
                               (lambda: g["bytes"].__setitem__(1, 109), capi.ERR_BOUNDS, "beyond the 208-byte source arena"),
                               (lambda: s["n_datagrams"].__setitem__(0, 1), capi.ERR_INVALID, "take 1 datagrams of a table of 2")):
        keep = s.copy(), g.copy()
        change()
        with pytest.raises(capi.OhGpuError) as e:
            capi.raop_rx_batch_check(s, g, 208)
        assert e.value.code == code and text in str(e.value), str(e.value)
        s[:], g[:] = keep
