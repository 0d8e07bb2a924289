"""The Songcast receiver's ABI without a device: the size of every new struct of include/ohgpu.h and the offset of every field, from
a compiled offsetof program, against ohpipeline_amd.capi's dtypes; the constants; the new symbols."""
import os
import re
import subprocess

from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {
    "ohgpu_ohm_rx_datagram": (capi.OHM_RX_DATAGRAM, 16, {}),
    "ohgpu_ohm_rx_stream": (capi.OHM_RX_STREAM, 64, {"state_reserved": "state_in.reserved", **{k: "state_in." + k for k in capi.OHM_RX_STATE_FIELDS}}),
    "ohgpu_ohm_rx_record": (capi.OHM_RX_RECORD, 104, {}),
    "ohgpu_ohm_rx_stream_result": (capi.OHM_RX_STREAM_RESULT, 136, {"state_reserved": "state_out.reserved", **{k: "state_out." + k for k in capi.OHM_RX_STATE_FIELDS}}),
}
CONSTANTS = {
    "OHGPU_OHM_RX_OK": capi.OHM_RX_OK, "OHGPU_OHM_RX_NOT_OHM": capi.OHM_RX_NOT_OHM, "OHGPU_OHM_RX_NOT_AUDIO": capi.OHM_RX_NOT_AUDIO,
    "OHGPU_OHM_RX_TRUNCATED": capi.OHM_RX_TRUNCATED, "OHGPU_OHM_RX_BAD_HEADER": capi.OHM_RX_BAD_HEADER, "OHGPU_OHM_RX_OVERSIZE": capi.OHM_RX_OVERSIZE,
    "OHGPU_OHM_RX_OUTPUT": capi.OHM_RX_OUTPUT, "OHGPU_OHM_RX_DUPLICATE": capi.OHM_RX_DUPLICATE, "OHGPU_OHM_RX_PENDING": capi.OHM_RX_PENDING,
    "OHGPU_OHM_RX_DROPPED_BY_RESET": capi.OHM_RX_DROPPED_BY_RESET, "OHGPU_OHM_RX_STALE": capi.OHM_RX_STALE, "OHGPU_OHM_RX_NOT_REACHED": capi.OHM_RX_NOT_REACHED,
    "OHGPU_OHM_RX_IGNORED": capi.OHM_RX_IGNORED, "OHGPU_OHM_RX_EVENT_NEW_STREAM": capi.OHM_RX_EVENT_NEW_STREAM, "OHGPU_OHM_RX_EVENT_DELAY": capi.OHM_RX_EVENT_DELAY,
    "OHGPU_OHM_RX_EVENT_HALT": capi.OHM_RX_EVENT_HALT, "OHGPU_OHM_RX_STOP_NONE": capi.OHM_RX_STOP_NONE, "OHGPU_OHM_RX_STOP_STALE": capi.OHM_RX_STOP_STALE,
    "OHGPU_OHM_RX_STOP_HALT": capi.OHM_RX_STOP_HALT, "OHGPU_OHM_RX_MAX_RESEND": 20,
}


def test_struct_sizes_and_every_field_offset_match_the_header(tmp_path):
    items = [(name, None, "sizeof(%s)" % name) for name in STRUCTS]
    for name, (dtype, _, renamed) in STRUCTS.items():
        items += [(name, field, "offsetof(%s, %s)" % (name, renamed.get(field, field))) for field in dtype.names]
    items += [(None, c, "(size_t)%s" % c) for c in CONSTANTS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\nint main(){\n' +
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
    # every byte of every struct is a named field: nothing the device writes is lost between the fields
    for name, (dtype, size, _) in STRUCTS.items():
        assert sum(dtype.fields[f][0].itemsize for f in dtype.names) == size, name


def test_every_new_symbol_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ohgpu.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ohgpu_ohm_rx_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["ohgpu_ohm_rx_batch_check", "ohgpu_ohm_rx_batch_create", "ohgpu_ohm_rx_batch_phase_ms", "ohgpu_ohm_rx_batch_results",
                        "ohgpu_ohm_rx_batch_run", "ohgpu_ohm_rx_process_host"]
    for name in declared:
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name


def test_the_check_runs_without_a_device_and_names_what_it_refuses():
    import numpy as np
    import pytest
    s, g = np.zeros(1, dtype=capi.OHM_RX_STREAM), np.zeros(2, dtype=capi.OHM_RX_DATAGRAM)
    s["n_datagrams"], s["dst_capacity"] = 2, 100
    g["src_offset"], g["bytes"] = (0, 100), (100, 108)
    capi.ohm_rx_batch_check(s, g, 208, 100)
    for change, code, text in ((lambda: g["src_offset"].__setitem__(1, 98), capi.ERR_INVALID, "no multiple of 4"),
                               (lambda: s["dst_capacity"].__setitem__(0, 91), capi.ERR_BOUNDS, "may carry 92 audio bytes"),
                               (lambda: s["n_datagrams"].__setitem__(0, 1), capi.ERR_INVALID, "take 1 datagrams of a table of 2")):
        keep = s.copy(), g.copy()
        change()
        with pytest.raises(capi.OhGpuError) as e:
            capi.ohm_rx_batch_check(s, g, 208, 100)
        assert e.value.code == code and text in str(e.value), str(e.value)
        s[:], g[:] = keep
