"""CPU-side checks of the C ABI: the library loads, exports exactly what include/ohgpu.h declares,
its struct layouts match the header, and the host-side tables (ramp multipliers, resampler design)
agree with the golden data / the oracle.  No compute call is made (there is no GPU here)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ohgpu.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ohgpu_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = capi.lib()
    names = declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/ohgpu.h but not exported by libohgpu.so"
    assert sorted(capi.SYMBOLS) == names, "capi.SYMBOLS and include/ohgpu.h disagree"
    assert L.ohgpu_abi_version() == 1


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\n#include "ohp_pipeline.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ohgpu_msg_desc), sizeof(ohgpu_src_msg_desc),'
                   'sizeof(ohp_msg_desc), sizeof(ohp_src_msg_desc), offsetof(ohgpu_msg_desc, flags),'
                   'offsetof(ohgpu_src_msg_desc, n_frames), offsetof(ohgpu_src_msg_desc, flags));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"),
                           str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == out[2] == capi.MSG_DESC.itemsize == O.MSG_DESC.itemsize == 32
    assert out[1] == out[3] == capi.SRC_MSG_DESC.itemsize == O.SRC_MSG_DESC.itemsize == 64
    assert out[4] == capi.MSG_DESC.fields["flags"][1] == 31
    assert out[5] == capi.SRC_MSG_DESC.fields["n_frames"][1] == 40
    assert out[6] == capi.SRC_MSG_DESC.fields["flags"][1] == 55


def test_songcast_struct_layouts_match_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ohgpu_ohm_stream), sizeof(ohgpu_ohm_fragment),'
                   'sizeof(ohgpu_ohm_frame_desc), offsetof(ohgpu_ohm_stream, codec), offsetof(ohgpu_ohm_fragment, flags),'
                   'offsetof(ohgpu_ohm_frame_desc, first_fragment), offsetof(ohgpu_ohm_frame_desc, flags),'
                   'sizeof(ohgpu_flywheel_desc));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out[0] == capi.OHM_STREAM.itemsize == 64
    assert out[1] == capi.OHM_FRAGMENT.itemsize == 24
    assert out[2] == capi.OHM_FRAME_DESC.itemsize == 48
    assert out[3] == capi.OHM_STREAM.fields["codec"][1] == 21
    assert out[4] == capi.OHM_FRAGMENT.fields["flags"][1] == 18
    assert out[5] == capi.OHM_FRAME_DESC.fields["first_fragment"][1] == 36
    assert out[6] == capi.OHM_FRAME_DESC.fields["flags"][1] == 42
    assert out[7] == capi.FLYWHEEL_DESC.itemsize == 48


def test_batch_paths_query_is_exported_and_laid_out_as_the_header_says(tmp_path):
    """ohgpu_batch_paths_info: the read-only call that tells a test which kernel path a pcm / Songcast / fmt batch was planned onto."""
    assert "ohgpu_batch_paths_info" in capi.SYMBOLS and hasattr(capi.lib(), "ohgpu_batch_paths_info")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(ohgpu_batch_paths), offsetof(ohgpu_batch_paths, launches),'
                   'offsetof(ohgpu_batch_paths, heavy_chunks), offsetof(ohgpu_batch_paths, ohm_headers_separate),'
                   'offsetof(ohgpu_batch_paths, reserved));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    f = capi.BATCH_PATHS.fields
    assert out == [capi.BATCH_PATHS.itemsize, f["launches"][1], f["heavy_chunks"][1], f["ohm_headers_separate"][1], f["reserved"][1]]
    assert out[0] == 64
    # the fmt routes' fields came out of `reserved`: the older fields stay where they were, the struct stays 64 bytes
    assert (f["launches"][1], f["heavy_chunks"][1], f["ohm_headers_separate"][1]) == (4, 16, 36)
    names = ("fmt_wide_records", "fmt_stereo_records", "fmt_stereo_kind", "fmt_stereo_bytes", "fmt_staged_chunks", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ohgpu.h"\nint main(){printf("' + "%zu " * len(names) + '\\n", '
                   + ", ".join(f"offsetof(ohgpu_batch_paths, {n})" for n in names) + ");return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert out == [f[n][1] for n in names] == [40, 44, 48, 52, 56, 60]
    assert capi.lib().ohgpu_batch_paths_info(None, None) == capi.ERR_INVALID      # (no context, no device: a null batch is refused)


def test_ramp_table_equals_reference_data():
    """The table the DEVICE uses (generated in host_design.cpp) equals RampArray.h:7-74 entry for entry."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "ramp_table_q15.json")))["values"]
    assert capi.ramp_table().tolist() == golden


@pytest.mark.parametrize("rin,rout,T", [(44100, 48000, 32), (96000, 48000, 64), (88200, 48000, 24), (48000, 44100, 32),
                                        (32000, 48000, 16), (192000, 48000, 96)])
def test_src_design_equals_oracle(rin, rout, T):
    """Product-side filter design (C++) and the oracle's (C) produce the same Q28 table."""
    L_, M_, coef = capi.src_design(rin, rout, T, 9.0, 20000.0)
    ref = O.Src(rin, rout, T, 9.0, 20000.0)
    assert (L_, M_) == (ref.L, ref.M)
    assert np.array_equal(coef, ref.coef_q28)
    assert ref.sum_abs_max < (1 << 30)
    for n in (0, 1, 146, 147, 148, 220, 441000):
        assert capi.lib().ohgpu_src_out_frames(L_, M_, n) == ref.out_frames(n)


def test_init_without_gpu_fails_loudly():
    L = capi.lib()
    n = L.ohgpu_device_count()
    if n > 0:
        pytest.skip("a GPU is visible; the no-device path cannot be exercised")
    h = C.c_void_p()
    assert L.ohgpu_init(0, C.byref(h)) == capi.ERR_NO_DEVICE
    assert b"no CPU fallback" in L.ohgpu_last_error()
    with pytest.raises(capi.OhGpuError):
        capi.Context(0)


def test_product_never_touches_the_oracle():
    """The product path may not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "ohpipeline_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".hpp")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                code = re.sub(r"//.*|/\*.*?\*/|#.*|\"\"\".*?\"\"\"", "", text, flags=re.S)
                assert "ohp_" not in code and "oracle_lib" not in code, f"{f} references the oracle"
    needed = subprocess.check_output(["readelf", "-d", capi.LIB_PATH]).decode()
    assert "ohp_oracle" not in needed


def test_the_shipped_library_is_not_a_diagnostic_build():
    """The kernels have no compile-time ablation switches, tunables, phase stamps or environment hooks: no preprocessor
    conditional under csrc/ names one of their families, no source calls getenv, and the shipped object carries no hook names in its
    data and no getenv among its imports."""
    from ohpipeline_amd import build as product_build
    lib_path = product_build.LIB_PATH
    blob = open(lib_path, "rb").read()
    for needle in (b"OHGPU_DIAG", b"OHGPU_EXP", b"STAMP_FILE"):
        assert needle not in blob, needle
    imports = subprocess.run(["nm", "-D", "--undefined-only", lib_path], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in imports
    assert "OHGPU_DIAG" not in " ".join(sum(product_build.SOURCE_FLAGS.values(), []))
    csrc = os.path.join(ROOT, "ohpipeline_amd", "csrc")
    switch = re.compile(r"MF_|OHGPU_DIAG|OHGPU_LEGACY|OHGPU_PLAN_TIMING|OHGPU_EXP|OHGPU_WG_ROWS|OHGPU_LINE_\w*GROUPS_PER_CU|OHGPU_LEAN_")
    for name in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, name), errors="replace").read()
        assert "getenv" not in text, f"{name}: getenv"
        for no, line in enumerate(text.splitlines(), 1):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                assert not switch.search(line), f"{name}:{no}: a compile-time switch: {line.strip()}"


# ---- the signatures: every prototype of the six public headers against its symbol table's entry, class by class
_INT64, _INT32 = {"uint64_t", "int64_t", "size_t"}, {"int", "unsigned", "uint32_t", "int32_t"}


def _c_class(decl, named):
    """The class of a C parameter (`named`: the last word is its name) or return type: ptr, i64, i32, f64, f32."""
    if "*" in decl or "[" in decl:
        return "ptr"
    words = [w for w in decl.split() if w not in ("const", "struct")]
    if named and len(words) > 1:
        words = words[:-1]
    assert len(words) == 1, f"cannot classify {decl!r}"
    w = words[0]
    if w in ("double", "float"):
        return {"double": "f64", "float": "f32"}[w]
    assert w in _INT64 | _INT32, f"cannot classify {decl!r}"
    return "i64" if w in _INT64 else "i32"


def header_prototypes(header):
    """{name: (return class, [argument classes])} of every ohgpu_* function a header under include/ declares."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)            # preprocessor lines, continued ones too
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    while True:                                                                      # struct, union and enum bodies, innermost first
        text, n = re.subn(r"\{[^{}]*\}", " ", text)
        if not n:
            break
    out = {}
    for stmt in text.split(";"):                                                     # a prototype runs to its `;`, across lines
        m = re.fullmatch(r"[\s}]*(?!typedef\b)([\w\s\*]+?)\b(ohgpu_[a-z0-9_]+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m:
            assert "(" not in stmt, f"{header}: a statement with a parenthesis that is no ohgpu_* prototype: {stmt.strip()!r}"
            continue
        ret, name, params = m.groups()
        assert "(" not in params and name not in out, f"{header}: {name}"
        params = [p.strip() for p in params.split(",")] if params.strip() not in ("", "void") else []
        out[name] = (_c_class(ret, named=False), [_c_class(p, named=True) for p in params])
    return out


def _ctypes_class(t):
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    if t in (C.c_double, C.c_float):
        return "f64" if t is C.c_double else "f32"
    assert t in (C.c_uint64, C.c_int64, C.c_size_t, C.c_int, C.c_uint32, C.c_int32), f"cannot classify {t!r}"
    return {8: "i64", 4: "i32"}[C.sizeof(t)]


def test_symbol_tables_match_the_headers_prototypes_argument_by_argument():
    """Return class, argument count and each argument's class (pointer, 64-bit integer, 32-bit integer, double, float) of every
    ohgpu_* prototype in the six headers against the entry of that header's table; each table holds exactly its header's functions."""
    from ohpipeline_amd import build as product_build
    public = sorted(os.path.basename(h) for h in product_build.HEADERS if os.path.dirname(h) == os.path.join(ROOT, "include"))
    assert public == sorted(os.listdir(os.path.join(ROOT, "include")))
    ABI_TABLES = capi.ABI_TABLES                                                     # the registry lib() binds: header file name -> table
    assert sorted(ABI_TABLES) == public, "capi.ABI_TABLES must list exactly the headers the build lists under include/"
    tables = (capi.SYMBOLS, capi.CENC_SYMBOLS, capi.CBCS_SYMBOLS, capi.RAOP_RX_SYMBOLS, capi.TS_SYMBOLS, capi.VORBIS_SYMBOLS)
    assert sorted(map(id, ABI_TABLES.values())) == sorted(map(id, tables))
    protos = {h: header_prototypes(h) for h in public}
    assert {h: len(p) for h, p in protos.items()} == {"ohgpu.h": 158, "ohgpu_cenc.h": 13, "ohgpu_cbcs.h": 13, "ohgpu_raop_rx.h": 8,
                                                      "ohgpu_ts.h": 20, "ohgpu_vorbis.h": 13}
    found = [n for p in protos.values() for n in p]
    entries = [n for t in ABI_TABLES.values() for n in t]
    assert len(found) == len(set(found)) == 225 and len(entries) == len(set(entries))
    assert set(entries) == set(found)
    for h, table in ABI_TABLES.items():
        assert set(table) == set(protos[h]), f"{h}: its table and its prototypes disagree"
        for name, (res, args) in table.items():
            want = protos[h][name]
            got = (_ctypes_class(res), [_ctypes_class(a) for a in args])
            assert len(got[1]) == len(want[1]), f"{name}: {len(got[1])} argtypes, the header has {len(want[1])} parameters"
            assert got == want, f"{name}: capi has {got}, {h} declares {want}"
            fn = getattr(capi.lib(), name)                                           # ... and lib() bound what the registry lists
            assert fn.restype is res and list(fn.argtypes) == list(args), f"{name}: not bound as its table says"
