"""tests/far_cases.py and the far-position builders, checked without a device: the models are invariant under the shifts the GPU tests
use; every placement, with all its aliases, lies inside the far blocks and off the other copy; a straddling placement holds its
boundary byte strictly inside; every ohgpu_*_batch_create of include/ohgpu.h has a relocator; and relocate changes the listed
fields alone."""
import os
import re

import numpy as np
import pytest

import dsd_pcm_cases as DC
import far_cases as FAR
import src_cases as SC
import src_pull_cases as PC
import src_textbook as TB
from ohpipeline_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ohgpu.h")).read()


# ---------------------------------------------------------------- model invariance
@pytest.mark.parametrize("f", [SC.F44, SC.F96, SC.F48], ids=["44to48", "96to48", "48to44"])
def test_src_model_is_the_same_near_and_far(f):
    """tests/src_cases.far_stream at every anchor: out_frame0 across 2^31 and 2^32, the input frame across 2^32, the ABI's limit."""
    rin, rout, T = f
    L, M, coef = capi.src_design(rin, rout, T, 9.0, 20000.0)
    table = capi.ramp_table()
    for label, anchor in SC.far_anchors(L, M).items():
        near, _ = SC.far_stream(L, M, T, SC.S24, anchor, False)
        far, _ = SC.far_stream(L, M, T, SC.S24, anchor, True)
        dn, df = near.descs(), far.descs()
        assert bytes(near.src) == bytes(far.src) and near.dst == far.dst
        moved = [k for k in dn.dtype.names if not np.array_equal(dn[k], df[k])]
        assert moved == ["src_frame0", "out_frame0"], (label, moved)
        k = (df["out_frame0"].astype(object) - dn["out_frame0"]) // L
        assert (k * L == df["out_frame0"].astype(object) - dn["out_frame0"]).all() and (k * M == df["src_frame0"].astype(object) - dn["src_frame0"]).all()
        assert int(df["out_frame0"].max()) <= SC.FAR_LIMIT and int(df["src_frame0"].max()) <= SC.FAR_LIMIT
        if label == "limit":
            assert SC.FAR_LIMIT in (int(df["out_frame0"][-1]), int(df["src_frame0"][0]))
        elif anchor[0] == "out":
            lo, hi = df["out_frame0"].astype(object), df["out_frame0"].astype(object) + df["n_frames"] - 1
            assert ((lo < anchor[1]) & (anchor[1] < hi)).sum() == 1
        want = TB.batch_bytes(coef, L, M, T, dn, near.arena(), near.dst, table, SC.FILL)
        assert (want != SC.FILL).sum() > 3 * 3000 and np.array_equal(TB.batch_bytes(coef, L, M, T, df, far.arena(), far.dst, table, SC.FILL), want), label


@pytest.mark.parametrize("T", [32, 64])
def test_src_pull_model_is_the_same_near_and_far(T):
    table = capi.src_pull_design(44100, 48000, T, PC.S, 8.0 if T == 32 else 9.0, 20000.0, 0.001)
    (near, _), (far, labels) = PC.far_streams(T, False), PC.far_streams(T, True)
    src, dn = near.arrays()
    src_far, df = far.arrays()
    assert np.array_equal(src, src_far) and near.dst_bytes == far.dst_bytes and len(labels) == len(df) == 2 * (4 * 4 + 1)
    assert [k for k in dn.dtype.names if not np.array_equal(dn[k], df[k])] == ["src_frame0", "pos_frame"]
    assert np.array_equal(df["pos_frame"] - dn["pos_frame"], df["src_frame0"] - dn["src_frame0"])
    first = df[[i for i, name in enumerate(labels) if name.endswith("m0")]]
    assert (first["pos_frac"] == PC.FAR_FRAC).all() and (first["pos_frac"].astype(object) + first["step"] >= 1 << 32).all()
    last = df["pos_frame"].astype(object) + ((df["pos_frac"].astype(object) + (df["n_frames"].astype(object) - 1) * df["step"]) >> 32)
    for boundary in (1 << 31, 1 << 32):
        assert ((df["pos_frame"] < boundary) & (last > boundary)).any(), boundary
    assert int(df["pos_frame"].max()) == 1 << 48
    ramp = capi.ramp_table()
    want = PC.expected(table, dn, src, near.dst_bytes, ramp)
    assert np.count_nonzero(want) > want.size // 2 and np.array_equal(PC.expected(table, df, src, far.dst_bytes, ramp), want)


@pytest.mark.parametrize("key", list(DC.DESIGNS), ids=[f"D{D}T{T}" for D, T in DC.DESIGNS])
def test_dsd_pcm_model_is_the_same_near_and_far(key):
    D, T = key
    near, far = DC.positions(key, False), DC.positions(key, True)
    assert np.array_equal(near.src, far.src) and near.dst_bytes == far.dst_bytes
    assert [k for k in near.descs.dtype.names if not np.array_equal(near.descs[k], far.descs[k])] == ["src_chunk0", "out_frame0"]
    shift = far.descs["out_frame0"].astype(object) - near.descs["out_frame0"]
    assert (shift % 2 == 0).all() and (shift * D == 16 * (far.descs["src_chunk0"].astype(object) - near.descs["src_chunk0"])).all()
    lo, hi = far.descs["out_frame0"].astype(object), far.descs["out_frame0"].astype(object) + far.descs["n_frames"] - 1
    for what, boundary in (("bit", (1 << 32) // D), ("byte", (1 << 35) // D), ("chunk", (1 << 36) // D), ("frame 2^31", 1 << 31), ("frame 2^32", 1 << 32)):
        assert ((lo < boundary) & (boundary < hi)).any(), what
    assert int(hi.max()) == 1 << 40 and sorted(hi)[-2] == (1 << 40) - 1
    assert capi.dsd_pcm_batch_check(D, T, far.descs, far.src.size, far.dst_bytes) is None
    over = far.descs.copy()
    over["out_frame0"][over["out_frame0"] == 1 << 40] += 1
    with pytest.raises(capi.OhGpuError):
        capi.dsd_pcm_batch_check(D, T, over, far.src.size, far.dst_bytes)
    assert (near.want() != DC.FILL).sum() > 6 * 2000 and np.array_equal(far.want(), near.want())


# ---------------------------------------------------------------- the arenas
SIZES = [(34, 34), (1000, 4097), (123457, 65536), (FAR.MAX_RANGE, FAR.MAX_RANGE)]


@pytest.mark.parametrize("family", sorted(FAR.RELOCATE))
@pytest.mark.parametrize("name", FAR.PAIRS)
def test_every_placement_and_its_aliases_lie_inside_the_blocks(family, name):
    src_align, dst_align = FAR.ALIGN[family]
    for n_src, n_dst in SIZES:
        far = FAR.pair(name, n_src, n_dst, src_align, dst_align)
        for side, (n, align) in enumerate(((n_src, src_align), (n_dst, dst_align))):
            near, at = FAR.near(align), far[side]
            assert near % align == 0 and at % align == 0 and at + n > 1 << 31
            windows = [(near - FAR.GUARD, n + 2 * FAR.GUARD), (at - FAR.GUARD, n + 2 * FAR.GUARD)]
            for off, m in windows:
                assert 0 <= off and off + m <= FAR.SPAN
            assert not FAR.overlaps(*windows[0], *windows[1]) and FAR.aliases(near, n) == []
            wrong = FAR.aliases(at, n)
            assert wrong, "a far range has aliases"
            for off, m in wrong:
                assert -FAR.LEAD <= off and off + m <= FAR.SPAN, (off, m)
                assert not FAR.overlaps(off, m, *windows[0]) and not FAR.overlaps(off, m, *windows[1]), (off, m)


def test_aliases_are_the_three_wrong_arithmetics():
    """Byte by byte, for ranges across each boundary: the low 32 bits, those sign-extended, the low 31 bits."""
    for at in ((1 << 31) - 3, (1 << 32) - 3, (1 << 32) + (1 << 31) - 3, FAR.BEYOND, 5):
        want = set()
        for b in range(at, at + 7):
            low32 = b & 0xffffffff
            want |= {w for w in (low32, low32 - (1 << 32) if low32 >> 31 else low32, b & 0x7fffffff) if w != b}
        got = {off + i for off, n in FAR.aliases(at, 7) for i in range(n)}
        assert got == want, at
    assert min(off for off, _ in FAR.aliases((1 << 31) - 3, 7)) == -FAR.LEAD


@pytest.mark.parametrize("align", [1, 4, 16])
def test_a_straddling_placement_holds_its_boundary_strictly_inside(align):
    for n in (2 * align + 2, 35, 4097, 123457, FAR.MAX_RANGE):
        for kind, boundary in (("s31", 1 << 31), ("s32", 1 << 32)):
            at = FAR.placement(kind, n, align)
            assert at % align == 0 and at < boundary < at + n - 1
    assert FAR.placement("beyond", 35, 1) == (1 << 32) + (1 << 25) + 4099 and FAR.placement("beyond", 35, 16) % 16 == 0
    assert FAR.LEAD == 1 << 31 and FAR.SPAN == (1 << 32) + (1 << 26)


# ---------------------------------------------------------------- the families
def test_every_batch_family_of_the_header_has_a_relocator():
    families = set(re.findall(r"\bint\s+ohgpu_(\w+?)_batch_create\s*\(", HEADER))
    assert len(families) >= 17 and families == set(FAR.RELOCATE) == set(FAR.ALIGN)
    # ... and a far test of its name that relocates it (read from the module's text: a test module is not imported)
    text = open(os.path.join(ROOT, "tests", "test_gpu_far_offsets.py")).read()
    assert set(re.findall(r"^def test_(\w+)\(", text, re.M)) == families
    for family in families:
        body = text[text.index(f"def test_{family}("):]
        body = body[:body.find("\n\n\n")]
        assert f'"{family}"' in body and "FAR.SPAN" in body and "FAR.Twin(" in body, family


TABLES = {"pcm": {"descs": capi.MSG_DESC}, "fmt": {"descs": capi.FMT_DESC}, "dsd": {"descs": capi.DSD_DESC}, "dsd_pcm": {"descs": capi.DSD_PCM_MSG_DESC},
          "flac": {"descs": capi.FLAC_STREAM_DESC}, "alac": {"descs": capi.ALAC_STREAM_DESC, "packets": capi.ALAC_PACKET},
          "raop": {"descs": capi.RAOP_STREAM_DESC, "packets": capi.ALAC_PACKET}, "flywheel": {"descs": capi.FLYWHEEL_DESC},
          "ohm": {"streams": capi.OHM_STREAM, "frames": capi.OHM_FRAME_DESC, "fragments": capi.OHM_FRAGMENT},
          "ohm_rx": {"streams": capi.OHM_RX_STREAM, "datagrams": capi.OHM_RX_DATAGRAM}, "ogg": {"descs": capi.OGG_STREAM_DESC},
          "mp4": {"descs": capi.MP4_STREAM_DESC}, "mp4f": {"descs": capi.MP4F_STREAM_DESC}, "iff": {"descs": capi.IFF_STREAM_DESC},
          "dsd_file": {"descs": capi.DSD_FILE_STREAM_DESC}, "src": {"descs": capi.SRC_MSG_DESC}, "src_pull": {"descs": capi.SRC_PULL_MSG_DESC}}


@pytest.mark.parametrize("family", sorted(FAR.RELOCATE))
def test_relocate_moves_the_listed_fields_and_nothing_else(family):
    assert set(TABLES[family]) == set(FAR.RELOCATE[family])
    rng = np.random.default_rng(len(family))
    tables = {}
    for name, dtype in TABLES[family].items():
        raw = rng.integers(0, 256, size=3 * dtype.itemsize, dtype=np.uint8)
        t = raw.view(dtype).copy()
        for f in dtype.names:                                      # (offsets that do not wrap when moved)
            if f.endswith("_offset") and dtype[f] == np.dtype("<u8"):
                t[f] >>= np.uint64(24)
        tables[name] = t
    src_shift, dst_shift = (1 << 32) + 48, (1 << 31) + 16
    moved = FAR.relocate(family, tables, src_shift, dst_shift)
    seen = {"src": 0, "dst": 0}
    for name, (src_fields, dst_fields) in FAR.RELOCATE[family].items():
        before, after = tables[name], moved[name]
        assert after is not before and after.dtype == before.dtype
        for f in before.dtype.names:
            shift = src_shift if f in src_fields else dst_shift if f in dst_fields else 0
            assert np.array_equal(after[f], before[f] + np.uint64(shift) if shift else before[f]), (name, f)
        # every offset into an arena the table has is listed: the 64-bit fields named *_offset
        offsets = {f for f in before.dtype.names if f in ("src_offset", "dst_offset")}
        assert offsets == set(src_fields) | set(dst_fields), (name, offsets)
        seen["src"] += len(src_fields)
        seen["dst"] += len(dst_fields)
    assert seen["src"] == 1 and seen["dst"] == (0 if family == "mp4" else 1)


def test_every_64_bit_field_of_the_result_structs_is_classified():
    """RESULTS against the header: each struct it names, its uint64_t / int64_t fields, each in exactly one list."""
    for struct, lists in FAR.RESULTS.items():
        body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}\s*" + struct + ";", HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in re.findall(r"\bu?int64_t\s+([^;]+);", body):
            fields += [f.strip() for f in decl.split(",")]
        listed = [f for k in ("src", "dst", "same") for f in lists.get(k, ())]
        if struct == "ohgpu_ohm_rx_stream_result":                # (its first fields are an ohgpu_ohm_rx_state, named there)
            fields.append("last_sample_start")
        assert sorted(listed) == sorted(fields), (struct, sorted(fields))
    structs = set(re.findall(r"typedef struct (ohgpu_\w*(?:result|record|run|frame|sample|ogg_packet))\s*\{", HEADER))
    with_64 = {s for s in structs if re.search(r"int64_t", re.search(r"typedef struct " + s + r"\s*\{(.*?)\}\s*" + s + ";", HEADER, re.S).group(1))}
    assert with_64 - {"ohgpu_ohm_frame"} <= set(FAR.RESULTS) | {"ohgpu_flac_frame"}, with_64 - set(FAR.RESULTS)
