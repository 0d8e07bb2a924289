"""The workgroup matrix kernel's LDS work, read off its gfx950 assembly and off the bank model (no GPU needed).

Tiles.  Where the accumulators' initial values stay in registers (WgGeom::kBiasRegs: packed stereo S24 and S16 through the
polyphase filters) a tile reads its six sample operands from the LDS and nothing else; six and eight channels (the first
would spill, the second measured slower) and the planar forms keep their table and its two reads a tile.

Split.  tools/micro/lds_conflicts.py models the banks for the stereo split's lane roles: the ones the kernel keeps, and the two
conflict-free ones that were measured against them and not kept.
"""
import importlib.util
import os
import re

from test_mfma_kernel_asm import NAME, ROOT, wg  # noqa: F401  (the fixture: one cross-compile shared with that module's cache)


def _key(name):
    rows, planar, pairs, hb, src_le, dst_le = (int(x) for x in NAME.match(name).groups())
    return rows, planar, pairs, bool(hb)


def _bias_in_registers(name):
    rows, planar, pairs, hb = _key(name)
    return not hb and planar in (0, 4) and pairs == 1


def _lds_reads(body):
    """[(line index, mnemonic)] of every LDS read, and the index of the first and the last matrix instruction."""
    tiles = [i for i, l in enumerate(body) if "v_mfma_i32_16x16x64_i8" in l]
    reads = [(i, m.group(1)) for i, l in enumerate(body) for m in [re.match(r"^\s*(ds_read\w*)", l)] if m]
    return reads, tiles[0], tiles[-1], len(tiles) // 12


def _blocks(body, mnemonic):
    """Lengths of the runs of consecutive `mnemonic` lines."""
    runs, cur = [], 0
    for l in body:
        if re.match(r"^\s*" + mnemonic + r"\s", l):
            cur += 1
        elif cur:
            runs.append(cur)
            cur = 0
    return runs


def test_a_tile_reads_six_operands_and_nothing_else_where_the_constants_are_in_registers(wg):
    """Between the first and the last matrix instruction every LDS read is a ds_read_b64 of a tile's operands; they come six at a
    time (issue_planes is one block), one block per tile -- but that the first tile of a pattern may share its block between the
    ramped and the plain copy of the tiles (the reads are issued before the copies part), and the very first is issued in front
    of the first matrix instruction."""
    seen = 0
    for name, (rows, planar, body, meta) in wg.items():
        if not _bias_in_registers(name):
            continue
        seen += 1
        reads, first, last, n_tiles = _lds_reads(body)
        inside = [m for i, m in reads if first <= i <= last]
        assert inside and set(inside) == {"ds_read_b64"}, (name, sorted(set(inside)))
        assert not [m for i, m in reads if m == "ds_read2_b64"], name                  # the table's reads, anywhere
        blocks = _blocks(body, "ds_read_b64")
        assert set(blocks) == {6}, (name, sorted(set(blocks)))
        copies = 2 * (rows // 8)                                                       # (pattern of the wave's tiles) x (ramped or not)
        assert n_tiles - copies // 2 <= len(blocks) <= n_tiles, (name, len(blocks), n_tiles)
        assert 6 * (len(blocks) - copies // 2) <= len(inside) <= 6 * len(blocks), (name, len(inside), len(blocks))
    assert seen == 8, seen                                                             # stereo S24, stereo S16: four byte orders each


def test_six_channels_and_the_planar_forms_keep_their_table(wg):
    """Unchanged: two reads of initial values a tile beside the six operand reads -- ds_read2_b64 of the two-copy table (six and
    eight channels), 16-byte reads of the four-copy one (planar) -- and the half-band forms, whose two values were in registers already,
    read operands only."""
    seen = 0
    for name, (rows, planar, body, meta) in wg.items():
        r, pl, pairs, hb = _key(name)
        if _bias_in_registers(name):
            continue
        seen += 1
        reads, first, last, n_tiles = _lds_reads(body)
        inside = [m for i, m in reads if first <= i <= last]
        assert set(_blocks(body, "ds_read_b64")) == {6}, name
        if hb:
            assert set(inside) == {"ds_read_b64"}, (name, sorted(set(inside)))
        elif pairs in (3, 4):
            assert set(inside) == {"ds_read_b64", "ds_read2_b64"}, (name, sorted(set(inside)))
            assert sum(m == "ds_read2_b64" for i, m in reads) == 2 * n_tiles, name
        else:
            assert pl in (1, 2, 3) and set(inside) == {"ds_read_b64", "ds_read_b128"}, (name, sorted(set(inside)))
            assert 2 * n_tiles - 2 <= sum(m == "ds_read_b128" for m in inside) <= 2 * n_tiles, name
    assert seen == 2 * 4 + 3 * 4 + 6, seen                                             # six and eight channels; the half-band forms; the planar ones


def _model():
    spec = importlib.util.spec_from_file_location("lds_conflicts", os.path.join(ROOT, "tools", "micro", "lds_conflicts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_bank_model_of_the_stereo_split():
    """The lane roles the kernel keeps -- lane = row on the union run -- are conflict-free on the plane stores and on the tiles' reads;
    the split's 4-byte reads meet their banks twice (312 LDS cycles a pass for 156).  Two roles that model to no conflict anywhere --
    half waves of four rows x eight half chunks on the union run, and every row 16-byte aligned with lanes by ds_read_b128's
    groups -- were built, were bit-exact and measured no faster, so they are models here and not kernel code."""
    m = _model()
    every = [(r, h) for r in range(16) for h in range(24)]
    kept = m.stereo_split_model()
    assert kept["tasks_once"], kept                        # every (row, half chunk) of the pass, once
    assert kept["store_cycles"] == kept["store_ideal"] == 6 * 8, kept           # six wave-rounds x one ds_write_b128 a digit x eight groups
    assert (kept["read_cycles"], kept["read_ideal"]) == (312, 6 * 13 * 2), kept   # thirteen dwords a task, two groups of 32 lanes
    cycles, ideal, agree = m.stereo_tile_read_model()
    assert agree and cycles == ideal, (cycles, ideal, agree)
    for kw in (dict(task=m.stereo_union_group_task, swizzle=1), dict(task=m.stereo_lane_task, aligned=True, swizzle=3)):
        tried = m.stereo_split_model(**kw)
        assert tried["tasks_once"] and tried["read_cycles"] == tried["read_ideal"] and tried["store_cycles"] == tried["store_ideal"], (kw, tried)
        cycles, ideal, agree = m.stereo_tile_read_model(kw["swizzle"])
        assert agree and cycles == ideal, (kw, cycles, ideal, agree)
    for wave in range(4):                                  # (the aligned roles' lane arithmetic is the table of ds_read_b128's lane groups)
        for lane in range(64):
            assert m.stereo_lane_task(wave, lane, 0) in every
    # ... and the model does see the conflicts of roles that have them: lane = row on aligned rows, the groups without the swizzle
    assert m.stereo_split_model(aligned=True)["read_cycles"] == 4 * 72
    assert m.stereo_split_model(task=m.stereo_lane_task, aligned=True)["store_cycles"] == 4 * 48
