"""The PCM message path on the device against tests/pcm_textbook.py (messages the model is fast enough for: up to MODEL_MAX_SUB
subsamples) and against the oracle that tests/test_pcm_textbook.py ties to the model (larger ones), at the shapes where the
planner and the line kernel cut: csrc/pcm_line_kernel.hip's chunks of 512 subsamples (staged path), groups of four subsamples, trips
of 128 groups, merged plain runs re-cut near 4096 subsamples, first / last destination dword written byte by byte, 16-byte source
pieces at the arena's very ends.  Zero differing bytes everywhere, guard bytes included.

Every test first asks ohgpu_batch_paths_info which path the planner chose (staged / register-plain "group" / register ramped-or-
attenuated "heavy") and asserts it, then runs under both kernel variants (`vctx`: the tuned line kernel, and variant 1 = the
generic kernel of csrc/pcm_kernels.hip, which must give the same bytes from the same batch description).

The largest message: ohgpu_pcm_batch_create states no cap of its own -- validate_msg (csrc/api_pcm.hip) bounds a message by its
arenas, by n_frames < 2^32 and, when ramped, by n_frames <= 131071 (the reference's TInt ramp product, Msg.cpp:835) -- so messages
beyond the reference's 9216-byte cell are part of the contract and are tested here against the model directly
(test_messages_beyond_the_reference_cell).  Prefixes are not reachable through ohgpu_pcm_batch_create (only the Songcast frame
batch passes them): they are tests/test_gpu_ohm_textbook.py's.

Mutations of the library these tests were seen to fail under on an MI355X (one build each, never committed; all of them produce
wrong bytes only):
  * csrc/pcm_line_kernel.hip ramp_out_sel, `pos = le ? db - 1 - m : m` replaced by `le ? db - m : m` (the ramped group path's
    little-endian output selector): 19 failures -- test_cutting_rules_within_one_message and
    test_ramp_shapes_at_every_channel_count at all nine 16/24/32-bit depth pairs, test_uniform_and_mixed_batches_give_equal_bytes.
  * plan_pcm_line, `magic_u31(d.n_frames > 1 ? d.n_frames - 1 : 1, ...)` replaced by `... ? d.n_frames : 1` (`frames - 1`
    replaced by `frames` in the ramp's division): 41 failures -- every test that ramps, on the staged and the register path alike.
  * plan_pcm_line, staged chunks' `c.q0 = (uint32_t)q0` replaced by `c.q0 = 0` (a later chunk of a message ramps and places its
    silence id bytes as if it were the first): 12 failures -- every case with 8-bit audio on either side in
    test_cutting_rules_within_one_message, test_ramp_shapes_at_every_channel_count, test_every_source_and_destination_alignment and
    test_arenas_sized_to_the_byte.
(The generic kernel, variant 1, shares none of the three: its cases stayed green under each, as they should.)
"""
import itertools

import numpy as np
import pytest

import oracle_lib as O
import pcm_textbook as PT
from ohpipeline_amd import capi
from pcm_cases import (LE, BE, kMax, DEPTHS, ENDIANS, MODEL_MAX_SUB, FILL, PLAIN, RAMPED, ATTENUATED, SILENT, expected, path_of, fields,
                       pack)   # noqa: F401  (the builders: shared with the far-offset tests)

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["tuned", "v1"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    yield ctx
    ctx.set_kernel_variant(0)


def run(ctx, descs, src, dst_bytes):
    """(device output over the WHOLE destination arena, the batch's paths).  Both arenas are allocated to the byte."""
    d_src = ctx.upload(src if src.size else np.zeros(1, np.uint8))
    d_dst = ctx.malloc(max(dst_bytes, 1))
    ctx.memset(d_dst, FILL, max(dst_bytes, 1))
    b = ctx.pcm_batch(descs, src.size, dst_bytes)
    try:
        paths = ctx.batch_paths(b)
        ctx.pcm_run(b, d_src, d_dst)
        out = ctx.download(d_dst, dst_bytes)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return out, paths


def check(ctx, descs, src, dst_bytes, what):
    got, paths = run(ctx, descs, src, dst_bytes)
    want = expected(descs, src, dst_bytes)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} differing bytes, first at {bad[:6].tolist()} (paths {paths})"
    return paths


def largest(sbits, ch):
    return O.MAX_BYTES // (ch * sbits // 8)


CUT_COUNTS = [1, 2, 3, 4, 5, 7, 8, 9, 507, 508, 509, 511, 512, 513, 515, 516, 517, 1019, 1020, 1021, 1023, 1024, 1025, 1027, 1028, 1029]


@pytest.mark.parametrize("sbits,dbits", list(itertools.product(DEPTHS, DEPTHS)))
def test_cutting_rules_within_one_message(vctx, sbits, dbits):
    """One-channel messages (frames = subsamples) of 4k +/- 1, 511..513, 1023..1025, 128 groups +/- 1 group and +/- 1 subsample, 256
    groups likewise, the largest message the depth admits in a reference cell and that minus one frame (also at three channels);
    plain and ramped each (silent and, at 16 bits, attenuated on a rotation), back to back with no gap so that partial first and
    last dwords share their dword with a neighbour, every byte-order pair, every depth pair."""
    rng = np.random.default_rng(1000 + sbits * 8 + dbits)
    for se, de in ENDIANS:
        counts = CUT_COUNTS + [largest(sbits, 1) - 1, largest(sbits, 1)]
        msgs = []
        for k, n in enumerate(counts):
            msgs += [(n, 1, PLAIN), (n, 1, RAMPED)]
            if k % 3 == 0:
                msgs.append((n, 1, SILENT))
            if sbits == 16 and k % 3 == 1:
                msgs.append((n, 1, ATTENUATED))
        msgs += [(largest(sbits, 3), 3, RAMPED), (largest(sbits, 3) - 1, 3, PLAIN), (largest(sbits, 3), 3, PLAIN)]
        descs, src, dst_bytes = pack(rng, msgs, sbits, se, dbits, de, src_lead=(sbits + dbits) // 8 % 5)
        paths = check(vctx, descs, src, dst_bytes, f"{sbits}->{dbits} se={se} de={de}")
        kinds = {path_of(sbits, dbits, kind) for _, _, kind in msgs}
        assert paths["line_planned"] == 1 and all(paths[k] > 0 for k in kinds), paths
        assert all(paths[k] == 0 for k in ("staged_chunks", "group_chunks", "heavy_chunks") if k not in kinds), paths
        if "heavy_chunks" in kinds:
            assert paths["heavy_chunks"] == sum(kind in (RAMPED, ATTENUATED) for _, _, kind in msgs)     # one chunk per message


OFFSET_CASES = [(24, 24, PLAIN), (32, 16, PLAIN), (16, 24, RAMPED), (24, 32, RAMPED), (16, 16, ATTENUATED), (8, 16, PLAIN),
                (24, 8, RAMPED), (24, 24, SILENT)]


@pytest.mark.parametrize("sbits,dbits,kind", OFFSET_CASES)
def test_every_source_and_destination_alignment(vctx, sbits, dbits, kind):
    """Source offset mod 16 = 0..15 x destination offset mod 16 = 0..15 x subsample counts around a group, a trip and a chunk, on
    each path; every message in a slot of its own with guard bytes on both sides."""
    rng = np.random.default_rng(2000 + sbits + dbits)
    counts = [1, 3, 4, 5, 8, 9, 129, 513]
    rows, sp, dp = [], 0, 0
    for (so, do), n in itertools.product(itertools.product(range(16), range(16)), counts):
        k = len(rows)
        flags, att, ramp = fields(kind, sbits, k)
        ch = 1 if n % 2 else (n if n < 9 else 1)
        sp = (sp + 15) // 16 * 16 + so
        dp = (dp + 15) // 16 * 16 + 16 + do
        rows.append((sp, dp, n // ch, ramp[0], ramp[1], att, ch, sbits, LE if k % 2 else BE, dbits, LE if k % 3 == 0 else BE, flags))
        sp += n * sbits // 8
        dp += n * dbits // 8
    descs = np.array(rows, dtype=O.MSG_DESC)
    src = rng.integers(0, 256, size=sp, dtype=np.uint8)
    paths = check(vctx, descs, src, dp + 7, f"{sbits}->{dbits} {kind}")
    mine = path_of(sbits, dbits, kind)
    assert paths["line_planned"] == 1 and paths["launches"] == 1 and paths[mine] >= (len(rows) if mine != "group_chunks" else 1), paths
    assert all(paths[k] == 0 for k in ("staged_chunks", "group_chunks", "heavy_chunks") if k != mine), paths


@pytest.mark.parametrize("sbits,dbits,kind", [(24, 24, PLAIN), (16, 32, PLAIN), (32, 24, RAMPED), (16, 16, ATTENUATED), (8, 24, PLAIN),
                                              (16, 8, RAMPED)])
def test_arenas_sized_to_the_byte(vctx, sbits, dbits, kind):
    """A message that starts at byte 0 and one that ends exactly where the uploaded source arena ends, the two back to back and the
    arenas allocated to the byte: the 16-byte pieces (staged path) and the unaligned group loads (register path) stay inside."""
    rng = np.random.default_rng(3000 + sbits + dbits)
    for n, m in [(1, 1), (2, 3), (3, 5), (5, 4), (16, 17), (17, 16), (129, 127), (513, 511), (1, 1025)]:
        descs, src, dst_bytes = pack(rng, [(n, 1, kind), (m, 1, kind)], sbits, LE, dbits, BE, dst_lead=0, dst_tail=0)
        assert int(descs["src_offset"][0]) == 0 and int(descs["src_offset"][1]) + m * sbits // 8 == src.size
        assert int(descs["dst_offset"][1]) + m * dbits // 8 == dst_bytes
        paths = check(vctx, descs, src, dst_bytes, f"{sbits}->{dbits} {kind} n={n},{m}")
        assert paths[path_of(sbits, dbits, kind)] >= 1, paths


RUN_TOTALS = [[600, 3495], [600, 3496], [600, 3497], [2048, 2047], [2048, 2048], [2048, 2049], [4095, 4097], [4096, 4096], [4097, 4095],
              [600, 7591], [600, 7592], [600, 7593], [4096, 4095], [4096, 4097], [1365, 1365, 1365], [1365, 1366, 1365, 4097],
              [100, 1000], [3, 4, 5, 4080, 4], [8193]]


@pytest.mark.parametrize("sbits,dbits", list(itertools.product([16, 24, 32], [16, 24, 32])))
def test_plain_runs_around_the_merged_chunk_size(vctx, sbits, dbits):
    """Runs of one stream's plain messages that the planner appends to one chunk and re-cuts near 4096 subsamples
    (kGroupChunkSub): totals of 4095 / 4096 / 4097 and 8191 / 8192 / 8193 subsamples with the size boundary inside a message, exactly
    between two messages, and one subsample to either side; every register depth pair, at 1 and 2 channels, 128-byte aligned and
    unaligned destinations.  [600, 3496] and [100, 1000] must come out as ONE chunk (the merge really happened: the second message's
    target is below 1.25 times the run); a run never takes the staged or the heavy path.  NOT covered: merging of up to eight
    messages per chunk, which the planner only does for batches of some 400 000 plain messages and more (merge_msgs > 1)."""
    rng = np.random.default_rng(4000 + sbits + dbits)
    for (se, de), lead in zip(ENDIANS, (0, 1, 128, 77)):
        for sizes in RUN_TOTALS:
            for ch in (1, 2):
                msgs = [((n + ch - 1) // ch, ch, PLAIN) for n in sizes]
                descs, src, dst_bytes = pack(rng, msgs, sbits, se, dbits, de, src_lead=lead % 7, dst_lead=lead)
                descs["flags"] = 0                               # (one selector for the whole run: a ZERO_LSB32 message would end it)
                paths = check(vctx, descs, src, dst_bytes, f"{sbits}->{dbits} {sizes} ch={ch} lead={lead}")
                assert paths["staged_chunks"] == 0 and paths["heavy_chunks"] == 0 and paths["launches"] == 1, paths
                if ch == 1 and sizes in ([600, 3496], [100, 1000]):
                    assert paths["group_chunks"] == 1, (sizes, paths)
                if ch == 1 and sizes == [8193]:
                    assert paths["group_chunks"] == 2, paths      # (one message, cut where the run passes a chunk and a quarter)


@pytest.mark.parametrize("sbits,dbits,ch", [(24, 24, 2), (16, 24, 2), (32, 16, 6), (16, 16, 1)])
def test_runs_of_five_interrupted_in_every_position(vctx, sbits, dbits, ch):
    """Five back-to-back messages of one stream, four plain and one ramped / attenuated / silent in every position: the plain
    neighbours merge around it, the interrupter takes its own path, and the bytes on both sides of every seam are right."""
    rng = np.random.default_rng(5000 + sbits + dbits)
    for kind in (RAMPED, SILENT) + ((ATTENUATED,) if sbits == 16 else ()):
        for pos, n in itertools.product(range(5), (1, 43, 220)):
            msgs = [(n, ch, kind if k == pos else PLAIN) for k in range(5)]
            descs, src, dst_bytes = pack(rng, msgs, sbits, LE, dbits, BE, src_lead=pos, dst_lead=pos + 1)
            descs["flags"] &= ~np.uint8(O.FLAG_ZERO_LSB32)
            paths = check(vctx, descs, src, dst_bytes, f"{sbits}->{dbits} {kind} at {pos}, n={n}")
            assert paths[path_of(sbits, dbits, kind)] >= 1 and paths["group_chunks"] >= 1, paths
            if kind != SILENT:
                assert paths["heavy_chunks"] == 1 and paths["staged_chunks"] == 0, paths
            else:
                assert paths["heavy_chunks"] == 0 and paths["launches"] == 1, paths      # (silence rides in its layout's launch)


@pytest.mark.parametrize("sbits,dbits", [(16, 16), (16, 24), (16, 32), (24, 16), (24, 24), (24, 32), (32, 16), (32, 24), (32, 32), (8, 8),
                                         (8, 24), (24, 8)])
def test_ramp_shapes_at_every_channel_count(vctx, sbits, dbits):
    """frames == 1 (the start value, no division), frames == 2, up-ramps (the truncation toward zero works the other way), endpoints
    one apart, flat ramps, at 1, 2, 3, 5, 6, 7, 8 channels (frame = subsample / channels: the multiplier changes inside a group of
    four subsamples in every possible position), and the largest ramped message validation admits (131071 frames)."""
    rng = np.random.default_rng(6000 + sbits + dbits)
    ramps = [(kMax, 0), (0, kMax), (kMax, kMax - 1), (100, 101), (8191, 8190), (5, 5), (kMax, kMax), (0, 0), (17, 16001), (16001, 17)]
    rows, sp, dp = [], 1, 2
    for ch, n, ramp in itertools.product([1, 2, 3, 5, 6, 7, 8], [1, 2, 3, 4, 5, 9, 43], ramps):
        k = len(rows)
        rows.append((sp, dp, n, ramp[0], ramp[1], 256, ch, sbits, LE if k % 2 else BE, dbits, LE if k % 3 == 0 else BE, O.FLAG_RAMP))
        sp += n * ch * sbits // 8
        dp += n * ch * dbits // 8
    for ramp in [(kMax, 0), (0, kMax), (8191, 8190)]:
        rows.append((sp, dp, 131071, ramp[0], ramp[1], 256, 1, sbits, LE, dbits, BE, O.FLAG_RAMP))
        sp += 131071 * sbits // 8
        dp += 131071 * dbits // 8
    descs = np.array(rows, dtype=O.MSG_DESC)
    src = rng.integers(0, 256, size=sp, dtype=np.uint8)
    paths = check(vctx, descs, src, dp + 3, f"{sbits}->{dbits}")
    mine = path_of(sbits, dbits, RAMPED)
    assert paths[mine] >= len(rows) and paths["group_chunks"] == 0 and paths["launches"] == 1, paths
    with pytest.raises(capi.OhGpuError):                          # one frame more overflows the reference's TInt product: refused
        bad = descs[-1:].copy()
        bad["n_frames"] = 131072
        vctx.pcm_batch(bad, src.size + 8, dp + 8)


def test_uniform_and_mixed_batches_give_equal_bytes(vctx):
    """The same messages as a batch of one layout and inside a batch that mixes every layout (a launch per layout): equal bytes."""
    rng = np.random.default_rng(7000)
    layouts = [(sb, se, db, de) for sb, db in itertools.product(DEPTHS, DEPTHS) for se, de in ((LE, BE), (BE, LE))]
    per_layout, src_parts, sp, dp = [], [], 0, 0
    for k, (sb, se, db, de) in enumerate(layouts):
        msgs = [(n, 1 + (k + j) % 3, [PLAIN, RAMPED, PLAIN, SILENT, PLAIN][j]) for j, n in enumerate([5, 43, 130, 7, 300])]
        d, s, nbytes = pack(rng, msgs, sb, se, db, de, dst_lead=k % 4, dst_tail=k % 3)
        d["src_offset"] += sp
        d["dst_offset"] += dp
        per_layout.append((d, sp, s.size, dp, nbytes))
        src_parts.append(s)
        sp += s.size
        dp += nbytes
    src = np.concatenate(src_parts)
    mixed = np.concatenate([np.stack([d[j] for d, *_ in per_layout]) for j in range(5)])      # layouts alternate message by message
    got_mixed, paths = run(vctx, mixed, src, dp)
    assert paths["launches"] == 10 and paths["staged_chunks"] > 0 and paths["group_chunks"] > 0 and paths["heavy_chunks"] > 0, paths
    assert np.array_equal(got_mixed, expected(mixed, src, dp))
    for d, s0, sn, d0, dn in per_layout:
        got, p = run(vctx, d, src, dp)
        assert p["launches"] == 1, p
        assert np.array_equal(got[d0:d0 + dn], got_mixed[d0:d0 + dn]), (int(d["src_bits"][0]), int(d["dst_bits"][0]))
        assert (got[:d0] == FILL).all() and (got[d0 + dn:] == FILL).all()


@pytest.mark.parametrize("sbits", [24, 32])
def test_messages_beyond_the_reference_cell(vctx, sbits):
    """Single messages of 4097 and 8193 subsamples (12 291 .. 32 772 bytes: beyond DecodedAudio::kMaxBytes) against the MODEL, plain
    and ramped, to every register depth: validation admits them, so they are part of the contract."""
    rng = np.random.default_rng(8000 + sbits)
    for dbits, n, kind in itertools.product([16, 24, 32], [4097, 8193], [PLAIN, RAMPED]):
        descs, src, dst_bytes = pack(rng, [(n, 1, kind)], sbits, LE, dbits, BE, src_lead=1, dst_lead=1)
        got, paths = run(vctx, descs, src, dst_bytes)
        want = np.full(dst_bytes, FILL, dtype=np.uint8)
        PT.process_batch(descs, src, want)
        assert np.array_equal(got, want), (sbits, dbits, n, kind, paths)
        assert paths[path_of(sbits, dbits, kind)] >= 1 and paths["staged_chunks"] == 0, paths


def test_paths_query_refuses_other_batches(ctx):
    d = np.zeros(1, dtype=capi.FLYWHEEL_DESC)
    d["channel_bytes"], d["in_samples"], d["out_frames"], d["block_frames"], d["sample_rate"], d["channels"] = 176, 44, 882, 44, 44100, 2
    b = ctx.flywheel_batch(d, 176 * 2, 882 * 8)
    try:
        with pytest.raises(capi.OhGpuError) as e:
            ctx.batch_paths(b)
        assert e.value.code == capi.ERR_INVALID
    finally:
        ctx.batch_destroy(b)
    empty = ctx.pcm_batch(np.zeros(0, dtype=O.MSG_DESC), 0, 16)
    try:
        assert not any(ctx.batch_paths(empty).values())
    finally:
        ctx.batch_destroy(empty)
