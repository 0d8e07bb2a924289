"""DSD on the device (ohgpu_dsd_batch_create / ohgpu_dsd_batch_run / ohgpu_dsd_process_host: the DSF, DFF and raw packers, the
playable pass-through, silence and the 0x69 tail fill) against tests/dsd_textbook.py, on both of the planner's paths
(csrc/dsd_line_kernel.hip, plan_dsd_line) and, under kernel variant 1, on dsd_kernel_v1:

    wide      a descriptor whose offsets are 16-byte aligned and that has a body of whole lanes: a packer with P <= 4 and at least
              8 chunks (a lane = 8 chunks = two 16-byte loads, two to four 16-byte stores), a pass-through or a silence of at
              least 16 bytes.  Its last n % 8 chunks and the edges of its fill still go out byte by byte.
    generic   every other descriptor that has chunks: byte by byte.

Conventions, as tests/test_gpu_fmt_textbook.py: both arenas allocated to the byte, the destination pre-filled with 0xA5, the WHOLE
destination arena compared with the model's, zero differing bytes.  Every check first asks ohgpu_dsd_batch_paths how the batch was
planned and asserts the counts against the rule above, recomputed here (`planned`), then compares; every test that runs a kernel
runs under the tuned kernel and under variant 1 (`vctx`), each against the model.  A piece is 2048 chunks, a wave's pass 512, a
lane 8: the chunk counts go round each of them.

Mutations of the library that these tests are meant to fail under (to be built once each, never committed; all of them produce
wrong bytes inside the arenas only).  None has been built yet, so what each is expected to break is a prediction:
  * dsd_src_of, DFF's `c * 4 + ch + 2 * i` replaced by `c * 4 + ch * 2 + i` (the wide path packs DFF as if it were Raw): expected to
    fail every tuned DFF case with a wide body and leave every variant-1 case green.
  * dsd_fill, the tail's `lane < len - tail0` replaced by `lane + 1 < len - tail0` (the fill's last byte is left out): expected to fail
    the tuned tail, silence, alignment and exact-arena cases whose fill does not end on a 16-byte boundary.
  * dsd_kernel_v1, DSF's `pl[4096]` replaced by `pl[4097]`: expected to fail every variant-1 DSF case and no tuned one.
(The wide path's selector tables -- dsd_perm for the nine instantiations -- were replayed on the CPU with v_perm_b32 and
v_bfrev_b32 emulated, eight chunks against a per-byte statement: all nine agree.)
"""
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest

import dsd_textbook as DT
from ohpipeline_amd import capi
from dsd_cases import (FILL, PASS, DSF, DFF, RAW, KINDS, FORMATS, MORE_FORMATS, CUTS, Batch, whole, planned,
                       expected)   # noqa: F401  (the builders: shared with the far-offset tests)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "dsd_textbook.json")
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
    """(device output over the WHOLE destination arena, the batch's paths, its totals).  Both arenas are allocated to the byte."""
    d_src = ctx.upload(src if src.size else np.zeros(1, np.uint8))
    d_dst = ctx.malloc(max(dst_bytes, 1))
    ctx.memset(d_dst, FILL, max(dst_bytes, 1))
    b = ctx.dsd_batch(descs, src.size, dst_bytes)
    try:
        paths, info = ctx.dsd_batch_paths(b), ctx.batch_info(b)
        with pytest.raises(capi.OhGpuError):                               # (the PCM / fmt query does not know this kind of batch)
            ctx.batch_paths(b)
        ctx.dsd_run(b, d_src, d_dst)
        out = ctx.download(d_dst, dst_bytes) if dst_bytes else np.zeros(0, np.uint8)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return out, paths, info


def check(ctx, batch, what, wide=None, generic=None):
    """Asserts the plan (against the rule, and against the counts the test means to reach, when given), then zero differing bytes
    over the whole arena."""
    descs, src, dst_bytes = batch
    got, paths, info = run(ctx, descs, src, dst_bytes)
    assert paths == planned(descs), (what, paths, planned(descs))
    if wide is not None:
        assert paths["wide_descs"] == wide, (what, paths)
    if generic is not None:
        assert paths["generic_descs"] == generic, (what, paths)
    assert info == DT.totals(descs), what
    want = expected(descs, src, dst_bytes)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} differing bytes, first at {bad[:6].tolist()} ({paths})"
    return paths


# ---------------------------------------------------------------- the wide path
@pytest.mark.parametrize("kind", [PASS, DSF, DFF, RAW], ids=KINDS.values())
def test_every_format_around_every_cut(vctx, kind):
    """Every (W, P) x chunk counts around a lane (8), a wave's pass (512) and a piece (2048) and two pieces, all offsets 16-byte
    aligned: the wide path wherever the rule has one (P = 8 has none for a packer).  DSF and DFF take the counts as they are -- most
    end inside a block, so the fill follows a ragged end -- Raw and pass-through whole blocks (the count rounded up).  DSF runs of
    2049 .. 6151 chunks cross one and two plane pairs and end inside one."""
    b = Batch(7100 + kind)
    for (W, P), n in itertools.product(MORE_FORMATS, CUTS):
        b.add(kind, W, P, n if kind in (DSF, DFF) else whole(n, W - P), sres=0, dres=0, gap=16 * (n % 2))
    batch = b.finish(dst_tail=16)
    rule = planned(batch[0])
    assert rule["wide_descs"] > 4 * len(CUTS) and rule["generic_descs"] >= (1 if kind == PASS else 2)
    check(vctx, batch, f"{KINDS[kind]} around the cuts")


@pytest.mark.parametrize("kind", [PASS, DSF, DFF, RAW], ids=KINDS.values())
def test_silence_of_every_format(vctx, kind):
    """OHGPU_DSD_FLAG_SILENCE on every kind: no source is read (the source arena is empty), every byte 0x69, whole blocks from one
    block to several pieces, at aligned and odd destinations."""
    b = Batch(7200 + kind)
    for k, ((W, P), blocks) in enumerate(itertools.product(MORE_FORMATS, (1, 2, 3, 5, 128, 129, 600, 2049))):
        b.add(kind, W, P, blocks * (W - P), dres=0 if k % 3 else (1 + k) % 16, gap=k % 4, silence=True)
    descs, src, dst_bytes = b.finish(dst_tail=3)
    assert src.size == 0
    check(vctx, (descs, src, dst_bytes), f"silence as {KINDS[kind]}")


# ---------------------------------------------------------------- every alignment
@pytest.mark.parametrize("kind", [PASS, DSF, DFF, RAW], ids=KINDS.values())
def test_every_source_and_destination_alignment(vctx, kind):
    """Source residue 0-15 x destination residue 0-15, the format and the chunk count rotating (8 to 70 chunks, tails for DSF and
    DFF): 256 descriptors of which the one at (0, 0) alone is wide; then one of 2100 chunks at each of eight pairs, (0, 0) the last
    (a multiple of 4 or 8 is not enough)."""
    b, k = Batch(7300 + kind, src_lead=1, dst_lead=2), 0
    for sres, dres in itertools.product(range(16), range(16)):
        W, P = FORMATS[k % 4]
        n = 8 + (7 * k) % 63
        b.add(kind, W, P, n if kind in (DSF, DFF) else whole(n, W - P), sres=sres, dres=dres, gap=k % 3)
        k += 1
    for i, (sres, dres) in enumerate(((1, 0), (0, 1), (15, 15), (8, 0), (0, 8), (4, 12), (3, 5), (0, 0))):
        W, P = FORMATS[i % 4]
        b.add(kind, W, P, 2100 if kind in (DSF, DFF) else whole(2100, W - P), sres=sres, dres=dres, gap=1)
    batch = b.finish(dst_tail=5)
    check(vctx, batch, f"{KINDS[kind]} at every alignment", wide=2, generic=256 + 8 - 2)


# ---------------------------------------------------------------- tails
@pytest.mark.parametrize("kind", [DSF, DFF], ids=["dsf", "dff"])
def test_every_tail(vctx, kind):
    """Tails of 1 .. chunks per block - 1 chunks behind 0, 1, 2, 128 and 512 whole blocks, for every format with more than one chunk
    to a block ((16, 0): tails of 1 .. 15), aligned (wide from 8 chunks on) and at odd offsets (generic)."""
    b, k = Batch(7400 + kind, src_lead=3, dst_lead=1), 0
    for (W, P) in ((2, 0), (6, 2), (8, 4), (3, 0), (16, 0), (12, 8)):
        per_block = W - P
        for blocks, tail, odd in itertools.product((0, 1, 2, 128, 512), range(1, per_block), (False, True)):
            b.add(kind, W, P, blocks * per_block + tail, sres=5 if odd else 0, dres=(3 + k) % 16 or 1 if odd else 0, gap=k % 2)
            k += 1
    batch = b.finish(dst_tail=2)
    rule = planned(batch[0])
    assert rule["wide_descs"] > 40 and rule["generic_descs"] > 40
    check(vctx, batch, f"{KINDS[kind]} tails")


def test_five_chunks_make_two_blocks(vctx):
    """The worked case: five DSF or DFF chunks at (6, 2) are 30 bytes of chunks and 18 bytes of 0x69."""
    for kind in (DSF, DFF):
        descs, src, dst_bytes = Batch(7500 + kind).add(kind, 6, 2, 5).finish()
        assert dst_bytes == 48
        got, _, _ = run(vctx, descs, src, dst_bytes)
        assert got[30:].tolist() == [0x69] * 18 and got[0] == 0 and got[3] == 0
        check(vctx, (descs, src, dst_bytes), "five chunks", wide=0, generic=1)


# ---------------------------------------------------------------- batches
def test_mixed_batch_with_empty_descriptors(vctx):
    """All kinds, formats and both paths in one batch, silent descriptors and descriptors of no chunks (their offsets far outside
    the arenas) among them, the first descriptor at byte 0 and the last ending with the last byte of both arenas: one launch."""
    b = Batch(7600)
    shapes = [(DSF, 2, 0, 4100, 0, 0), (DFF, 6, 2, 37, 3, 5), (RAW, 8, 4, 512, 0, 0), (PASS, 6, 2, 1024, 0, 0), (DSF, 6, 2, 2049, 0, 0),
              (RAW, 1, 0, 77, 0, 0), (DFF, 8, 4, 2051, 0, 0), (PASS, 12, 8, 400, 16 - 7, 2), (DSF, 8, 4, 9, 0, 0), (DFF, 1, 0, 8, 0, 0),
              (RAW, 6, 2, 8, 1, 0), (DSF, 12, 8, 333, 0, 0), (DFF, 2, 0, 2047, 0, 0)]
    for k, (kind, W, P, n, sres, dres) in enumerate(shapes):
        b.add(kind, W, P, n, sres=sres, dres=dres, gap=0 if k in (0, len(shapes) - 1) else k % 3)
        if k % 4 == 1:
            b.empty(kind, W, P, silence=k % 8 == 1)
        if k % 5 == 2:
            b.add(kind, W, P, 3 * (W - P), dres=None, silence=True)
    b.add(DFF, 2, 0, 64, sres=0, dres=0)
    descs, src, dst_bytes = b.finish()
    assert int(descs["src_offset"][0]) == 0 and int(descs["dst_offset"][0]) == 0
    assert int(descs["src_offset"][-1]) + 256 == src.size and int(descs["dst_offset"][-1]) + 256 == dst_bytes
    paths = check(vctx, (descs, src, dst_bytes), "mixed")
    assert paths["launches"] == 1 and paths["wide_descs"] >= 8 and paths["generic_descs"] >= 4


def test_more_pieces_than_waves(vctx):
    """12288 descriptors of one to three lanes -- more pieces than the launch has waves on any CDNA part (4 x 8 x CUs), so the piece
    loop goes round -- and no other."""
    b = Batch(7700)
    for k in range(12288):
        kind = (DSF, DFF, RAW, PASS)[k % 4]
        W, P = FORMATS[(k // 4) % 4]
        b.add(kind, W, P, whole(8 + k % 17, W - P), sres=0, dres=0)
    batch = b.finish()
    check(vctx, batch, "12288 pieces", wide=12288, generic=0)


def test_nothing_to_do(vctx):
    """A batch of no descriptors, and one of empty descriptors only: accepted, no launch, nothing written, no arena needed."""
    empty = vctx.dsd_batch(np.zeros(0, dtype=capi.DSD_DESC), 0, 0)
    try:
        assert vctx.dsd_batch_paths(empty) == {"wide_descs": 0, "generic_descs": 0, "launches": 0}
        assert vctx.batch_info(empty) == {"n_msgs": 0, "in_frames": 0, "out_frames": 0, "src_bytes_touched": 0, "dst_bytes_written": 0}
        vctx.dsd_run(empty, None, None)
    finally:
        vctx.batch_destroy(empty)
    descs, src, _ = Batch(7800).empty(DSF, 2, 0).empty(PASS, 8, 4, silence=True).finish()
    got, paths, info = run(vctx, descs, src, 8)
    assert paths == {"wide_descs": 0, "generic_descs": 0, "launches": 0} and (got == FILL).all() and info["n_msgs"] == 2


def test_golden_fixture_batches(vctx):
    """The seeded batches of tests/golden/dsd_textbook.json: the device's whole destination arena hashes to what the model gave
    when the fixture was written."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_dsd_textbook_fixtures as G
    finally:
        sys.path.pop(0)
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["fill"] == FILL and len(fx["batches"]) == 3
    for entry in fx["batches"]:
        rows, src, dst_bytes = G.batches()[entry["name"]]
        assert rows == entry["descriptors"]
        descs = np.zeros(len(rows), dtype=capi.DSD_DESC)
        for i, r in enumerate(rows):
            for key, v in r.items():
                descs[key][i] = v
        src = np.frombuffer(src, dtype=np.uint8)
        assert hashlib.sha256(src.tobytes()).hexdigest() == entry["src_sha256"] and dst_bytes == entry["dst_bytes"]
        got, paths, _ = run(vctx, descs, src, dst_bytes)
        assert paths == planned(descs) and paths["generic_descs"] > 0 and (paths["wide_descs"] > 4 or entry["name"] != "aligned"), (entry["name"], paths)
        assert hashlib.sha256(got.tobytes()).hexdigest() == entry["dst_sha256"], entry["name"]
        check(vctx, (descs, src, dst_bytes), entry["name"])


# ---------------------------------------------------------------- validation
def _one(kind, W, P, n, so=0, do=0, flags=0, reserved=None):
    return np.array([(so, do, n, kind, flags, W, P, reserved or [0] * 8)], dtype=capi.DSD_DESC)


def _refused(ctx, descs, src_bytes, dst_bytes, code):
    before = ctx.device_allocations()
    with pytest.raises(capi.OhGpuError) as e:
        ctx.batch_destroy(ctx.dsd_batch(descs, src_bytes, dst_bytes))
    assert e.value.code == code, (code, str(e.value))
    assert ctx.device_allocations() == before                              # (a refusal keeps nothing)


def test_validation_refusals(ctx):
    """ohgpu_dsd_batch_create's checks, by error code (no kernel runs): unknown kinds and flags, reserved bytes, every (W, P) the
    format does not have, Raw / pass-through / silence that are not whole blocks -- also behind a good descriptor."""
    big = 1 << 20
    warm = ctx.dsd_batch(_one(DFF, 6, 2, 8), big, big)                      # (the context's cache holds a block from here on)
    ctx.batch_destroy(warm)
    for kind in (0, 5, 6, 255):
        _refused(ctx, _one(kind, 6, 2, 4), big, big, capi.ERR_INVALID)
    for flags in (2, 3, 0x80):
        _refused(ctx, _one(DFF, 6, 2, 4, flags=flags), big, big, capi.ERR_INVALID)
    _refused(ctx, _one(DFF, 6, 2, 4, reserved=[0, 0, 0, 1, 0, 0, 0, 0]), big, big, capi.ERR_INVALID)
    for W, P in ((0, 0), (6, 1), (7, 3), (6, 4), (8, 2), (4, 2), (9, 4), (16, 4), (2, 2), (12, 6), (255, 250)):
        for kind in (PASS, DSF, DFF, RAW):
            _refused(ctx, _one(kind, W, P, 0), big, big, capi.ERR_INVALID)
            _refused(ctx, _one(kind, W, P, 0, flags=capi.DSD_FLAG_SILENCE), big, big, capi.ERR_INVALID)
    for W, P in ((2, 0), (6, 2), (8, 4), (12, 8)):
        for n in (1, W - P - 1, W - P + 1, 5 * (W - P) + 1):
            _refused(ctx, _one(RAW, W, P, n), big, big, capi.ERR_INVALID)
            _refused(ctx, _one(PASS, W, P, n), big, big, capi.ERR_INVALID)
            for kind in (PASS, DSF, DFF, RAW):
                _refused(ctx, _one(kind, W, P, n, flags=capi.DSD_FLAG_SILENCE), big, big, capi.ERR_INVALID)
    two = np.concatenate([_one(DFF, 6, 2, 8), _one(RAW, 6, 2, 5, so=64, do=64)])
    _refused(ctx, two, big, big, capi.ERR_INVALID)


# (one descriptor at offsets that are not zero, the bytes of source and destination it needs, whether it is wide)
EXACT = [(_one(DSF, 2, 0, 2049, so=16, do=32), 16 + 2 * 8192, 32 + 2050 * 4, True),
         (_one(DSF, 6, 2, 5, so=3, do=1), 3 + 8192, 1 + 48, False),
         (_one(DFF, 6, 2, 13, so=16, do=16), 16 + 52, 16 + 4 * 24, True),
         (_one(DFF, 8, 4, 9, so=7, do=2), 7 + 36, 2 + 3 * 32, False),
         (_one(RAW, 8, 4, 12, so=32, do=48), 32 + 48, 48 + 96, True),
         (_one(RAW, 1, 0, 9, so=5, do=3), 5 + 36, 3 + 36, False),
         (_one(PASS, 6, 2, 12, so=16, do=16), 16 + 72, 16 + 72, True),
         (_one(PASS, 12, 8, 8, so=1, do=9), 1 + 96, 9 + 96, False),
         (_one(DFF, 2, 0, 6, so=1 << 30, do=16, flags=capi.DSD_FLAG_SILENCE), 0, 16 + 24, True)]


def test_arenas_exact_and_one_byte_short(vctx):
    """One descriptor at offsets that are not zero, on both paths: each arena one byte short is refused as out of bounds; exact is
    accepted, planned as named and right to the last byte under both kernel variants.  (A silent descriptor reads no source: its
    source offset may point anywhere.)"""
    rng = np.random.default_rng(7900)
    for descs, src_bytes, dst_bytes, wide in EXACT:
        if src_bytes:
            _refused(vctx, descs, src_bytes - 1, dst_bytes, capi.ERR_BOUNDS)
        _refused(vctx, descs, src_bytes, dst_bytes - 1, capi.ERR_BOUNDS)
        src = rng.integers(0, 256, size=src_bytes, dtype=np.uint8)
        check(vctx, (descs, src, dst_bytes), f"exact arenas, kind {int(descs['kind'][0])}", wide=int(wide), generic=int(not wide))


# ---------------------------------------------------------------- host buffers
def test_process_host_preserves_uncovered_bytes_and_allocates_nothing_when_steady(vctx):
    """ohgpu_dsd_process_host: host arrays in and out, destination bytes between and around the outputs left as they were, the
    call counted in ohgpu_host_transfer_stats, and from the second call on no device allocation."""
    b = Batch(8000, src_lead=2, dst_lead=7)
    b.add(DSF, 6, 2, 2053, sres=0, dres=0, gap=3).add(DFF, 2, 0, 45, gap=5).add(RAW, 8, 4, 64, sres=0, dres=0, gap=16)
    b.add(PASS, 6, 2, 16, gap=1).add(DFF, 8, 4, 12, gap=9, silence=True).empty()
    descs, src, dst_bytes = b.finish(dst_tail=11)
    want = expected(descs, src, dst_bytes)
    before = vctx.host_transfer_stats()
    allocs = []
    for _ in range(4):
        dst = np.full(dst_bytes, FILL, dtype=np.uint8)
        vctx.dsd_process_host(descs, src, dst)
        bad = np.nonzero(dst != want)[0]
        assert bad.size == 0, f"{bad.size} differing bytes, first at {bad[:6].tolist()}"
        allocs.append(vctx.device_allocations())
    after = vctx.host_transfer_stats()
    assert after["calls"] == before["calls"] + 4 and after["src_calls"] == before["src_calls"]
    assert after["h2d_bytes"] == before["h2d_bytes"] + 4 * src.size and after["d2h_bytes"] > before["d2h_bytes"]
    assert allocs[1] == allocs[2] == allocs[3], allocs
    with pytest.raises(capi.OhGpuError) as e:                               # one byte short: refused, the destination untouched
        dst = np.full(dst_bytes - 12, FILL, dtype=np.uint8)
        vctx.dsd_process_host(descs, src, dst)
    assert e.value.code == capi.ERR_BOUNDS and (dst == FILL).all()
