"""The layout-changing processors on the device (ohgpu_fmt_batch_create / ohgpu_fmt_batch_run: a11 unpack-to-planes, a13 Songcast
pack, a14 FLAC pack) against tests/fmt_textbook.py, on each of the planner's five routes (csrc/fmt_line_kernel.hip, plan_fmt_line):

    "pcm_line"                  1  uniform mono / stereo a13 of >= 16 bits, rewritten as PCM messages for pcm_line_kernel
    "ohm_wide"                  2  a13 of streams that all have more than two channels, on ohm_wide_kernel
    "unpack_stereo_kernel<N>"   3  uniform stereo a11 of N = 2, 3, 4 source bytes, register only
    "flac_stereo_kernel<N>"     3  uniform stereo a14 to N = 1, 2, 3 destination bytes, register only
    "fmt_line_kernel"           4  everything else the planner can cut into staged chunks
    "fmt_kernel_v1"             5  what it gives up on (and every batch under kernel variant 1)

Conventions: both arenas allocated to the byte, the destination pre-filled with 0xA5, the WHOLE destination arena compared with
the model's (gaps between outputs, bytes between a11's planes and past each plane's last frame included), zero differing bytes.
Every check first asks ohgpu_batch_paths_info which route the batch was planned onto and asserts it by the names above, then
compares; every test that runs a kernel runs under the tuned kernels and under variant 1 (`vctx`), each against the model (only
test_validation_refusals, which runs none, takes the plain context).  Plane values of a14 are
drawn over the whole TInt32 range, so the truncation of what lies above the depth is exercised wherever a14 is.

The staged kernel's chunk rule, recomputed here (frames_per_chunk): a chunk holds at most 512 destination subsamples, and its
source bytes must fit the 2304-byte staging buffer less 32 bytes of alignment slack -- a11 and a13 stage frames_per_chunk + 4
whole frames of channels * bytes, a14 one run of 4 * frames + 64 bytes per channel.  The chunk counts the planner reports are
asserted against it.

Mutations of the library these tests were seen to fail under on an MI355X (one build each, never committed; all of them produce
wrong bytes inside the arenas only):
  * unpack_stereo_kernel, the tail's `f0 + lane / 8` replaced by `f0 + lane / 16`: 7 failures -- test_unpack_stereo_at_every_alignment
    and test_unpack_stereo_record_loop_and_arena_ends at 16, 24 and 32 bits, test_arenas_exact_and_one_byte_short (tuned).
  * unpack_stereo_kernel, `if (c == 0) o0[f] = w; else o1[f] = w;` with `c == 1` (whole groups land in the other plane): the same 7.
  * flac_stereo_kernel, the odd last frame's `xv >> (8 * (DB - 1 - b))` replaced by `xv >> (8 * b)`: 5 failures --
    test_flac_stereo_at_every_alignment and test_flac_stereo_record_loop_and_arena_ends to 16 and 24 bits (one byte has no order),
    test_arenas_exact_and_one_byte_short (tuned).
  * flac_stereo_kernel, the carry into the next word `v >> (32 - 8 * (o & 3))` replaced by `v >> (24 - 8 * (o & 3))`: 3 failures --
    the same two tests to 24 bits (the only depth whose subsamples straddle a word) and the exact arenas (tuned).
  * fmt_line_kernel, the `db == 3` selector for o == 1, 0x05040201 replaced by 0x05040200: 8 failures --
    test_staged_kernel_around_every_chunk_cut and test_staged_kernel_at_every_alignment for a13 and a14, test_staged_kernel_named_cases,
    test_staged_kernel_every_wave_stages_twice, test_golden_fixture_batches, test_arenas_exact_and_one_byte_short (tuned).
  * fmt_line_kernel, the `db == 4 && dhead != 0` branch's `alignbyte(subsample(qa + 1), v, o)` with 0 for o: 6 failures -- the chunk
    cut and alignment tests for a11, named cases, every_wave_stages_twice, the fixture's batches, the exact arenas (tuned).
  * fmt_line_kernel, the `db == 2 && (dhead & 1)` branch likewise: 7 failures -- as for the `db == 3` selector, less the exact arenas.
  * plan_fmt_line, a13's `map_c` for ten channels 8 replaced by 7: 4 failures -- the chunk cut and alignment tests for a13, named cases
    ("ten next to nine"), the fixture's batches (tuned).
  * plan_fmt_line, a later a13 chunk's `dst_off` one frame early (`f0 - (f0 ? 1 : 0)`): the same 4.
  * plan_fmt_line, a11's `k.map_c = p` replaced by `p ? p - 1 : 0` (a plane gets its neighbour's channel): 6 failures -- as for the
    `db == 4` branch.
  * fmt_kernel_v1, a13's `first = ch < 10 ? 0 : 8` with `ch < 11`: 9 failures, all under variant 1 -- the chunk cut and alignment tests
    for a13, named cases, test_wide_sender_packs at all four widths, the fixture's batches, the exact arenas (the ten-channel case).
  * fmt_kernel_v1, a14's `v >> (8 * (db - 1 - b))` replaced by `v >> (8 * b)`: 14 failures -- test_batches_the_planner_gives_up_on, the
    fixture's batches and the exact arenas (their three-channel case with planes 36 bytes apart) under both variants, and under
    variant 1 every a14 test to 16 and 24 bits.
(A mutation of a tuned kernel left every variant-1 case green, and a mutation of fmt_kernel_v1 every tuned case that the planner does
not itself hand to fmt_kernel_v1, as it should be: each is held to the model, not to the other.)
"""
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest

import fmt_textbook as FT
from device_shape import compute_units
from ohpipeline_amd import capi
from fmt_cases import (A11, A13, A14, FILL, PCM_LINE, OHM_WIDE, FMT_LINE, FMT_V1, STEREO, INT32_MIN, INT32_MAX, EDGES, frames_per_chunk, Batch,
                       route_of, expected)   # noqa: F401  (the builders: shared with the far-offset tests)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "fmt_textbook.json")
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
    b = ctx.fmt_batch(descs, src.size, dst_bytes)
    try:
        paths, info = ctx.batch_paths(b), ctx.batch_info(b)
        ctx.fmt_run(b, d_src, d_dst)
        out = ctx.download(d_dst, dst_bytes) if dst_bytes else np.zeros(0, np.uint8)
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
    return out, paths, info


def check(ctx, batch, route, what, totals=False, records=None):
    """Asserts the route (and the number of records / chunks, when given), then zero differing bytes over the whole arena."""
    descs, src, dst_bytes = batch
    got, paths, info = run(ctx, descs, src, dst_bytes)
    assert route_of(paths) == route, (what, paths)
    if records is not None:
        key = {PCM_LINE: "group_chunks", OHM_WIDE: "fmt_wide_records", FMT_LINE: "fmt_staged_chunks"}.get(route, "fmt_stereo_records")
        assert paths[key] == records, (what, records, paths)
    if totals:
        assert info == FT.totals(descs, src.tobytes()), what
    want = expected(descs, src, dst_bytes)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} differing bytes, first at {bad[:6].tolist()} ({route}, {paths})"
    return paths


# ---------------------------------------------------------------- route 3: the register-only stereo kernels
@pytest.mark.parametrize("sb", [2, 3, 4])
def test_unpack_stereo_at_every_alignment(vctx, sb):
    """a11, uniform stereo, the whole cross: 1-9 frames (groups of four and every tail) x every source residue mod 16 x every
    destination residue mod 4 x plane strides of 4 * frames, + 4 and + 5 (an odd one: the second plane's wide stores at another
    alignment than the first's), 1728 descriptors; then 255 / 256 / 257 / 1027 frames (a wave's pass of 256) x every source residue
    x every destination residue, the stride rotating through + 0, + 4, + 5, + 7; zero-frame descriptors in between.  One batch:
    many records, one launch."""
    b, k = Batch(3100 + sb, src_lead=1, dst_lead=2), 0
    for sres, dres, extra in itertools.product(range(16), range(4), (0, 4, 5)):
        for n in range(1, 10):
            b.unpack(2, sb, n, sres, dres, extra, gap=k % 3)
            k += 1
        if dres == 0 and extra == 0:
            b.zero(A11, 2, 8 * sb)
    for sres, dres, n in itertools.product(range(16), range(4), (255, 256, 257, 1027)):
        b.unpack(2, sb, n, sres, dres, (0, 4, 5, 7)[(sres + dres + n) % 4], gap=1)
        k += 1
    assert k == 1728 + 256
    batch = b.finish(dst_tail=3)
    n_rec = int((batch[0]["n_frames"] > 0).sum())
    check(vctx, batch, STEREO[(A11, sb)], f"a11 stereo {8 * sb} bit", totals=True, records=n_rec)


@pytest.mark.parametrize("sb", [2, 3, 4])
def test_unpack_stereo_record_loop_and_arena_ends(vctx, sb):
    """More records than the launch has waves (4 * 4 * CUs: the record loop goes round), the first descriptor starting at byte 0
    of both arenas, the last ending at the last byte of both, zero-frame descriptors among them."""
    n_rec = 4 * 4 * compute_units() + 37
    b = Batch(3200 + sb)
    for k in range(n_rec):
        b.unpack(2, sb, 1 + k % 9, extra=(0, 4, 1)[k % 3], gap=0 if k in (0, n_rec - 1) else k % 2)
        if k % 1000 == 500:
            b.zero(A11, 2, 8 * sb)
    descs, src, dst_bytes = b.finish()
    assert int(descs["src_offset"][0]) == 0 and int(descs["dst_offset"][0]) == 0
    last = descs[-1]
    assert int(last["src_offset"]) + int(last["n_frames"]) * 2 * sb == src.size
    assert int(last["dst_offset"]) + int(last["dst_plane_stride"]) + 4 * int(last["n_frames"]) == dst_bytes
    check(vctx, (descs, src, dst_bytes), STEREO[(A11, sb)], f"a11 stereo {8 * sb} bit, {n_rec} records", records=n_rec)


@pytest.mark.parametrize("bits", [8, 16, 24])
def test_flac_stereo_at_every_alignment(vctx, bits):
    """a14, uniform stereo: 1, 2, 3, 127, 128, 129 frames at source offsets 0, 4, 8, 12 mod 16 x destination offsets 0-3 (the two-
    frame store, 4 / 8 / 12 bytes, at every alignment), plane strides that are multiples of 4 but not of 16; 4097 frames at each
    source offset; planes of the edge values (0, +-1, INT32_MIN / MAX, +-2^7, +-2^15, +-2^23 and their neighbours) and, everywhere
    else, of the whole TInt32 range: what lies above the depth is dropped.  Zero-frame descriptors in between."""
    def odd_stride(n, k):
        s = 4 * n + 4 * (k % 3)
        return s if s % 16 else s + 4

    b, k = Batch(3300 + bits, src_lead=4, dst_lead=1), 0
    for sres, dres, n in itertools.product((0, 4, 8, 12), range(4), (1, 2, 3, 127, 128, 129)):
        b.flac(2, bits, n, sres, dres, stride=odd_stride(n, k), gap=k % 3)
        k += 1
        if k % 24 == 0:
            b.zero(A14, 2, 32, bits)
    for sres in (0, 4, 8, 12):
        b.flac(2, bits, 4097, sres, (sres // 4 + 1) % 4, stride=odd_stride(4097, sres // 4), gap=2)
        b.flac(2, bits, len(EDGES), sres, sres // 4, stride=odd_stride(len(EDGES), 1), values=EDGES, gap=1)
    batch = b.finish(dst_tail=3)
    assert all(int(s) % 16 for s in batch[0]["src_plane_stride"][batch[0]["n_frames"] > 0])
    n_rec = int((batch[0]["n_frames"] > 0).sum())
    check(vctx, batch, STEREO[(A14, bits // 8)], f"a14 stereo to {bits} bit", totals=True, records=n_rec)


@pytest.mark.parametrize("bits", [8, 16, 24])
def test_flac_stereo_record_loop_and_arena_ends(vctx, bits):
    """More records than the launch has waves (4 * 6 * CUs), both arenas used from their first byte to their last."""
    n_rec = 4 * 6 * compute_units() + 41
    b = Batch(3400 + bits)
    for k in range(n_rec):
        n = 1 + k % 5
        b.flac(2, bits, n, stride=4 * n + 4 * (k % 2), gap=0 if k in (0, n_rec - 1) else k % 2)
    descs, src, dst_bytes = b.finish()
    last = descs[-1]
    assert int(descs["src_offset"][0]) == 0 and int(descs["dst_offset"][0]) == 0
    assert int(last["src_offset"]) + int(last["src_plane_stride"]) + 4 * int(last["n_frames"]) == src.size
    assert int(last["dst_offset"]) + int(last["n_frames"]) * 2 * bits // 8 == dst_bytes
    check(vctx, (descs, src, dst_bytes), STEREO[(A14, bits // 8)], f"a14 stereo to {bits} bit, {n_rec} records", records=n_rec)


# ---------------------------------------------------------------- route 4: the staged kernel
def _add(b, kind, ch, width, n, sres=None, dres=None, gap=0):
    """width: source bytes (a11, a13) or destination bytes (a14); a14's planes 16 bytes apart or a multiple, its source offset a
    multiple of 4."""
    if kind == A11:
        return b.unpack(ch, width, n, sres, dres, extra=(0, 4, 3)[(ch + n) % 3], gap=gap)
    if kind == A13:
        return b.sender(ch, width, n, sres, dres, gap=gap)
    return b.flac(ch, 8 * width, n, None if sres is None else sres & ~3, dres, gap=gap)


def _chunks(descs):
    """The chunks the documented rule gives: per descriptor (per plane for a11) ceil(frames / frames_per_chunk)."""
    total = 0
    for d in descs:
        n, ch, kind = int(d["n_frames"]), int(d["channels"]), int(d["kind"])
        fpc = frames_per_chunk(kind, ch, int(d["src_bits"]) // 8)
        total += (ch if kind == A11 else 1) * ((n + fpc - 1) // fpc)
    return total


@pytest.mark.parametrize("kind", [A11, A13, A14], ids=["a11", "a13", "a14"])
def test_staged_kernel_around_every_chunk_cut(vctx, kind):
    """For every (channels, width) pair the kind admits: frames_per_chunk - 1, exactly, + 1, and twice + 1 frames (the 52-frame chunks
    of ten 32-bit channels among them), the descriptors back to back at rotating offsets.  The planner's chunk count is asserted
    against the rule."""
    widths = (1, 2, 3) if kind == A14 else (1, 2, 3, 4)
    b, k = Batch(4100 + kind, src_lead=3, dst_lead=1), 0
    for ch, width in itertools.product(range(1, 11), widths):
        fpc = frames_per_chunk(kind, ch, 4 if kind == A14 else width)
        assert fpc >= 4, (kind, ch, width)
        for n in (fpc - 1, fpc, fpc + 1, 2 * fpc + 1):
            _add(b, kind, ch, width, n, sres=(5 * k) % 16, dres=k % 4, gap=k % 2)
            k += 1
    assert frames_per_chunk(A11, 10, 4) == frames_per_chunk(A13, 10, 4) == 52 and frames_per_chunk(A14, 10, 4) == 40
    batch = b.finish(dst_tail=2)
    check(vctx, batch, FMT_LINE, f"kind {kind} around the chunk cuts", totals=True, records=_chunks(batch[0]))


@pytest.mark.parametrize("kind", [A11, A13, A14], ids=["a11", "a13", "a14"])
def test_staged_kernel_at_every_alignment(vctx, kind):
    """Destination offset 0-3 x 1-8 one-channel frames at every destination width (the end falls on each of the four byte positions;
    for a11, 4 bytes wide, this is `dhead != 0`, for 2 bytes `dhead & 1`), then the source head at every residue mod 16 (a14: 0, 4,
    8, 12, planes a multiple of 16 apart) x destination offset 0-3 with channels 1-10 and the frame count rotating, 70 and 300
    frames among them."""
    widths = (1, 2, 3) if kind == A14 else (1, 2, 3, 4)
    b, k = Batch(4200 + kind, src_lead=1), 0
    for width, dres, n in itertools.product(widths, range(4), range(1, 9)):
        _add(b, kind, 1, width, n, sres=(3 * k) % 16, dres=dres, gap=1 + k % 2)
        k += 1
    counts = (1, 2, 3, 4, 5, 6, 7, 9, 70, 300)
    for width, sres, dres in itertools.product(widths, range(0, 16, 4 if kind == A14 else 1), range(4)):
        _add(b, kind, 1 + (3 * k + k // 10) % 10, width, counts[k % 10], sres=sres, dres=dres, gap=k % 3)
        k += 1
    batch = b.finish(dst_tail=1)
    assert {int(c) for c in batch[0]["channels"]} == set(range(1, 11))
    check(vctx, batch, FMT_LINE, f"kind {kind} at every alignment", records=_chunks(batch[0]))


def test_staged_kernel_named_cases(vctx):
    """The batches the planner must NOT hand to a faster route, and the channel rule: ten channels next to nine (channels 8 and 9
    against 0 and 1; a stereo stream beside them keeps the batch off the wide-stream kernel); mono and stereo a13 in one batch; 8-bit stereo a13; 8-bit stereo a11; stereo a11 of two depths; stereo a14 to
    two depths; a mix of all three kinds with the first descriptor starting at byte 0 and the last ending at the last byte of both
    arenas."""
    cases = {
        "ten next to nine": Batch(4301, 2, 1).sender(10, 2, 65, dres=1).sender(9, 2, 65, gap=1).sender(10, 4, 53).sender(9, 3, 7, gap=2)
                                             .sender(10, 1, 230).sender(10, 3, 1).sender(2, 2, 5, gap=1),
        "mono and stereo a13": Batch(4302, 1, 3).sender(1, 2, 300).sender(2, 2, 300).sender(1, 3, 513, gap=1).sender(2, 4, 257).sender(1, 4, 5),
        "8-bit stereo a13": Batch(4303, 5, 1).sender(2, 1, 255).sender(2, 1, 1, gap=1).sender(2, 1, 258),
        "8-bit stereo a11": Batch(4304, 7, 2).unpack(2, 1, 255, extra=4).unpack(2, 1, 3, gap=1).unpack(2, 1, 513, extra=1),
        "stereo a11 of two depths": Batch(4305, 1, 1).unpack(2, 2, 257).unpack(2, 3, 257, gap=3, extra=4),
        "stereo a14 to two depths": Batch(4306, 0, 3).flac(2, 16, 129).flac(2, 24, 129, gap=1),
        "all kinds, arenas to the byte": Batch(4307).unpack(3, 3, 100).sender(6, 3, 77, gap=1).flac(5, 24, 63, gap=2)
                                                    .flac(1, 8, 33, stride=4 * 33, gap=1).unpack(1, 2, 9, gap=1).sender(2, 4, 64),
    }
    for what, b in cases.items():
        descs, src, dst_bytes = b.finish()
        if what.startswith("all kinds"):
            last = descs[-1]
            assert int(descs["src_offset"][0]) == 0 and int(descs["dst_offset"][0]) == 0
            assert int(last["src_offset"]) + 64 * 2 * 4 == src.size and int(last["dst_offset"]) + 64 * 2 * 3 == dst_bytes
        check(vctx, (descs, src, dst_bytes), FMT_LINE, what, totals=True, records=_chunks(descs))


def test_staged_kernel_every_wave_stages_twice(vctx):
    """More than twice 4 * 8 * CUs chunks of one to three frames, all kinds and 1-4 channels: the launch holds 4 * 8 * CUs waves, so
    every wave's staging buffer is used, fenced and used again by a chunk of another kind and shape."""
    want_chunks = 2 * 4 * 8 * compute_units() + 129
    b, k, chunks = Batch(4400, 1, 1), 0, 0
    while chunks < want_chunks:
        kind, ch, width, n = (A11, A13, A14)[k % 3], 1 + (k // 3) % 4, 1 + (k // 12) % 3, 1 + (k // 7) % 3
        _add(b, kind, ch, width, n, dres=k % 4 if k % 5 == 0 else None)
        chunks += ch if kind == A11 else 1
        k += 1
    batch = b.finish(dst_tail=1)
    assert _chunks(batch[0]) == chunks > 2 * 4 * 8 * compute_units()
    check(vctx, batch, FMT_LINE, f"{chunks} small chunks", records=chunks)


# ---------------------------------------------------------------- routes 1, 2 and 5
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("sb", [2, 3, 4])
def test_narrow_sender_packs_as_pcm_messages(vctx, ch, sb):
    """Route 1: uniform mono / stereo a13 of 16 / 24 / 32 bits, one frame to several rounds of 256, odd source and destination
    offsets, the last descriptor ending with the source arena."""
    b = Batch(5100 + 10 * ch + sb, src_lead=1, dst_lead=1)
    for k, n in enumerate((1, 2, 3, 4, 5, 255, 256, 257, 700, 1025, 7, 513)):
        b.sender(ch, sb, n, sres=(7 * k + 1) % 16, dres=(k + 1) % 4, gap=k % 3)
        if k == 4:
            b.zero(A13, ch, 8 * sb)
    descs, src, dst_bytes = b.finish(dst_tail=2)
    assert int(descs["src_offset"][-1]) + 513 * ch * sb == src.size
    check(vctx, (descs, src, dst_bytes), PCM_LINE, f"a13 {ch} ch {8 * sb} bit", totals=True)


@pytest.mark.parametrize("sb", [1, 2, 3, 4])
def test_wide_sender_packs(vctx, sb):
    """Route 2: a13 of streams of 3-10 channels at every width, one frame to several rounds of 256, odd offsets, a ten-channel
    stream next to a nine-channel one, the last descriptor ending with the source arena."""
    b = Batch(5200 + sb, src_lead=3, dst_lead=1)
    shapes = [(3, 1), (6, 240), (8, 241), (10, 33), (9, 33), (4, 1000), (5, 2), (7, 513), (6, 3), (10, 257), (3, 77), (8, 255), (9, 256), (10, 1)]
    for k, (ch, n) in enumerate(shapes):
        b.sender(ch, sb, n, sres=(5 * k + 3) % 16, dres=k % 4, gap=k % 3)
        if k == 6:
            b.zero(A13, 5, 8 * sb)
    descs, src, dst_bytes = b.finish(dst_tail=3)
    assert int(descs["src_offset"][-1]) + 10 * sb == src.size
    check(vctx, (descs, src, dst_bytes), OHM_WIDE, f"a13 wide {8 * sb} bit", totals=True, records=len(shapes))


def test_batches_the_planner_gives_up_on(vctx):
    """Route 5: a14 of three channels whose planes are 4 * frames + 4 bytes apart (not a multiple of 16) inside a mixed batch, and
    alone; every count of ohgpu_batch_paths zero; the generic kernel serves the batch under both variants."""
    mixed = Batch(5300, 2, 1).unpack(3, 3, 100, extra=4).sender(6, 2, 300).flac(3, 16, 65, stride=4 * 65 + 4, gap=1).sender(2, 2, 44)
    mixed = mixed.flac(2, 24, 64, gap=1).unpack(2, 2, 9).finish(dst_tail=2)
    alone = Batch(5301).flac(3, 24, 513, stride=4 * 513 + 4).finish()
    for what, batch in (("mixed", mixed), ("alone", alone)):
        paths = check(vctx, batch, FMT_V1, what, totals=True)
        assert not any(paths.values()), paths
    empty = vctx.fmt_batch(np.zeros(0, dtype=capi.FMT_DESC), 0, 0)
    try:
        assert route_of(vctx.batch_paths(empty)) == FMT_V1 and not any(vctx.batch_paths(empty).values())
        assert vctx.batch_info(empty) == {"n_msgs": 0, "in_frames": 0, "out_frames": 0, "src_bytes_touched": 0, "dst_bytes_written": 0}
        vctx.fmt_run(empty, None, None)                                 # nothing to do, nothing touched
    finally:
        vctx.batch_destroy(empty)


def test_golden_fixture_batches(vctx):
    """The seeded batches of tests/golden/fmt_textbook.json: the device's whole destination arena hashes to what the model gave
    when the fixture was written."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_fmt_textbook_fixtures as G
    finally:
        sys.path.pop(0)
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["fill"] == FILL and len(fx["batches"]) == 3
    for entry in fx["batches"]:
        rows, src, dst_bytes = G.batches()[entry["name"]]
        descs = np.zeros(len(rows), dtype=capi.FMT_DESC)
        for i, r in enumerate(rows):
            for key, v in r.items():
                descs[key][i] = v
        src = np.frombuffer(src, dtype=np.uint8)
        assert hashlib.sha256(src.tobytes()).hexdigest() == entry["src_sha256"] and dst_bytes == entry["dst_bytes"]
        gives_up = any(r["kind"] == A14 and r["channels"] > 1 and r["src_plane_stride"] % 16 for r in rows)
        assert gives_up == (entry["name"] == "mixed_c")
        got, paths, _ = run(vctx, descs, src, dst_bytes)
        assert route_of(paths) == (FMT_V1 if gives_up else FMT_LINE), (entry["name"], paths)
        assert hashlib.sha256(got.tobytes()).hexdigest() == entry["dst_sha256"], entry["name"]
        check(vctx, (descs, src, dst_bytes), FMT_V1 if gives_up else FMT_LINE, entry["name"])


# ---------------------------------------------------------------- validation
def _one(kind, ch, n, sbits, dbits=0, so=0, do=0, sstride=0, dstride=0):
    return np.array([(so, do, sstride, dstride, n, kind, ch, sbits, dbits, [0] * 8)], dtype=capi.FMT_DESC)


def _refused(ctx, descs, src_bytes, dst_bytes, code):
    with pytest.raises(capi.OhGpuError) as e:
        ctx.batch_destroy(ctx.fmt_batch(descs, src_bytes, dst_bytes))
    assert e.value.code == code, (code, str(e.value))


def test_validation_refusals(ctx):
    """ohgpu_fmt_batch_create's checks, by error code (no kernel runs here, so the kernel variant does not matter): channels 0 and
    11; source widths 0, 12, 40; an unknown kind; a14 to 32 bits (unsupported, as in the reference) and from anything but 32, at a
    source offset or plane stride that is not a multiple of 4; a11 planes that overlap."""
    big = 1 << 16
    for kind in (A11, A13, A14):
        for ch in (0, 11):
            _refused(ctx, _one(kind, ch, 4, 32 if kind == A14 else 16, 16, sstride=16, dstride=16), big, big, capi.ERR_INVALID)
    for kind in (A11, A13):
        for sbits in (0, 12, 40):
            _refused(ctx, _one(kind, 2, 4, sbits, dstride=16), big, big, capi.ERR_INVALID)
    for kind in (0, 4, 255):
        _refused(ctx, _one(kind, 2, 4, 16, 16, sstride=16, dstride=16), big, big, capi.ERR_INVALID)
    _refused(ctx, _one(A14, 2, 4, 32, 32, sstride=16), big, big, capi.ERR_UNSUPPORTED)
    for dbits in (0, 12, 20, 40):
        _refused(ctx, _one(A14, 2, 4, 32, dbits, sstride=16), big, big, capi.ERR_UNSUPPORTED)
    for sbits in (8, 16, 24, 0):
        _refused(ctx, _one(A14, 2, 4, sbits, 16, sstride=16), big, big, capi.ERR_INVALID)
    for so, stride in ((1, 16), (2, 16), (3, 16), (0, 17), (0, 18), (4, 30)):
        _refused(ctx, _one(A14, 2, 4, 32, 16, so=so, sstride=stride), big, big, capi.ERR_INVALID)
    for stride in (0, 4, 15):                                           # a11: four frames need 16 bytes per plane
        _refused(ctx, _one(A11, 2, 4, 16, dstride=stride), big, big, capi.ERR_INVALID)


# (one descriptor, the source arena's bytes, the destination arena's bytes, the route it is planned onto)
EXACT = [(_one(A11, 3, 5, 24, so=7, do=3, dstride=23), 7 + 5 * 3 * 3, 3 + 2 * 23 + 20, FMT_LINE),
         (_one(A11, 2, 6, 16, so=3, do=1, dstride=29), 3 + 6 * 2 * 2, 1 + 29 + 24, "unpack_stereo_kernel<2>"),
         (_one(A11, 2, 7, 24, so=1, do=2, dstride=28), 1 + 7 * 2 * 3, 2 + 28 + 28, "unpack_stereo_kernel<3>"),
         (_one(A13, 10, 6, 32, so=5, do=1), 5 + 6 * 10 * 4, 1 + 6 * 2 * 3, OHM_WIDE),
         (_one(A13, 1, 6, 16, so=5, do=1), 5 + 6 * 2, 1 + 6 * 2, PCM_LINE),
         (_one(A13, 2, 5, 8, so=2, do=3), 2 + 5 * 2, 3 + 5 * 2, FMT_LINE),
         (_one(A14, 3, 7, 32, 24, so=8, do=2, sstride=32), 8 + 2 * 32 + 28, 2 + 7 * 3 * 3, FMT_LINE),
         (_one(A14, 2, 7, 32, 16, so=4, do=1, sstride=28), 4 + 28 + 28, 1 + 7 * 2 * 2, "flac_stereo_kernel<2>"),
         (_one(A14, 2, 5, 32, 24, so=12, do=3, sstride=20), 12 + 20 + 20, 3 + 5 * 2 * 3, "flac_stereo_kernel<3>"),
         (_one(A14, 3, 7, 32, 16, so=4, do=1, sstride=32 + 4), 4 + 2 * 36 + 28, 1 + 7 * 3 * 2, FMT_V1)]


def test_arenas_exact_and_one_byte_short(vctx):
    """One descriptor at offsets that are not zero, on every route: each arena one byte short is refused as out of bounds; exact
    is accepted, planned onto the route named, and right to the last byte under both kernel variants.  Then descriptors of no
    frames with offsets beyond the arenas: accepted, no route's count set, nothing written."""
    rng = np.random.default_rng(6000)
    for descs, src_bytes, dst_bytes, route in EXACT:
        _refused(vctx, descs, src_bytes - 1, dst_bytes, capi.ERR_BOUNDS)
        _refused(vctx, descs, src_bytes, dst_bytes - 1, capi.ERR_BOUNDS)
        src = rng.integers(0, 256, size=src_bytes, dtype=np.uint8)
        check(vctx, (descs, src, dst_bytes), route, f"exact arenas, {route}", totals=True, records=None if route in (FMT_V1, PCM_LINE) else 1 if route != FMT_LINE else _chunks(descs))
    for kind, ch, sbits, dbits in ((A11, 2, 16, 0), (A11, 5, 8, 0), (A13, 2, 24, 0), (A13, 7, 16, 0), (A14, 2, 32, 16), (A14, 4, 32, 8)):
        descs = _one(kind, ch, 0, sbits, dbits, so=1 << 50, do=(1 << 50) + 1, sstride=1 << 40, dstride=0)
        got, paths, info = run(vctx, descs, np.zeros(0, np.uint8), 8)
        assert route_of(paths) == FMT_V1 and not any(paths.values()), paths
        assert (got == FILL).all()
        assert info == {"n_msgs": 1, "in_frames": 0, "out_frames": 0, "src_bytes_touched": 0, "dst_bytes_written": 0}
