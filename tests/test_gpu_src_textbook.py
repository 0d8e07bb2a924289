"""Every resampler plan kind on the GPU against the textbook model (tests/src_textbook.py) -- not the oracle, whose polyphase
indexing the kernels share.  A matrix of cells, each first asserting the kernel its batch runs on (ctx.src_kernel_name), then
comparing the GPU's bytes with the model's for four input classes: impulses (the expected outputs read straight from the table),
rounding ties, rails, seeded noise in ragged unsorted messages; and, where the cell's filter is in tests/golden/src_textbook.json,
the fixture's two inputs against its hashes (check_cell is the cell's body; tests/test_gpu_src_ratios.py runs it over the rate ratios,
with tables steered to the block kernel a cell is meant for).  Then the same batch for three periods on every plan kind (run,
ohgpu_src_batch_advance, ohgpu_src_batch_set_ramps, a refused set_ramps), the filters' audio in the frequency domain (no model),
and the pulled path at phase-aligned steps against the same operation."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import src_pull_model as PM
import src_textbook as TB
from ohpipeline_amd import capi

from src_cases import (LE, BE, kMax, RAMPS, FILL, F44, F96, F48, F32, WG, LEAN, BLOCK, V1, S24, WG_LAYOUTS, LEAN_ONLY_LAYOUTS, BLOCK_LAYOUTS, CELLS, layout_id, cell_id,
                       phase_sum, LEAN_SUMS, ROUND1_SUMS, steered, Filter, Batch, model, assert_same, run, block_of, full_scale, one_stream)   # noqa: F401

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "src_textbook.json")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ramp_table():
    return capi.ramp_table()


@pytest.fixture(scope="module")
def filters(ctx):
    made = {}

    def get(f):
        if f not in made:
            made[f] = Filter(ctx, *f)
        return made[f]
    yield get
    for f in made.values():
        ctx.src_destroy(f.handle)


def check_cell(ctx, flt, ramp_table, kernel, variant, lay, name):
    """One cell of a matrix: the batch runs on `kernel` under `variant`, and its bytes equal the model's for the four input classes.
    Sizes: four blocks of input (3000 frames at least) -- whole blocks, a block edge inside a message, a generic head and tail."""
    ch, sb, se, db, de, planar = lay
    L_blk, M_blk = block_of(ctx, flt, lay, variant)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lo, hi = full_scale(sb)
    msg = 220 if flt.rout == 44100 else 240
    block_plan = kernel != V1
    while not block_plan and M_blk < flt.T + 4 * ch:      # (block_of's stand-in for a plan without blocks: any whole periods will do, wide
        L_blk, M_blk = 2 * L_blk, 2 * M_blk               # enough that no output sees two of the impulses below)
    n_in = max(4 * M_blk, 3000)

    # (a) impulses: input frame 0, the first and the last input frame of block 1, the newest frame of a message's first output;
    # channel c 2c frames further in (the last frame of the block: 2c frames back), signs alternating
    # (a block shorter than a window and the channels' offsets: the last frame of block 2 instead, so that no output sees two impulses)
    first_msg = next(m for m in range(0, 1 << 30, msg) if (m * flt.M) // flt.L >= 2 * M_blk + 3 * flt.T)
    last_of = 2 if M_blk - 1 - 4 * (ch - 1) >= flt.T else 3
    sites = [(0, 1), (M_blk, 1), (last_of * M_blk - 1, -1), ((first_msg * flt.M) // flt.L, 1)]
    y = np.zeros((n_in, ch), dtype=np.int64)
    for i, (n, way) in enumerate(sites):
        for c in range(ch):
            y[n + way * 2 * c, c] = hi if (i + c) % 2 == 0 else lo
    b, n_out = one_stream(flt, lay, y, rng, msg)
    descs, src = b.descs(), b.arena()
    s24 = np.zeros((n_out, ch), dtype=np.int64)
    m = np.arange(n_out)
    for i, (n, way) in enumerate(sites):
        for c in range(ch):
            s24[:, c] += TB.impulse_response(flt.coef, flt.L, flt.M, flt.T, int(y[n + way * 2 * c, c]) << TB.source_shift(sb), n + way * 2 * c, m)
    want = np.full(b.dst, FILL, dtype=np.uint8)
    for d in descs:
        o = int(d["out_frame0"])
        piece = TB.pack(s24[o:o + int(d["n_frames"])], d, ramp_table)
        want[int(d["dst_offset"]):int(d["dst_offset"]) + piece.size] = piece
    assert np.array_equal(model(flt, descs, src, b.dst, ramp_table), want)
    got, plan = run(ctx, flt, variant, kernel, descs, src, b.dst)
    assert_same(got, want, "impulses")
    assert not block_plan or plan["block_kernel_out_frames"] > 0

    # (b) rounding ties (windows apart), both signs, one source step either side, some past the clamp
    y = rng.integers(lo, hi + 1, size=(n_in, ch))
    ties = TB.plant_ties(rng, flt.coef, flt.L, flt.M, flt.T, y, sb)
    sums = np.array([acc for acc, offset in ties.values() if offset == 0], dtype=object)
    # (a table without an odd coefficient has no tie to plant: the identity, 48 -> 48 kHz -- one coefficient of 2^28 -- sums to multiples of 2^28)
    assert (len(ties) > 20 and (sums < 0).any() and (sums > 0).any()) or not (flt.coef & 1).any()
    b, _ = one_stream(flt, lay, y, rng, msg)
    descs, src = b.descs(), b.arena()
    got, _ = run(ctx, flt, variant, kernel, descs, src, b.dst)
    assert_same(got, model(flt, descs, src, b.dst, ramp_table), "ties")

    # (c) rails: full-scale DC at each rail, then a full-scale square wave in the pass band; the outputs clamp on both sides
    y = np.empty((n_in, ch), dtype=np.int64)
    third = n_in // 3
    y[:third], y[third:2 * third] = np.where(np.arange(ch) % 2 == 0, hi, lo), np.where(np.arange(ch) % 2 == 0, lo, hi)
    y[2 * third:] = np.where((np.arange(n_in - 2 * third) // 24) % 2 == 0, hi, lo)[:, None]
    if int(flt.coef.astype(np.int64).sum()) < (flt.L << 28) * 7 // 8:
        # (a table steered down passes DC and the square wave below full scale: in the last third, windows apart, the frames of an
        # output's window at the rails by the signs of their coefficients -- sum |c| times full scale, past the clamp, either way)
        h = TB.prototype(flt.coef, flt.L, flt.T)
        m = -(-(2 * third + flt.T) * flt.L // flt.M)
        for i in range(1 << 30):
            t = m * flt.M
            n_lo, n_hi = TB.frames_read(h.size, flt.L, [t])
            if n_hi >= n_in:
                break
            n = np.arange(n_lo, n_hi + 1)
            for c in range(ch):
                y[n, c] = np.where(h[t - n * flt.L] * (1 if (i + c) % 2 == 0 else -1) >= 0, hi, lo)
            m += TB.tie_gap(flt.L, flt.M, flt.T)
    b, n_out = one_stream(flt, lay, y, rng, msg)
    descs, src = b.descs(), b.arena()
    s24 = np.concatenate([TB.resample(flt.coef, flt.L, flt.M, flt.T, y << TB.source_shift(sb), 0, m, min(msg, n_out - m))
                          for m in range(0, n_out, msg)])             # (a message at a time: the model's matrix is outputs x frames)
    # (the rails: the clamp's -- or, below them, what sum |c| lets a full-scale source reach: an identity filter, 48 -> 48 kHz, from S16)
    reach = [int(np.clip((phase_sum(flt.coef, flt.L, flt.T) * (v << TB.source_shift(sb)) + (1 << 27)) >> 28, TB.S24_MIN, TB.S24_MAX)) for v in (lo, hi)]
    assert (s24 == reach[1]).sum() > 10 and (s24 == reach[0]).sum() > 10
    got, _ = run(ctx, flt, variant, kernel, descs, src, b.dst)
    assert_same(got, model(flt, descs, src, b.dst, ramp_table), "rails")

    # (d) noise in ragged messages whose ends miss the block edges, RAMPS and ZERO_LSB32, one stream from its start and one asked
    # for from the middle (its buffer starts there), the descriptors shuffled
    b = Batch()
    first = 3 * M_blk + 11
    for f0, m, end in ((0, 0, TB.out_frames(flt.L, flt.M, n_in)),
                       (first, -(-(first + flt.T) * flt.L // flt.M) + 1, TB.out_frames(flt.L, flt.M, first + n_in))):
        s = b.add_stream(rng.integers(lo, hi + 1, size=(n_in, ch)), lay, rng, first=f0)
        i = 0
        while m < end:
            n = min((1, 5, 43, 220, 239, 241, 700)[i % 7], end - m)
            ramp = RAMPS[i % len(RAMPS)]
            b.add_msg(s, m, n, (capi.FLAG_RAMP if i % 3 else 0) | (capi.FLAG_ZERO_LSB32 if i % 4 == 1 else 0), ramp)
            m += n
            i += 1
    descs, src = b.descs(), b.arena()
    descs = descs[rng.permutation(descs.size)]
    got, plan = run(ctx, flt, variant, kernel, descs, src, b.dst)
    assert_same(got, model(flt, descs, src, b.dst, ramp_table), "ragged noise")
    assert not block_plan or (plan["block_kernel_out_frames"] > 0 and plan["generic_pieces"] > 0), plan


@pytest.mark.parametrize("cell", CELLS, ids=[cell_id(c) for c in CELLS])
def test_every_plan_kind_equals_the_model(ctx, filters, ramp_table, cell):
    kernel, variant, f, lay = cell
    flt = filters(f)
    ch, sb, se, db, de, planar = lay
    check_cell(ctx, flt, ramp_table, kernel, variant, lay, cell_id(cell))
    rng = np.random.default_rng(zlib.crc32(cell_id(cell).encode()) + 1)
    msg = 220 if flt.rout == 44100 else 240

    # the golden fixture's inputs, where the cell's filter is there and its layout carries S24 in and out
    fx = {(e["rate_in"], e["rate_out"], e["T"]): e for e in json.load(open(FIXTURE))["filters"]}
    if f in fx and ch == 2 and sb in (24, 32) and db == 24:
        for inp in fx[f]["inputs"]:
            x = TB.fixture_input(inp["kind"], flt.coef, flt.L, flt.M, flt.T)
            b, n_out = one_stream(flt, lay, x, rng, msg, ramp_every=0)
            got, _ = run(ctx, flt, variant, kernel, b.descs(), b.arena(), b.dst)
            y = PM.decode_s24(got[3:3 + n_out * 6], 2, 24, de)
            assert y[:64].tolist() == inp["first_64"], inp["kind"]
            assert hashlib.sha256(np.ascontiguousarray(y, dtype="<i4").tobytes()).hexdigest() == inp["s24_sha256"], inp["kind"]


@pytest.mark.parametrize("kernel,variant", [(WG, 0), (LEAN, 4), (V1, 1)], ids=["wg", "lean", "generic"])
def test_planar_planes_with_bits_above_the_depth(ctx, filters, ramp_table, kernel, variant):
    """OHGPU_FLAG_SRC_PLANAR32 is a14 -> a1 -> a-R in one pass, and a14 (CodecFlac::CallbackWrite) keeps the low src_bits bits of
    every TInt32 and drops the rest.  16-bit stereo planes whose upper 16 bits are noise, against the model of the composition: pack
    the planes as a14 does (tests/fmt_textbook.py), resample the packed bytes.  Bits above the depth are ignored on every kernel."""
    import fmt_textbook as FT
    lay = (2, 16, BE, 24, BE, True)
    flt = filters(F44)
    rng = np.random.default_rng(515)
    n_in = 3000
    y = rng.integers(-32768, 32768, size=(n_in, 2))
    y[:6, 0], y[:6, 1] = (-32768, 32767, -1, 0, 1, -32767), (32767, -32768, 0, -1, -2, 2)
    b, n_out = one_stream(flt, lay, y, rng, 240)
    descs, src = b.descs(), b.arena()
    off, stride = int(descs["src_offset"][0]), int(descs["src_plane_stride"][0])
    dirty = src.copy()
    for c in range(2):
        words = dirty[off + c * stride:off + c * stride + 4 * n_in].view("<u4")
        words[:] = (words & 0xFFFF) | (rng.integers(0, 1 << 16, size=n_in).astype(np.uint32) << 16)
    assert (dirty != src).sum() > n_in
    fd = {"kind": FT.FLAC_PACK, "channels": 2, "n_frames": n_in, "src_bits": 32, "dst_bits": 16, "src_offset": off, "dst_offset": 0,
          "src_plane_stride": stride, "dst_plane_stride": 0}
    (_, packed), = FT.flac_pack(fd, dirty.tobytes())
    assert FT.flac_pack(fd, src.tobytes()) == [(0, packed)]             # (in range, the planes say the same)
    packed_descs = descs.copy()
    packed_descs["flags"] &= ~np.uint8(capi.FLAG_SRC_PLANAR32)
    packed_descs["src_offset"], packed_descs["src_plane_stride"], packed_descs["src_endian"] = 0, 0, BE
    want = model(flt, packed_descs, np.frombuffer(packed, dtype=np.uint8), b.dst, ramp_table)
    assert np.array_equal(model(flt, descs, src, b.dst, ramp_table), want)
    got, _ = run(ctx, flt, variant, kernel, descs, dirty, b.dst)
    assert_same(got, want, "planes with noise above bit 15")
    got, _ = run(ctx, flt, variant, kernel, descs, src, b.dst)
    assert_same(got, want, "planes in range")


# ------------------------------------------------------------------------------------------ the same batch, three periods
# (the last three: a block whose input is shorter than its output, on either block kernel -- 24 -> 48 kHz, the table as designed and
# steered up; and one four times as long -- 192 -> 48 kHz, the plain 64-tap lean kernel)
REUSE = {"wg": (WG, 0, F44, [S24]), "lean": (LEAN, 4, F44, [S24]), "round1": (BLOCK, 0, F48, [S24]),
         "two-layouts": (WG, 0, F44, [S24, (6, 24, LE, 24, BE, False)]), "generic": (V1, 0, F44, [(2, 24, LE, 8, BE, False)]),
         "lean-24to48": (LEAN, 0, (24000, 48000, 32, 10000.0, LEAN_SUMS), [S24]),
         "round1-24to48": (BLOCK, 0, (24000, 48000, 32, 10000.0, ROUND1_SUMS), [S24]),
         "lean-192to48": (LEAN, 0, (192000, 48000, 64, 15300.0, None), [S24])}


@pytest.mark.parametrize("kind", list(REUSE))
def test_the_same_batch_for_three_periods(ctx, filters, ramp_table, kind):
    """A period of messages that starts 37 outputs into a block and ends 13 short of one (generic pieces beside the block units),
    two ramped messages in seven: (1) run; (2) ohgpu_src_batch_advance by 5 blocks, new audio in the same arena; (3)
    ohgpu_src_batch_set_ramps with new endpoints.  Every period against the model on that period's descriptors; then a refused
    set_ramps (one endpoint beyond Ramp::kMax on a message inside whole blocks) and a run that must keep the old endpoints.  A
    batch of two layouts refuses set_ramps; a batch without a block plan refuses advance and re-ramps in place."""
    kernel, variant, f, layouts = REUSE[kind]
    flt = filters(f)
    L_blk, M_blk = block_of(ctx, flt, layouts[0], variant)
    msg = 220 if flt.rout == 44100 else 240
    period_blocks = max(3, -(-2000 // L_blk))
    head, tail = 37, 13
    out_frames = period_blocks * L_blk - head - tail
    hist = M_blk + flt.T
    win = period_blocks * M_blk + hist
    rng = np.random.default_rng(7 + len(kind))
    stream_layouts = layouts + layouts[:1]
    whole = [rng.integers(full_scale(lay[1])[0], full_scale(lay[1])[1] + 1, size=((20 + 3 * period_blocks) * M_blk, lay[0]))
             for lay in stream_layouts]

    def make(first_block, pair):
        b = Batch()
        for y, lay in zip(whole, stream_layouts):
            f0 = first_block * M_blk - hist
            s = b.add_stream(y[f0:f0 + win], lay, None, first=f0)
            m, i = first_block * L_blk + head, 0
            while m < first_block * L_blk + head + out_frames:
                n = min(msg, first_block * L_blk + head + out_frames - m)
                ramped = i % 7 < 2
                b.add_msg(s, m, n, capi.FLAG_RAMP if ramped else 0, pair if ramped else (kMax, kMax))
                m += n
                i += 1
        return b.descs(), b.arena(), b.dst

    at = 3
    d1, a1, dst_bytes = make(at, (kMax, 2000))
    b = d_src = d_dst = None
    try:
        ctx.set_kernel_variant(variant)
        b = ctx.src_batch(flt.handle, d1, a1.size, dst_bytes)
        assert ctx.src_kernel_name(b) == kernel
        d_src, d_dst = ctx.upload(a1), ctx.malloc(dst_bytes)

        def period(descs, arena, what):
            ctx.memset(d_dst, FILL, dst_bytes)
            ctx.src_run(b, d_src, d_dst)
            assert_same(ctx.download(d_dst, dst_bytes), model(flt, descs, arena, dst_bytes, ramp_table), what)

        period(d1, a1, "period 1")
        last, arena = d1, a1
        if kind == "generic":
            with pytest.raises(capi.OhGpuError) as e:
                ctx.src_batch_advance(b, 5)
            assert e.value.code == capi.ERR_UNSUPPORTED
        else:
            assert ctx.src_plan(b)["block_kernel_out_frames"] > 0 and ctx.src_plan(b)["generic_pieces"] > 0
            ctx.src_batch_advance(b, 5)
            at += 5
            last, arena, _ = make(at, (kMax, 2000))
            ctx.copy_h2d(d_src, arena)
            period(last, arena, "period 2: advanced")
        new, _, _ = make(at, (100, 16000))
        if kind == "two-layouts":
            with pytest.raises(capi.OhGpuError) as e:
                ctx.src_batch_set_ramps(b, new["ramp_start"], new["ramp_end"])
            assert e.value.code == capi.ERR_UNSUPPORTED
            return
        ctx.src_batch_set_ramps(b, new["ramp_start"], new["ramp_end"])
        period(new, arena, "period 3: new ramps")
        # refused: every ramped message gets other endpoints, one of them beyond Ramp::kMax -- nothing may change
        ramped = np.nonzero(new["flags"] & capi.FLAG_RAMP)[0]
        lo, hi = new["out_frame0"].astype(np.int64), new["out_frame0"].astype(np.int64) + new["n_frames"]
        mid = [k for k in ramped if kind == "generic" or ((at + 1) * L_blk <= lo[k] and hi[k] <= (at + period_blocks - 1) * L_blk)]
        assert mid, "no ramped message inside whole blocks"
        starts = np.where(new["flags"] & capi.FLAG_RAMP, 5000, new["ramp_start"]).astype(np.uint16)
        starts[mid[len(mid) // 2]] = kMax + 1
        with pytest.raises(capi.OhGpuError) as e:
            ctx.src_batch_set_ramps(b, starts, new["ramp_end"])
        assert e.value.code == capi.ERR_INVALID
        period(new, arena, "after a refused set_ramps")
    finally:
        ctx.set_kernel_variant(0)
        if b is not None:
            ctx.batch_destroy(b)
        if d_src is not None:
            ctx.free(d_src)
            ctx.free(d_dst)


# ------------------------------------------------------------------------------------------ audio
@pytest.mark.parametrize("kernel,variant,f,tone,others", [
    (WG, 0, F44, 15000, True), (WG, 0, F44, 19500, False), (LEAN, 4, F44, 15000, True), (LEAN, 4, F44, 19500, False),
    (WG, 0, F96, 19000, True), (LEAN, 4, F96, 19000, True), (WG, 0, F96, 30000, True), (LEAN, 4, F96, 30000, True),
    (BLOCK, 0, F48, 15000, True)])
def test_tones_through_the_filters(ctx, filters, ramp_table, kernel, variant, f, tone, others):
    """2 s of a -6 dBFS tone in both channels (the second a quarter period later), S24; output frames [rate_out, 2 rate_out) through a
    rectangular window, one bin per Hz: a tone in the pass band keeps its level within 0.01 dB; nothing else (images, aliases, a
    stop-band tone) reaches -85 dB below the input tone.  (19.5 kHz at 44.1 -> 48 kHz: its image lies in the transition band by
    design, the other bins are not looked at.)"""
    flt = filters(f)
    rin, rout = flt.rin, flt.rout
    A = 10 ** (-6 / 20) * TB.S24_MAX
    n = np.arange(2 * rin)
    y = np.stack([np.round(A * np.sin(2 * np.pi * tone * n / rin + ph)) for ph in (0.0, np.pi / 2)], axis=1).astype(np.int64)
    b, n_out = one_stream(flt, S24, y, None, 220 if rout == 44100 else 240, ramp_every=0)
    assert n_out == 2 * rout
    got, _ = run(ctx, flt, variant, kernel, b.descs(), b.arena(), b.dst)
    out = PM.decode_s24(got[3:3 + n_out * 6], 2, 24, BE)[rout:2 * rout].astype(np.float64)
    for c in range(2):
        amp = 2 * np.abs(np.fft.rfft(out[:, c])) / rout
        if tone < min(rin, rout) / 2:
            gain = 20 * np.log10(amp[tone] / A)
            assert abs(gain) <= 0.01, (c, gain)
            amp[tone] = 0
        if others:
            worst = int(np.argmax(amp))
            assert 20 * np.log10(amp[worst] / A) <= -85, (c, worst, 20 * np.log10(amp[worst] / A))


# ------------------------------------------------------------------------------------------ the pulled path
@pytest.mark.parametrize("s", [8, 6])
@pytest.mark.parametrize("T", [32, 64])
@pytest.mark.parametrize("ch", [2, 6])
def test_pulled_phase_aligned_steps_equal_the_textbook_operation(ctx, ramp_table, s, T, ch):
    """Steps a * 2^(32 - s) with a = P, about 0.92 P and 2 P, positions on the phase grid past T frames in: the pulled kernel's bytes
    equal upfirdn's operation (up = 2^s, down = a, on the table's prototype) through the same pack -- tables of 2^8 and 2^6 phases,
    the stereo and the any-channel instantiation, ramps and ZERO_LSB32 on some messages."""
    table = capi.src_pull_design(44100, 48000, T, s, 8.0 if T == 32 else 9.0, 20000.0, 0.001)
    flt = ctx.src_pull_create(T, s, table)
    P, unit = 1 << s, 1 << (32 - s)
    rng = np.random.default_rng(s * 100 + T + ch)
    n_in = 4000
    x = rng.integers(TB.S24_MIN, TB.S24_MAX + 1, size=(n_in, ch))
    x[1000:1400] = TB.S24_MAX
    x[1400:1800] = TB.S24_MIN
    src = TB.encode(x, 24, LE)
    descs, want, dp = [], [], 0
    for i, a in enumerate((P, (P * 92) // 100, 2 * P)):
        pos, frac = T + 5 + 7 * i, int(rng.integers(0, P)) * unit
        for k, n in enumerate((240, 1, 77, 240, 300)):
            d = np.zeros(1, dtype=capi.SRC_PULL_MSG_DESC)[0]
            d["src_frames"], d["pos_frame"], d["pos_frac"], d["step"], d["n_frames"] = n_in, pos, frac, a * unit, n
            d["dst_offset"], d["attenuation"] = dp, 256
            d["channels"], d["src_bits"], d["src_endian"], d["dst_bits"], d["dst_endian"] = ch, 24, LE, 24, BE
            d["flags"] = (capi.FLAG_RAMP if k % 2 else 0) | (capi.FLAG_ZERO_LSB32 if k == 3 else 0)
            d["ramp_start"], d["ramp_end"] = RAMPS[(i + k) % len(RAMPS)]
            y = TB.resample_pulled(table, s, x, 0, pos, frac, a * unit, n)
            piece = PM.pack(y, 24, BE, int(d["flags"]), RAMPS[(i + k) % len(RAMPS)], ramp_table)
            assert np.array_equal(piece, PM.message_bytes(table, s, d, src, ramp_table))
            descs.append(d)
            want.append(piece)
            dp += piece.size
            pos, frac = PM.advance(pos, frac, a * unit, n)
    assert pos < n_in
    descs = np.array(descs, dtype=capi.SRC_PULL_MSG_DESC)
    d_src, d_dst = ctx.upload(src), ctx.malloc(dp)
    b = ctx.src_pull_batch(flt, descs, src.size, dp)
    try:
        ctx.memset(d_dst, FILL, dp)
        ctx.src_pull_run(b, d_src, d_dst)
        assert_same(ctx.download(d_dst, dp), np.concatenate(want), f"pulled s={s} T={T} ch={ch}")
    finally:
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        ctx.src_pull_destroy(flt)
