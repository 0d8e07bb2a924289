"""Arena offsets of 2^31 and more, on the device.  Every test lays a family's small case twice into one batch -- copy 0 near the
arenas' start, copy 1 across byte 2^31, across byte 2^32 or beyond it -- inside the two far blocks of tests/far_cases.py, runs it
once, and compares windows: both copies' destination bytes against the family's textbook model of the near layout (zero differing
bytes), the guards either side of them and every alias window (where a truncated offset would have landed) against the fill.  Where
a family can say which kernel or path a batch was planned onto, that is asserted first.  How the placements, the lead-in and the
aliases are made, and that they are contained: tests/far_cases.py, tests/test_far_cases.py."""
import numpy as np
import pytest

import alac_cases as AC
import alac_textbook as AT
import dsd_cases as DL
import dsd_file_cases as DF
import dsd_pcm_cases as DC
import dsd_textbook as DT
import far_cases as FAR
import flac_cases as FC
import flywheel_cases as FW
import flywheel_textbook as FWT
import fmt_cases as FM
import iff_cases as IC
import mp4_cases as MC
import mp4f_cases as MF
import ogg_cases as GC
import ohm_cases as OB
import ohm_rx_cases as RXC
import pcm_cases as PK
import raop_cases as RC
import src_cases as SC
import src_pull_cases as PC
import src_pull_model as PM
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arenas(ctx):
    a = FAR.FarArenas(ctx)                                   # (a failed allocation is an error here, not a skip)
    try:
        yield a
    finally:
        a.close()


@pytest.fixture(scope="module")
def ramp_table():
    return capi.ramp_table()


pairs = pytest.mark.parametrize("pair", FAR.PAIRS)


# ---------------------------------------------------------------- the block resamplers
SRC_CELLS = [(SC.WG, 0, SC.F44, SC.S24), (SC.WG, 0, SC.F96, SC.S24), (SC.WG, 0, SC.F44, (8, 24, SC.LE, 24, SC.BE, False)),
             (SC.WG, 0, SC.F44, (2, 16, SC.BE, 24, SC.BE, True)), (SC.LEAN, 4, SC.F44, SC.S24), (SC.BLOCK, 0, SC.F48, SC.S24),
             (SC.V1, 1, SC.F44, SC.S24), (SC.V1, 0, SC.F44, (2, 24, SC.LE, 8, SC.BE, False))]


@pytest.fixture(scope="module")
def filters(ctx):
    made = {}

    def get(f):
        if f not in made:
            made[f] = SC.Filter(ctx, *f)
        return made[f]
    yield get
    for f in made.values():
        ctx.src_destroy(f.handle)


@pairs
@pytest.mark.parametrize("cell", SRC_CELLS, ids=[SC.cell_id(c) for c in SRC_CELLS])
def test_src(ctx, arenas, filters, ramp_table, cell, pair):
    """One stream mid-stream (src_frame0 > 0: no unit is an edge unit) of five whole blocks and more, a ragged head and tail left
    to the generic kernel, two messages in three ramped: on the workgroup matrix kernel (packed, eight channels, half-band, planar
    S16), the lean kernel, the block fallback and the generic kernel (variant 1, and the 8-bit destination)."""
    kernel, variant, f, lay = cell
    flt = filters(f)
    L_blk, _ = SC.block_of(ctx, flt, lay, variant)
    b, _ = SC.far_stream(flt.L, flt.M, flt.T, lay, ("out", 1 << 31), False, max(6 * L_blk + 50, 3300), seed=3)
    descs, src = b.descs(), b.arena()
    want = SC.model(flt, descs, src, b.dst, ramp_table)
    twin = FAR.Twin(arenas, src, np.full(b.dst, FILL, np.uint8), pair, *FAR.ALIGN["src"], FILL)
    twin.prepare()
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.src_batch(flt.handle, FAR.twice("src", descs, twin), FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.src_kernel_name(batch) == kernel
            plan = ctx.src_plan(batch)
            assert kernel == SC.V1 or (plan["block_kernel_out_frames"] >= 2 * 4 * L_blk and plan["generic_pieces"] > 0), plan
            ctx.src_run(batch, arenas.src, arenas.dst)
            ctx.sync()
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    twin.check(want, f"src {SC.cell_id(cell)} {pair}")


# ---------------------------------------------------------------- the pulled resampler
@pairs
@pytest.mark.parametrize("T", [32, 64])
def test_src_pull(ctx, arenas, ramp_table, T, pair):
    """Stereo and five channels, 300 outputs each and a ramped message of 77 behind them."""
    table = capi.src_pull_design(44100, 48000, T, PC.S, 8.0 if T == 32 else 9.0, 20000.0, 0.001)
    flt = ctx.src_pull_create(T, PC.S, table)
    try:
        rng = np.random.default_rng(T)
        a = PC.Arena()
        step = PM.step_of(44100, 48000, PM.multiplier_of(-400))
        for ch in (2, 5):
            PC.stream(a, rng, ch, 24, PM.ENDIAN_LITTLE, 24, PM.ENDIAN_BIG, T, [step] * 2, [300, 77], 400,
                      flags_of=lambda m: PM.FLAG_RAMP if m else 0, ramps_of=lambda m: (16384, 100))
        src, descs = a.arrays()
        assert len(descs) == 4
        want = np.full(a.dst_bytes + 5, FILL, dtype=np.uint8)
        for d in descs:
            piece = PM.message_bytes(table, PC.S, d, src, ramp_table)
            want[int(d["dst_offset"]):int(d["dst_offset"]) + piece.size] = piece
        twin = FAR.Twin(arenas, src, np.full(want.size, FILL, np.uint8), pair, *FAR.ALIGN["src_pull"], FILL)
        twin.prepare()
        batch = ctx.src_pull_batch(flt, FAR.twice("src_pull", descs, twin), FAR.SPAN, FAR.SPAN)
        try:
            ctx.src_pull_run(batch, arenas.src, arenas.dst)
            ctx.sync()
        finally:
            ctx.batch_destroy(batch)
        twin.check(want, f"src_pull T={T} {pair}")
    finally:
        ctx.src_pull_destroy(flt)


# ---------------------------------------------------------------- the line kernels: pcm, fmt, dsd
variants = pytest.mark.parametrize("variant", [0, 1], ids=["tuned", "v1"])
PCM_CASES = [(24, 24, PK.PLAIN), (16, 32, PK.PLAIN), (32, 24, PK.RAMPED), (16, 16, PK.ATTENUATED), (8, 24, PK.PLAIN), (16, 8, PK.RAMPED),
             (24, 24, PK.SILENT)]                 # test_arenas_sized_to_the_byte's depth pairs, and silence


@pairs
@variants
@pytest.mark.parametrize("sbits,dbits,kind", PCM_CASES)
def test_pcm(ctx, arenas, sbits, dbits, kind, variant, pair):
    """Messages of 513, 17 and 5 subsamples at odd offsets on the path their depths and kind name: staged (16-byte pieces; 8-bit
    audio and silence), register plain, register ramped or attenuated -- the path asserted, and no other taken."""
    rng = np.random.default_rng(4800 + sbits + dbits)
    descs, src, dst_bytes = PK.pack(rng, [(513, 1, kind), (17, 1, kind), (5, 1, kind)], sbits, PK.LE, dbits, PK.BE, src_lead=1, dst_lead=3,
                                    src_gap=2, dst_gap=1)
    want = PK.expected(descs, src, dst_bytes)
    twin = FAR.Twin(arenas, src, np.full(dst_bytes, PK.FILL, np.uint8), pair, *FAR.ALIGN["pcm"], PK.FILL)
    twin.prepare()
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.pcm_batch(FAR.twice("pcm", descs, twin), FAR.SPAN, FAR.SPAN)
        try:
            paths, mine = ctx.batch_paths(batch), PK.path_of(sbits, dbits, kind)
            assert paths["line_planned"] == 1 and paths["launches"] == 1 and paths[mine] >= 2, paths
            assert all(paths[k] == 0 for k in ("staged_chunks", "group_chunks", "heavy_chunks") if k != mine), paths
            ctx.pcm_run(batch, arenas.src, arenas.dst)
            ctx.sync()
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    twin.check(want, f"pcm {sbits}->{dbits} {kind} {pair}")


FMT_CASES = {
    "a11_stereo": (lambda: FM.Batch(4801, 1, 1).unpack(2, 3, 257, sres=5, dres=1, extra=4, gap=1).unpack(2, 3, 300, extra=7, gap=2), FM.STEREO[(FM.A11, 3)]),
    "a14_stereo": (lambda: FM.Batch(4802, 0, 3).flac(2, 24, 300, sres=4, dres=1, stride=4 * 300 + 20).flac(2, 24, 129, gap=1), FM.STEREO[(FM.A14, 3)]),
    "a13_stereo": (lambda: FM.Batch(4803, 3, 1).sender(2, 3, 257, dres=1).sender(2, 3, 300, gap=1), FM.PCM_LINE),
    "a13_wide": (lambda: FM.Batch(4804, 3, 1).sender(6, 3, 257, dres=1).sender(8, 3, 300, gap=1), FM.OHM_WIDE),
    "all_kinds": (lambda: FM.Batch(4805, 2, 1).unpack(3, 3, 100, extra=4).sender(6, 3, 77, gap=1).flac(5, 24, 63, gap=2), FM.FMT_LINE),
}


@pairs
@variants
@pytest.mark.parametrize("name", list(FMT_CASES))
def test_fmt(ctx, arenas, name, variant, pair):
    """The three kinds -- planar unpack and FLAC pack with plane strides that are no multiple of 16, Songcast pack -- each on the
    route asserted: the two stereo kernels, the PCM line kernel, the wide-stream kernel, and all three kinds on the staged kernel."""
    make, route = FMT_CASES[name]
    descs, src, dst_bytes = make().finish(dst_tail=3)
    want = FM.expected(descs, src, dst_bytes)
    twin = FAR.Twin(arenas, src, np.full(dst_bytes, FM.FILL, np.uint8), pair, *FAR.ALIGN["fmt"], FM.FILL)
    twin.prepare()
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.fmt_batch(FAR.twice("fmt", descs, twin), FAR.SPAN, FAR.SPAN)
        try:
            assert FM.route_of(ctx.batch_paths(batch)) == route
            ctx.fmt_run(batch, arenas.src, arenas.dst)
            ctx.sync()
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    twin.check(want, f"fmt {name} {pair}")


@pairs
@variants
def test_dsd(ctx, arenas, variant, pair):
    """Descriptors of 513 and 17 chunks (whole sample blocks where the kind asks for them): a DSF and a DFF packer on the wide path (16-byte aligned, whole lanes), a raw packer at odd
    offsets and a short pass-through on the generic one, and a silence; the plan asserted against the documented rule."""
    b = DL.Batch(4900, src_lead=0, dst_lead=0)
    per = DT.chunks_per_block
    b.add(DL.DSF, 6, 2, 513, sres=0, dres=0).add(DL.DFF, 2, 0, 17, sres=0, dres=0, gap=3)
    b.add(DL.RAW, 6, 2, DL.whole(513, per(6, 2)), sres=5, dres=3, gap=1).add(DL.PASS, 2, 0, per(2, 0), sres=7, dres=9)
    b.add(DL.RAW, 8, 4, DL.whole(17, per(8, 4)), dres=0, silence=True)
    descs, src, dst_bytes = b.finish(dst_tail=5)
    want = DL.expected(descs, src, dst_bytes)
    twin = FAR.Twin(arenas, src, np.full(dst_bytes, DL.FILL, np.uint8), pair, *FAR.ALIGN["dsd"], DL.FILL)
    twin.prepare()
    ctx.set_kernel_variant(variant)
    try:
        both = FAR.twice("dsd", descs, twin)
        batch = ctx.dsd_batch(both, FAR.SPAN, FAR.SPAN)
        try:
            paths = ctx.dsd_batch_paths(batch)
            assert paths == DL.planned(both) and paths["wide_descs"] >= 4 and paths["generic_descs"] >= 4, paths
            ctx.dsd_run(batch, arenas.src, arenas.dst)
            ctx.sync()
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    twin.check(want, f"dsd {pair}")


# ---------------------------------------------------------------- DSD -> PCM
@pairs
@pytest.mark.parametrize("variant", [0, 1], ids=["fast", "plain"])
def test_dsd_pcm(ctx, arenas, variant, pair):
    """Two messages of 17 and 513 frames (a tile and a frame), on the table route and on variant 1's plain one."""
    key = (32, 16)
    case = DC.Batch(key, 9700, src_lead=1, dst_lead=3).add(1001, 17, (6, 2), "noise", DC.RAMPS[2]) \
        .add(7, 513, (2, 0), "noise", None, capi.ENDIAN_LITTLE, src_gap=3, dst_gap=2).finish("far offsets", dst_tail=5)
    twin = FAR.Twin(arenas, case.src, np.full(case.dst_bytes, DC.FILL, np.uint8), pair, *FAR.ALIGN["dsd_pcm"], DC.FILL)
    twin.prepare()
    filt = ctx.dsd_pcm_create(key[0], key[1], DC.coef(key))
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.dsd_pcm_batch(filt, FAR.twice("dsd_pcm", case.descs, twin), FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.dsd_pcm_batch_paths(batch) == {"fast_descs": 0 if variant else 4, "plain_descs": 4 if variant else 0, "launches": 1}
            ctx.dsd_pcm_run(batch, arenas.src, arenas.dst)
            ctx.sync()
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
        ctx.dsd_pcm_destroy(filt)
    twin.check(case.want(), f"dsd_pcm {pair}")


# ---------------------------------------------------------------- FLAC
FLAC_CASES = [("tiny_s16_stereo_44k1_b16", False), ("tiny_s16_stereo_44k1_b16", True), ("fullscale_lpc_s24_stereo_48k_b192", False)]


@pairs
@pytest.mark.parametrize("variant", [0, 1], ids=["tuned", "v1"])
@pytest.mark.parametrize("name,packed", FLAC_CASES, ids=[f"{n.split('_')[0]}-{'packed' if p else 'planes'}" for n, p in FLAC_CASES])
def test_flac(ctx, arenas, name, packed, variant, pair):
    """A whole stream, in planes and packed: both copies' results equal the model's, bytes_consumed (from src_offset) unmoved."""
    case = FC.whole(FC.fixture(name), packed)
    lay = FC.Layout([case], seed=13)
    twin = FAR.Twin(arenas, lay.src, lay.dst0, pair, *FAR.ALIGN["flac"], 0xEE)
    twin.prepare()
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.flac_batch(FAR.twice("flac", lay.descs, twin), FAR.SPAN, FAR.SPAN)
        try:
            ctx.flac_run(batch, arenas.src, arenas.dst)
            res, frames = ctx.flac_results(batch, 2), ctx.flac_frames(batch)
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    model = FC.model(case)[0]
    for r in res:
        mine = (int(r["status"]), int(r["frames"]), int(r["samples"]), int(r["first_sample_decoded"]), int(r["bytes_consumed"]),
                int(r["candidates"]), int(r["candidates_rejected"]))
        assert mine == FC.result_tuple(model), (mine, FC.result_tuple(model))
    want_frames = [(k, f.header.blocksize, place, f.pos, f.end) for k in (0, 1) for f, place in zip(model.frames, model.places)]
    assert [(int(f["stream"]), int(f["blocksize"]), int(f["first_sample"]), int(f["src_pos"]), int(f["src_end"])) for f in frames] == want_frames
    twin.check(lay.want, f"flac {name} {pair}")


# ---------------------------------------------------------------- Apple Lossless, RAOP
def twice_with_packets(family, descs, packets, twin):
    """Both copies' stream descriptors and packet rows: the far copy's streams point at the far copy's rows."""
    copies = [FAR.relocate(family, {"descs": descs, "packets": packets}, twin.src_at[k], twin.dst_at[k]) for k in (0, 1)]
    copies[1]["descs"]["first_packet"] += len(packets)
    return np.concatenate([c["descs"] for c in copies]), np.concatenate([c["packets"] for c in copies])


def check_packets(job, sres, pres):
    assert [(int(p["status"]), int(p["samples"])) for p in pres] == 2 * [tuple(w) for w in job.want_packets]
    assert [(int(r["packets_ok"]), int(r["samples"]), int(r["first_bad_status"])) for r in sres] == 2 * job.want_streams()


@pairs
@pytest.mark.parametrize("variant", [0, 1], ids=["fused", "plain"])
def test_alac(ctx, arenas, variant, pair):
    """The hand_stereo8, shifted and six16_fl256 streams, in planes, packed little- and packed big-endian (six channels in planes too): the route asserted, every
    packet's and stream's result equal for both copies."""
    hand = AC.handmade()
    six = AC.load_fixture("six16_fl256")
    job = AC.Job([(AT.parse_config(hand["hand_stereo8"][0]), hand["hand_stereo8"][1], AT.PLANAR),
                  (AT.parse_config(hand["shifted"][0]), hand["shifted"][1], AT.PACKED_LE), (six["cfg"], six["packets"], AT.PACKED_BE),
                  (six["cfg"], six["packets"][:2], AT.PLANAR)])
    descs, packets = AC.capi_tables(job)
    twin = FAR.Twin(arenas, np.frombuffer(job.src, np.uint8), np.frombuffer(job.dst0, np.uint8), pair, *FAR.ALIGN["alac"], AC.FILL)
    twin.prepare()
    ctx.set_kernel_variant(variant)
    try:
        both = twice_with_packets("alac", descs, packets, twin)
        batch = ctx.alac_batch(*both, FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.batch_paths(batch)["alac_route"] == (capi.ALAC_ROUTE_PLAIN if variant else capi.ALAC_ROUTE_FUSED)
            ctx.alac_run(batch, arenas.src, arenas.dst)
            check_packets(job, *ctx.alac_results(batch, len(both[0]), len(both[1])))
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    assert all(st == AT.OK for st, _ in job.want_packets)
    twin.check(np.frombuffer(job.want, np.uint8), f"alac {pair}")


@pairs
@pytest.mark.parametrize("variant", [0, 1], ids=["fused", "plain"])
def test_raop(ctx, arenas, variant, pair):
    """One session's first two packets decrypted and decoded into planes, and the same two decrypted alone (a plaintext stream)."""
    s = RC.sessions()[0]
    job = RC.Job([RC.stream(s["key"], s["iv"], s["payloads"][:2], AT.PLANAR, s["cfg"]), RC.stream(s["key"], s["iv"], s["payloads"][:2])])
    descs, packets = RC.capi_tables(job)
    twin = FAR.Twin(arenas, np.frombuffer(job.src, np.uint8), np.frombuffer(job.dst0, np.uint8), pair, *FAR.ALIGN["raop"], RC.FILL)
    twin.prepare()
    ctx.set_kernel_variant(variant)
    try:
        both = twice_with_packets("raop", descs, packets, twin)
        batch = ctx.raop_batch(*both, FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.batch_paths(batch)["alac_route"] == (capi.ALAC_ROUTE_PLAIN if variant else capi.ALAC_ROUTE_FUSED)
            ctx.raop_run(batch, arenas.src, arenas.dst)
            check_packets(job, *ctx.raop_results(batch, len(both[0]), len(both[1])))
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    assert job.want_packets[0][0] == AT.OK and job.want_packets[0][1] > 0
    twin.check(np.frombuffer(job.want, np.uint8), f"raop {pair}")


# ---------------------------------------------------------------- FlywheelRamper
@pairs
def test_flywheel(ctx, arenas, pair):
    """Two requests (stereo at 44.1 kHz, three channels at 96 kHz: decimation 2), the unaligned layout."""
    reqs = [FW.request("far_a", 901, 44100, 2, "noise", out_frames=100, block_frames=44),
            FW.request("far_b", 902, 96000, 3, "mixed", extra=1, out_frames=97, block_frames=96)]
    src, offs, dst_bytes = FW.layout(reqs, unaligned=True)
    descs = np.zeros(len(reqs), dtype=capi.FLYWHEEL_DESC)
    want = np.full(dst_bytes, 0xEE, dtype=np.uint8)
    for i, (r, (so, do)) in enumerate(zip(reqs, offs)):
        descs["src_offset"][i], descs["dst_offset"][i] = so, do
        for f in ("channel_bytes", "in_samples", "out_frames", "block_frames", "sample_rate", "channels"):
            descs[f][i] = r[f]
        y = np.frombuffer(FWT.flywheel_ramp(r["blob"].tobytes(), r["channel_bytes"], r["in_samples"], r["sample_rate"], r["channels"],
                                            r["out_frames"], r["block_frames"]), dtype=np.uint8)
        want[do:do + y.size] = y
    twin = FAR.Twin(arenas, src, np.full(dst_bytes, 0xEE, np.uint8), pair, *FAR.ALIGN["flywheel"], 0xEE)
    twin.prepare()
    batch = ctx.flywheel_batch(FAR.twice("flywheel", descs, twin), FAR.SPAN, FAR.SPAN)
    try:
        info = ctx.batch_info(batch)
        assert info["n_msgs"] == 4 and info["in_frames"] == 2 * sum(r["in_samples"] for r in reqs), info
        ctx.flywheel_run(batch, arenas.src, arenas.dst)
        ctx.sync()
    finally:
        ctx.batch_destroy(batch)
    twin.check(want, f"flywheel {pair}")


# ---------------------------------------------------------------- Songcast: sender and receiver
@pairs
@variants
@pytest.mark.parametrize("ch", [2, 6], ids=["narrow", "wide"])
def test_ohm(ctx, arenas, ch, variant, pair):
    """One stream, three frames (plain, ramped and silent fragments, a frame of three fragments): a stereo stream on the fused route
    (header and audio in one pass of the line kernel), six channels on the channel-selecting kernel; variant 1: the generic route."""
    w = OB.Batch(4700 + ch)
    st = w.stream(48000, 24, ch, endian=OB.LE, codec=b"FLAC", total=(1 << 40) + 5)
    w.frame(st, [(st["max_samples"], "plain")], frame_no=7, start=(1 << 33) + 1, flags=capi.OHM_FLAG_LOSSLESS | capi.OHM_FLAG_TIMESTAMPED, net=5)
    w.frame(st, [(43, "ramp")], frame_no=8, start=(1 << 33) + 241)
    w.frame(st, [(1, "plain"), (7, "ramp"), (2, "silence")], frame_no=9, start=12345, gap=1)
    src = w._src_so_far()
    tables = {"streams": np.concatenate(w.streams), "frames": np.concatenate(w.frames), "fragments": np.concatenate(w.fragments)}
    want = np.full(w.dst_bytes + 3, OB.FILL, dtype=np.uint8)
    for off, gram in w.expected:
        want[off:off + gram.size] = gram
    twin = FAR.Twin(arenas, src, np.full(want.size, OB.FILL, np.uint8), pair, *FAR.ALIGN["ohm"], OB.FILL)
    twin.prepare()
    copies = [FAR.relocate("ohm", tables, twin.src_at[k], twin.dst_at[k]) for k in (0, 1)]
    copies[1]["frames"]["stream"] += len(tables["streams"])
    copies[1]["frames"]["first_fragment"] += len(tables["fragments"])
    batch = ctx.ohm_batch(*(np.concatenate([c[name] for c in copies]) for name in ("streams", "frames", "fragments")), FAR.SPAN, FAR.SPAN)
    try:
        paths = ctx.batch_paths(batch)
        if ch == 2:
            assert paths["line_planned"] == 1 and paths["ohm_headers_fused"] == 6 == paths["prefixed_chunks"] and paths["ohm_wide_fragments"] == 0, paths
        else:
            assert paths["ohm_wide_fragments"] > 0 and paths["ohm_headers_fused"] == 0, paths
        ctx.set_kernel_variant(variant)
        ctx.ohm_run(batch, arenas.src, arenas.dst)
        ctx.sync()
    finally:
        ctx.set_kernel_variant(0)
        ctx.batch_destroy(batch)
    twin.check(want, f"ohm {ch} ch {pair}")


@pairs
def test_ohm_rx(ctx, arenas, pair):
    """The first two committed sessions as two streams: every record and stream result equal for both copies, a record's
    dst_offset (absolute in the destination arena) moved by exactly the copy's relocation, everything else unmoved."""
    job = RXC.Job([RXC.session_stream(s) for s in RXC.load_sessions()[:2]])
    assert len(job.table) > 2 and any(int(r["audio_bytes"]) for r in job.want_records) and all(int(o) for o in job.d_streams["dst_offset"])
    twin = FAR.Twin(arenas, np.frombuffer(job.src, np.uint8), np.frombuffer(job.dst0, np.uint8), pair, *FAR.ALIGN["ohm_rx"], RXC.FILL)
    twin.prepare()
    copies = [FAR.relocate("ohm_rx", {"streams": job.d_streams, "datagrams": job.d_grams}, twin.src_at[k], twin.dst_at[k]) for k in (0, 1)]
    copies[1]["streams"]["first_datagram"] += len(job.d_grams)
    streams, grams = (np.concatenate([c[name] for c in copies]) for name in ("streams", "datagrams"))
    capi.ohm_rx_batch_check(streams, grams, FAR.SPAN, FAR.SPAN)
    batch = ctx.ohm_rx_batch(streams, grams, FAR.SPAN, FAR.SPAN)
    try:
        ctx.ohm_rx_run(batch, arenas.src, arenas.dst)
        sres, recs = ctx.ohm_rx_results(batch, len(streams), len(grams))
    finally:
        ctx.batch_destroy(batch)
    n = len(job.want_records)
    for k in (0, 1):
        want = job.want_records.copy()
        placed = want["dst_offset"] != 0                               # (a datagram that put no audio out has no place: 0)
        want["dst_offset"][placed] += np.uint64(twin.dst_at[k])
        got = recs[k * n:(k + 1) * n]
        assert got.tobytes() == want.tobytes(), RXC.describe(got, want)
        got = sres[k * len(job.streams):(k + 1) * len(job.streams)]
        assert got.tobytes() == job.want_results.tobytes(), RXC.describe(got, job.want_results)
    twin.check(np.frombuffer(job.want, np.uint8), f"ohm_rx {pair}")


# ---------------------------------------------------------------- the container walks: ogg, mp4, mp4f, iff, dsd_file
def two_copies(family, descs, twin, **row_counts):
    """Both copies' stream descriptors; the far copy's rows in the batch's tables lie behind the near copy's (field=rows a copy)."""
    copies = [FAR.relocate(family, {"descs": descs}, twin.src_at[k], twin.dst_at[k])["descs"] for k in (0, 1)]
    for field, n in row_counts.items():
        copies[1][field] += n
    return np.concatenate(copies)


def moved_rows(rows, field, shift):
    """A table of the model's rows with `field`, absolute in an arena, moved by `shift` in every row a run writes (the others are
    the 0xA5 the batch's tables start as)."""
    out = rows.copy()
    blank = np.frombuffer(bytes([0xA5]) * rows.dtype.itemsize, dtype=rows.dtype)[0]
    for k in range(out.size):
        if out[k].tobytes() != blank.tobytes():
            out[field][k] += np.uint64(shift)
    return out


@pairs
def test_ogg(ctx, arenas, pair):
    """Two streams of several pages and packets (one of two interleaved serials): results and packet records -- run_pos and
    page_offset are relative to the stream's own offsets -- equal for both copies."""
    named = GC.sessions()
    job = GC.Job([named["three_pages"], named["two_serials"]])
    assert [len(m["packets"]) for m in job.models] == [3, 2] and all(m["status"] == 0 for m in job.models)
    twin = FAR.Twin(arenas, job.src, job.dst0, pair, *FAR.ALIGN["ogg"], GC.FILL)
    twin.prepare()
    descs = two_copies("ogg", job.descs, twin, packet_first=job.n_packets)
    capi.ogg_batch_check(descs, 2 * job.n_packets, FAR.SPAN, FAR.SPAN)
    batch = ctx.ogg_batch(descs, 2 * job.n_packets, FAR.SPAN, FAR.SPAN)
    try:
        ctx.ogg_run(batch, arenas.src, arenas.dst)
        results, packets = ctx.ogg_results(batch, len(descs), 2 * job.n_packets)
    finally:
        ctx.batch_destroy(batch)
    n = len(job.streams)
    for k in (0, 1):
        GC.assert_same(results[k * n:(k + 1) * n], packets[k * job.n_packets:(k + 1) * job.n_packets], job.want.tobytes(), job)
    twin.check(job.want, f"ogg {pair}")


@pairs
@pytest.mark.parametrize("variant", [0, 1], ids=["fused", "plain"])
def test_mp4(ctx, arenas, variant, pair):
    """Two files (everything in one chunk; a chunk a sample): the results' offsets are from src_offset and stay; the packet rows'
    src_offset is absolute in the source arena and moves by exactly the copy's relocation."""
    job = MC.Job([MC.stream(m) for m in list(MC.named_good().values())[:2]])
    assert all(m["status"] == 0 and len(m["rows"]) > 1 for m in job.models)
    twin = FAR.Twin(arenas, job.src, np.full(64, MC.FILL, np.uint8), pair, *FAR.ALIGN["mp4"], MC.FILL)
    twin.prepare()
    descs = two_copies("mp4", job.descs, twin, packet_first=job.n_packets)
    capi.mp4_batch_check(descs, 2 * job.n_packets, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.mp4_batch(descs, 2 * job.n_packets, FAR.SPAN)
        try:
            assert ctx.batch_paths(batch)["mp4_route"] == (capi.MP4_ROUTE_PLAIN if variant else capi.MP4_ROUTE_FUSED)
            ctx.mp4_run(batch, arenas.src)
            results, packets, samples = ctx.mp4_results(batch, len(descs), 2 * job.n_packets)
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    n, rows = len(job.streams), job.n_packets
    for k in (0, 1):
        want = moved_rows(job.want_packets, "src_offset", twin.src_at[k])
        assert results[k * n:(k + 1) * n].tobytes() == job.want_results.tobytes(), k
        assert packets[k * rows:(k + 1) * rows].tobytes() == want.tobytes(), k
        assert samples[k * rows:(k + 1) * rows].tobytes() == job.want_samples.tobytes(), k


@pairs
@pytest.mark.parametrize("variant", [0, 1], ids=["phases", "plain"])
def test_mp4f(ctx, arenas, variant, pair):
    """Two fragmented streams that gather their samples: the packet rows' src_offset and the run rows' data_offset are absolute in
    the source arena and move by exactly the relocation; every other field, and the gathered bytes, are the near copy's."""
    job = MF.Job([MF.stream(m) for m in list(MF.named_good().values())[:2]])
    assert all(m["status"] == 0 for m in job.models) and (job.want_dst != MF.FILL).sum() > 1000
    twin = FAR.Twin(arenas, job.src, np.full(job.dst_bytes, MF.FILL, np.uint8), pair, *FAR.ALIGN["mp4f"], MF.FILL)
    twin.prepare()
    descs = two_copies("mp4f", job.descs, twin, packet_first=job.n_packets, run_first=job.n_runs)
    capi.mp4f_batch_check(descs, 2 * job.n_packets, 2 * job.n_runs, FAR.SPAN, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.mp4f_batch(descs, 2 * job.n_packets, 2 * job.n_runs, FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.mp4f_paths(batch)["route"] == (capi.MP4F_ROUTE_PLAIN if variant else capi.MP4F_ROUTE_PHASES)
            ctx.mp4f_run(batch, arenas.src, arenas.dst)
            results, runs, packets, samples = ctx.mp4f_results(batch, len(descs), 2 * job.n_packets, 2 * job.n_runs)
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    n, rows, rr = len(job.streams), job.n_packets, job.n_runs
    for k in (0, 1):
        assert results[k * n:(k + 1) * n].tobytes() == job.want_results.tobytes(), k
        assert packets[k * rows:(k + 1) * rows].tobytes() == moved_rows(job.want_packets, "src_offset", twin.src_at[k]).tobytes(), k
        assert runs[k * rr:(k + 1) * rr].tobytes() == moved_rows(job.want_runs, "data_offset", twin.src_at[k]).tobytes(), k
        assert samples[k * rows:(k + 1) * rows].tobytes() == job.want_samples.tobytes(), k
    twin.check(job.want_dst, f"mp4f {pair}")


@pairs
@pytest.mark.parametrize("variant", [0, 1], ids=["fused", "plain"])
def test_iff(ctx, arenas, variant, pair):
    """Two WAV files (16-bit stereo, 8-bit mono): the results' data_offset and error_offset are from src_offset and stay."""
    job = IC.Job([IC.stream(w) for w in list(IC.named_good().values())[:2]])
    assert all(m["status"] == 0 for m in job.models)
    twin = FAR.Twin(arenas, job.src, np.full(job.dst_bytes, IC.FILL, np.uint8), pair, *FAR.ALIGN["iff"], IC.FILL)
    twin.prepare()
    descs = two_copies("iff", job.descs, twin)
    capi.iff_batch_check(descs, FAR.SPAN, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.iff_batch(descs, FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.batch_paths(batch)["iff_route"] == (capi.IFF_ROUTE_PLAIN if variant else capi.IFF_ROUTE_FUSED)
            ctx.iff_run(batch, arenas.src, arenas.dst)
            results = ctx.iff_results(batch, len(descs))
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    for k in (0, 1):
        IC.assert_same(results[k * len(job.streams):(k + 1) * len(job.streams)], job.want_dst, job, f"copy {k}")
    twin.check(job.want_dst, f"iff {pair}")


@pairs
@pytest.mark.parametrize("variant", [0, 1], ids=["fused", "plain"])
def test_dsd_file(ctx, arenas, variant, pair):
    """Two DSF files into sample blocks of six words, two pad bytes a chunk; destination offsets multiples of 16."""
    job = DF.Job([DF.stream(w, 6, 2) for w in list(DF.named_good().values())[:2]])
    assert all(m["status"] == 0 and m["bytes_written"] > 0 for m in job.models)
    twin = FAR.Twin(arenas, job.src, np.full(job.dst_bytes, DF.FILL, np.uint8), pair, *FAR.ALIGN["dsd_file"], DF.FILL)
    twin.prepare()
    descs = two_copies("dsd_file", job.descs, twin)
    capi.dsd_file_batch_check(descs, FAR.SPAN, FAR.SPAN)
    ctx.set_kernel_variant(variant)
    try:
        batch = ctx.dsd_file_batch(descs, FAR.SPAN, FAR.SPAN)
        try:
            assert ctx.batch_paths(batch)["dsd_file_route"] == (capi.DSD_FILE_ROUTE_PLAIN if variant else capi.DSD_FILE_ROUTE_FUSED)
            ctx.dsd_file_run(batch, arenas.src, arenas.dst)
            results = ctx.dsd_file_results(batch, len(descs))
        finally:
            ctx.batch_destroy(batch)
    finally:
        ctx.set_kernel_variant(0)
    for k in (0, 1):
        DF.assert_same(results[k * len(job.streams):(k + 1) * len(job.streams)], job.want_dst, job, f"copy {k}")
    twin.check(job.want_dst, f"dsd_file {pair}")

