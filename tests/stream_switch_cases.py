"""The batches of tests/test_gpu_stream_switch.py (on the device) and tests/test_stream_switch_cases.py (the tables and the models
alone, on the CPU): for each of the eight families whose batch keeps per-run device records (flac, alac, raop, ohm_rx, ogg, mp4, iff,
dsd_file)
ONE set of tables and TWO source arenas of equal size, X and Y, with what the family's textbook model says a run over each must leave:
the whole destination arena (pre-filled, with guards), the results, the packet or sample tables.  A run of the batch over X and a run
over Y on another stream share the batch's records; every stream's output differs between X and Y, so that a mix-up of the two runs
cannot produce the right bytes by accident.

Every pair is made by the family's own case module (the writers, the Job, the comparison): X and Y are two Jobs over inputs of equal
lengths, and the builder asserts that their tables came out byte for byte the same.  Two to four streams of a few hundred bytes to a
few KiB (FLAC and MPEG-4 have one longer stream each; their builders say why), at least one of them busy in every phase.  Built once
and kept.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from ohpipeline_amd import capi

FAMILIES = ("flac", "alac", "raop", "ohm_rx", "ogg", "mp4", "iff", "dsd_file")


class Pair:
    """family; src["X"], src["Y"]: the source arenas (uint8, equal sizes); dst0: the destination arena before a run (None: the
    family has none); want["X"], want["Y"]: the model's arena after a run (None likewise); ranges: (offset, bytes) of every stream's
    output in the destination arena; summary[which]: the model's results in a form that compares with ==; tables[which]: the model's
    tables as bytes (MPEG-4, which has no arena).  check(): the library's own validation of the tables, without a device.
    create(ctx) -> batch; run(ctx, batch, d_src, d_dst, stream); verify(ctx, batch, which): the results and tables the batch holds
    are the model's for `which` (waits for the last run)."""

    def __init__(self, family, src, dst0, want, ranges, summary, check, create, run, verify, tables=None):
        self.family, self.src, self.dst0, self.want, self.ranges, self.summary = family, src, dst0, want, ranges, summary
        self.check, self.create, self.run, self.verify, self.tables = check, create, run, verify, tables
        assert src["X"].size == src["Y"].size and src["X"].dtype == src["Y"].dtype == np.uint8
        for a in list(src.values()) + [dst0] + list(want.values()):
            if a is not None:
                a.setflags(write=False)


def _u8(raw):
    return np.frombuffer(bytes(raw), dtype=np.uint8).copy()


def _same_tables(*pairs):
    for x, y in pairs:
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), "X and Y must share one set of tables"


def _padded(xs, ys):
    """Two lists of packets, each pair brought to its longer one's length with zeros behind the packet's end."""
    n = [max(len(x), len(y)) for x, y in zip(xs, ys)]
    return [x + bytes(k - len(x)) for x, k in zip(xs, n)], [y + bytes(k - len(y)) for y, k in zip(ys, n)]


# ---------------------------------------------------------------- FLAC (flac_cases: the clean tiny stream beside its `flipped_bit`)
def _flac_layout(cases):
    """tests/test_gpu_flac_textbook.py's layout: ragged source offsets with junk between the ranges, every case's share of the
    destination starting as FC.pattern from its own index 0, 0xEE between the shares."""
    import flac_cases as FC
    rng = np.random.default_rng(11)
    src, dst0, want, ranges, at = bytearray(), [], [], [], 0
    descs = np.zeros(len(cases), dtype=capi.FLAC_STREAM_DESC)
    for i, c in enumerate(cases):
        src += bytes(rng.integers(0, 256, (i * 7 + 1) % 13, dtype=np.uint8)) + (b"\xff\xf8" if i % 3 == 0 else b"")
        d = descs[i]
        d["src_offset"], d["src_bytes"], d["dst_offset"] = len(src), c.src_bytes, at
        src += c.data[c.offset:c.offset + c.src_bytes]
        d["dst_plane_stride"] = 0 if c.flags & FC.PACKED_BE else c.max_samples * 4
        d["first_sample"], d["max_samples"], d["sample_rate"] = c.first_sample, c.max_samples, c.rate
        d["blocksize"], d["max_blocksize"], d["channels"], d["bits"], d["flags"] = c.blocksize, c.max_blocksize, c.channels, c.bits, c.flags
        n = FC.arena_bytes(c)
        pad = -n % 4 + 4 * (i % 2)
        dst0 += [FC.pattern(n), np.full(pad, 0xEE, dtype=np.uint8)]
        want += [FC.model(c)[1], np.full(pad, 0xEE, dtype=np.uint8)]
        ranges.append((at, n))
        at += n + pad
    src += b"\xff"
    return descs, _u8(src), np.concatenate(dst0), np.concatenate(want), ranges


def _flac():
    """Three streams: a 24-bit stream of three frames of up to 4096 samples in planes (X whole, Y with a bit flipped in frame 2:
    corrupt after two frames), the six-frame tiny stream packed (X flipped in frame 1, Y whole -- flac_cases.device_cases' `flipped_bit`
    beside the clean stream), the eight-frame mono stream (X whole, Y flipped in frame 4).  The first is 53 KiB, far more than the
    other families' streams, on purpose: a FLAC run waits on the host for its scan, so all that can still be running when the next
    run is issued is what it queues behind that wait -- the probe, a thread a frame -- and frames of 16 samples are over at once."""
    import flac_cases as FC
    long, tiny, forms = FC.fixture("s24_stereo_44k1_b4096_l8"), FC.fixture("tiny_s16_stereo_44k1_b16"), FC.fixture("forms_s16_mono_11k_b16")

    def flipped(fx, frame, packed=False):
        bad = bytearray(fx.data)
        bad[FC.frame_spans(fx.name)[frame][0] + 12] ^= 0x10
        return FC.whole(fx, packed)._replace(label=f"{fx.name}:flipped@{frame}", data=bytes(bad))

    cases = {"X": [FC.whole(long), flipped(tiny, 1, packed=True), FC.whole(forms)],
             "Y": [flipped(long, 2), FC.whole(tiny, packed=True), flipped(forms, 4)]}
    lay = {w: _flac_layout(cases[w]) for w in "XY"}
    _same_tables((lay["X"][0], lay["Y"][0]), (lay["X"][2], lay["Y"][2]))
    descs, dst0 = lay["X"][0], lay["X"][2]
    models = {w: [FC.model(c)[0] for c in cases[w]] for w in "XY"}
    summary = {w: [FC.result_tuple(r) for r in models[w]] for w in "XY"}
    frames = {w: [(i, f.header.blocksize, place + c.first_sample, f.pos, f.end) for i, (c, r) in enumerate(zip(cases[w], models[w]))
                  for f, place in zip(r.frames, r.places)] for w in "XY"}

    def verify(ctx, b, which):
        res = ctx.flac_results(b, len(descs))
        got = [(int(r["status"]), int(r["frames"]), int(r["samples"]), int(r["first_sample_decoded"]), int(r["bytes_consumed"]), int(r["candidates"]),
                int(r["candidates_rejected"])) for r in res]
        assert got == summary[which], (which, got, summary[which])
        got = [(int(f["stream"]), int(f["blocksize"]), int(f["first_sample"]), int(f["src_pos"]), int(f["src_end"])) for f in ctx.flac_frames(b)]
        assert got == frames[which], (which, got, frames[which])

    return Pair("flac", {w: lay[w][1] for w in "XY"}, dst0, {w: lay[w][3] for w in "XY"}, lay["X"][4], summary,
                check=lambda: capi.flac_batch_check(descs, lay["X"][1].size, dst0.size),
                create=lambda ctx: ctx.flac_batch(descs, lay["X"][1].size, dst0.size),
                run=lambda ctx, b, s, d, stream: ctx.flac_run(b, s, d, stream), verify=verify)


# ---------------------------------------------------------------- Apple Lossless (alac_cases.handmade) and RAOP (raop_cases.Job) in front of it
def _alac_streams():
    """-> {which: [(cfg, packets, form)]}: the ten predictor orders of a mono stream in planes (Y: the same packets one place on),
    the two shifted 24-bit pairs packed little-endian (Y: swapped), the five shift factors packed big-endian (Y: one place on, and
    a channel-coupling tag where the second packet was: corrupt from there).  Every packet of Y is as long as X's in its place."""
    import alac_cases as AC
    import alac_textbook as T
    hand = AC.handmade()
    out = {"X": [], "Y": []}
    for name, form, spoil in (("orders", T.PLANAR, None), ("shifted", T.PACKED_LE, None), ("factors", T.PACKED_BE, 1)):
        cookie, packets = hand[name]
        other = packets[1:] + packets[:1]
        if spoil is not None:
            other[spoil] = bytes([2 << 5, 0, 0, 0])               # (alac_cases.malformed's "tag_cce")
        x, y = _padded(packets, other)
        out["X"].append((T.parse_config(cookie), x, form))
        out["Y"].append((T.parse_config(cookie), y, form))
    return out


def _alac_like(family, jobs, tables_of, batch_check, create, run, results):
    import alac_textbook as T
    tables = {w: tables_of(jobs[w]) for w in "XY"}
    _same_tables((tables["X"][0], tables["Y"][0]), (tables["X"][1], tables["Y"][1]), (_u8(jobs["X"].dst0), _u8(jobs["Y"].dst0)))
    descs, packets = tables["X"]
    src = {w: _u8(jobs[w].src) for w in "XY"}
    dst0 = _u8(jobs["X"].dst0)
    summary = {w: ([tuple(p) for p in jobs[w].want_packets], jobs[w].want_streams()) for w in "XY"}
    ranges = []
    for s in jobs["X"].streams:
        cfg = s.get("cfg")
        if cfg is None or s["form"] == 4:                                 # a RAOP plaintext stream: its packets, where the source has them
            first, last = jobs["X"].table[s["first_packet"]], jobs["X"].table[s["first_packet"] + s["n_packets"] - 1]
            ranges.append((s["dst_offset"], last[0] + last[1] - first[0]))
        elif s["form"] == T.PLANAR:
            ranges.append((s["dst_offset"], cfg["channels"] * s["plane_stride"]))
        else:
            ranges.append((s["dst_offset"], s["n_packets"] * cfg["frame_length"] * cfg["channels"] * (cfg["bit_depth"] // 8)))

    def verify(ctx, b, which):
        sres, pres = results(ctx, b, len(descs), len(packets))
        got = ([(int(p["status"]), int(p["samples"])) for p in pres], [(int(s["packets_ok"]), int(s["samples"]), int(s["first_bad_status"])) for s in sres])
        assert got == summary[which], (which, got, summary[which])

    return Pair(family, src, dst0, {w: _u8(jobs[w].want) for w in "XY"}, ranges, summary,
                check=lambda: batch_check(descs, packets, src["X"].size, dst0.size),
                create=lambda ctx: create(ctx, descs, packets, src["X"].size, dst0.size), run=run, verify=verify)


def _alac():
    import alac_cases as AC
    streams = _alac_streams()
    jobs = {w: AC.Job(streams[w]) for w in "XY"}
    return _alac_like("alac", jobs, AC.capi_tables, capi.alac_batch_check, lambda ctx, *a: ctx.alac_batch(*a),
                      lambda ctx, b, s, d, stream: ctx.alac_run(b, s, d, stream), lambda ctx, *a: ctx.alac_results(*a))


def _raop():
    """Four streams under four keys: a plaintext one of five packets (0, 3, 16, 100 and 1028 bytes: a tail alone, whole blocks, more than
    a piece), and the three Apple Lossless streams of _alac_streams encrypted packet by packet with the tests' own AES
    (raop_textbook.encrypt_packet); Y: other bytes of the same lengths under the same keys."""
    import alac_cases as AC
    import raop_cases as RC
    import raop_textbook as R
    rng = AC.Lcg(97)
    keys = [(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16)) for _ in range(4)]
    inner = _alac_streams()
    jobs = {}
    for w in "XY":
        plain = [RC.rand_bytes(rng, n) for n in (100, 16, 0, 3, 1028)]
        streams = [RC.stream(keys[0][0], keys[0][1], plain)]
        for (key, iv), (cfg, packets, form) in zip(keys[1:], inner[w]):
            streams.append(RC.stream(key, iv, [R.encrypt_packet(key, iv, p) for p in packets], form, cfg))
        jobs[w] = RC.Job(streams)
    return _alac_like("raop", jobs, RC.capi_tables, capi.raop_batch_check, lambda ctx, *a: ctx.raop_batch(*a),
                      lambda ctx, b, s, d, stream: ctx.raop_run(b, s, d, stream), lambda ctx, *a: ctx.raop_results(*a))


# ---------------------------------------------------------------- the Songcast receiver (ohm_rx_cases.Job)
def _ohm_rx():
    """Three streams, interleaved in the arena.  X: frames in order; a stream with a track message and a halt; 8-bit mono frames out
    of order inside the window.  Y: datagrams of the same lengths with other audio -- a frame missing (a repair and a resend request),
    no halt, another order."""
    import ohm_rx_cases as RC
    import ohm_textbook as OT
    lengths = [(40, 8, 120, 4, 64, 16, 200, 12), (16, 32, 8, 64, 4), (1, 5, 17, 64, 3, 255, 2, 33, 9)]
    frames = {"X": [[10, 11, 12, 13, 14, 15, 16, 17], [3, 4, 5, 6, 7], [0xfffffffe, 0xffffffff, 1, 0, 2, 4, 3, 5, 6]],
              "Y": [[10, 11, 13, 14, 12, 15, 17, 18], [3, 5, 4, 6, 7], [7, 8, 9, 10, 11, 12, 13, 14, 15]]}
    jobs = {}
    for w in "XY":
        rng = RC.Lcg(41 if w == "X" else 43)
        a = [RC.audio_gram(f, rng.bytes(n)) for f, n in zip(frames[w][0], lengths[0])]
        halt = OT.FLAG_HALT if w == "X" else 0
        b = [RC.audio_gram(f, rng.bytes(n), flags=OT.FLAG_LOSSLESS | (halt if k == 2 else 0), codec=b"abc") for k, (f, n) in enumerate(zip(frames[w][1], lengths[1]))]
        b.insert(2, RC.other_gram(4, rng.bytes(10)))
        c = [RC.audio_gram(f, rng.bytes(n), depth=8, channels=1) for f, n in zip(frames[w][2], lengths[2])]
        jobs[w] = RC.Job([RC.stream(a), RC.stream(b), RC.stream(c)])
    x, y = jobs["X"], jobs["Y"]
    _same_tables((x.d_streams, y.d_streams), (x.d_grams, y.d_grams), (_u8(x.dst0), _u8(y.dst0)))
    src, dst0 = {w: _u8(jobs[w].src) for w in "XY"}, _u8(x.dst0)
    summary = {w: (jobs[w].want_results.tobytes(), jobs[w].want_records.tobytes()) for w in "XY"}

    def verify(ctx, b, which):
        job = jobs[which]
        sres, recs = ctx.ohm_rx_results(b, len(job.streams), len(job.table))
        assert recs.tobytes() == job.want_records.tobytes(), (which, RC.describe(recs, job.want_records))
        assert sres.tobytes() == job.want_results.tobytes(), (which, RC.describe(sres, job.want_results))

    return Pair("ohm_rx", src, dst0, {w: _u8(jobs[w].want) for w in "XY"}, [(s["dst_offset"], s["dst_capacity"]) for s in x.streams], summary,
                check=lambda: capi.ohm_rx_batch_check(x.d_streams, x.d_grams, src["X"].size, dst0.size),
                create=lambda ctx: ctx.ohm_rx_batch(x.d_streams, x.d_grams, src["X"].size, dst0.size),
                run=lambda ctx, b, s, d, stream: ctx.ohm_rx_run(b, s, d, stream), verify=verify)


# ---------------------------------------------------------------- Ogg pages (ogg_cases.mux, with a tail of zeros)
def _ogg():
    """Three streams.  The pair of tests/test_gpu_ogg_textbook.py's second run: five packets in pages of three segments, and other
    packets with zeros where a page should follow (sync lost); three one-segment pages with other payloads; three pages, whole in
    X and with a bit of the middle one flipped in Y.  Each stream's packet table has room for the longer of its two lists."""
    import ogg_cases as GC
    import ogg_textbook as OX
    rng = GC.Lcg(77)
    first = b"".join(GC.mux([rng.bytes(n) for n in (5, 900, 0, 300, 41)], 4, max_segments=3))
    other = bytearray(b"".join(GC.mux([rng.bytes(n) for n in (300, 41, 500, 99)], 4, max_segments=3)))
    assert len(first) > len(other) + 30
    other += bytes(len(first) - len(other) - 30) + b"OggS" + bytes(26)
    pages = {w: GC.mux([rng.bytes(100), rng.bytes(100), rng.bytes(100)], 7, max_segments=1) for w in "XY"}
    good = GC.mux([rng.bytes(60), rng.bytes(200), rng.bytes(31)], 9, max_segments=1)
    bad = bytearray(good[1])
    bad[40] ^= 0x10
    data = {"X": [(first, 4), (b"".join(pages["X"]), 7), (b"".join(good), 9)],
            "Y": [(bytes(other), 4), (b"".join(pages["Y"]), 7), (good[0] + bytes(bad) + good[2], 9)]}
    caps = [max(len(OX.demux(data[w][i][0], data[w][i][1], 0, 0, 0)["packets"]) for w in "XY") for i in range(3)]
    jobs = {w: GC.Job([GC.stream(raw, serial=serial, packet_capacity=cap) for (raw, serial), cap in zip(data[w], caps)]) for w in "XY"}
    x, y = jobs["X"], jobs["Y"]
    assert x.n_packets == y.n_packets
    _same_tables((x.descs, y.descs), (x.dst0, y.dst0))
    summary = {w: [{f: m[f] for f in GC.RESULT_FIELDS} | {"packets": [{f: p[f] for f in GC.PACKET_FIELDS} for p in m["packets"]]} for m in jobs[w].models] for w in "XY"}

    def verify(ctx, b, which):
        job = jobs[which]
        results, packets = ctx.ogg_results(b, len(job.streams), job.n_packets)
        GC.assert_same(results, packets, job.want.tobytes(), job)          # (the arena is the caller's to compare: the model's own goes in here)

    return Pair("ogg", {w: jobs[w].src.copy() for w in "XY"}, x.dst0.copy(), {w: jobs[w].want.copy() for w in "XY"},
                [(int(d["dst_offset"]), int(d["dst_capacity"])) for d in x.descs], summary,
                check=lambda: capi.ogg_batch_check(x.descs, x.n_packets, x.src.size, x.dst0.size),
                create=lambda ctx: ctx.ogg_batch(x.descs, x.n_packets, x.src.size, x.dst0.size),
                run=lambda ctx, b, s, d, stream: ctx.ogg_run(b, s, d, stream), verify=verify)


# ---------------------------------------------------------------- MPEG-4 sample tables (mp4_cases)
MP4_TILE = 1024          # kMp4Tile


def _mp4():
    """Three files; Y is X with one entry of each sample size table set above the packet limit (a refused sample: every later sample of
    its chunk moves or is refused too, and the results say which was the first) and another duration in the first run of each time
    table (other first frames in the sample table); both runs write every row they have room for.  A
    file of a tile and 40 samples in chunks of nine (two tiles: carries between them), eleven samples with an entry a chunk, and an
    Apple Lossless fixture in a 64-bit chunk offset table."""
    import mp4_cases as MC
    files = [MC.mux(MC.pattern_packets(MP4_TILE + 40, seed=11), MC.PATTERN_COOKIE, per_chunk=[9]),
             MC.mux(MC.pattern_packets(11), MC.PATTERN_COOKIE, per_chunk=[2, 3, 2, 3, 1], entry_per_chunk=True),
             MC.named_good()["co64"]]
    spoiled = [MC.patched(MC.patched(m, m.find("stsz")[1] + 12 + 4 * k, 1 << 20), m.find("stts")[1] + 12, 1000 + k) for m, k in zip(files, (30, 4, 1))]
    jobs = {"X": MC.Job([MC.stream(m) for m in files]), "Y": MC.Job([MC.stream(raw, capacity=m.n) for raw, m in zip(spoiled, files)])}
    x, y = jobs["X"], jobs["Y"]
    assert x.n_packets == y.n_packets
    _same_tables((x.descs, y.descs))
    summary = {w: jobs[w].want_results.tobytes() for w in "XY"}
    tables = {w: (jobs[w].want_packets.tobytes(), jobs[w].want_samples.tobytes()) for w in "XY"}

    def verify(ctx, b, which):
        job = jobs[which]
        results, packets, samples = ctx.mp4_results(b, len(job.streams), job.n_packets)
        MC.assert_same(results, packets, samples, job, what=which)

    return Pair("mp4", {w: jobs[w].src.copy() for w in "XY"}, None, {"X": None, "Y": None}, [], summary,
                check=lambda: capi.mp4_batch_check(x.descs, x.n_packets, x.src.size),
                create=lambda ctx: ctx.mp4_batch(x.descs, x.n_packets, x.src.size),
                run=lambda ctx, b, s, d, stream: ctx.mp4_run(b, s, stream), verify=verify, tables=tables)


# ---------------------------------------------------------------- PCM files (iff_cases)
def _iff():
    """Four files, Y's with other samples: 16-bit WAV, 24-bit AIFF behind an SSND offset, little-endian AIFC (Y: another rate in the
    same ten bytes), and a 32-bit WAV that a 24-bit destination shortens (Y: its "fmt " chunk renamed -- no format, no audio)."""
    import iff_cases as IC
    s = IC.samples
    files = {"X": [IC.wav(s(40, 2, 2, 1), 2), IC.aiff(s(13, 2, 3, 24), 2, ssnd_offset=5), IC.aiff(s(18, 2, 2, 29), 2, compression=b"sowt", name=b""),
                   IC.wav(s(19, 2, 4, 4), 2, rate=96000)],
             "Y": [IC.wav(s(40, 2, 2, 101), 2), IC.aiff(s(13, 2, 3, 124), 2, ssnd_offset=5), IC.aiff(s(18, 2, 2, 129), 2, compression=b"sowt", name=b"", rate=48000),
                   IC.wav(s(19, 2, 4, 104), 2, rate=96000)]}
    broken = files["Y"][3]
    at = broken.data.index(b"fmt ")
    streams = {w: [IC.stream(f) for f in files[w]] for w in "XY"}
    streams["Y"][3] = dict(streams["X"][3], data=IC.patched(broken, at, b"fmt_"))
    jobs = {w: IC.Job(streams[w]) for w in "XY"}
    x, y = jobs["X"], jobs["Y"]
    assert x.dst_bytes == y.dst_bytes
    _same_tables((x.descs, y.descs))
    dst0 = np.full(x.dst_bytes, IC.FILL, dtype=np.uint8)
    summary = {w: [{k: m[k] for k in IC.FIELDS} for m in jobs[w].models] for w in "XY"}

    def verify(ctx, b, which):
        job = jobs[which]
        IC.assert_same(ctx.iff_results(b, len(job.streams)), job.want_dst, job, what=which)   # (the arena is the caller's to compare)

    return Pair("iff", {w: jobs[w].src.copy() for w in "XY"}, dst0, {w: jobs[w].want_dst.copy() for w in "XY"},
                [(int(d["dst_offset"]), int(d["dst_bytes_capacity"])) for d in x.descs], summary,
                check=lambda: capi.iff_batch_check(x.descs, x.src.size, dst0.size),
                create=lambda ctx: ctx.iff_batch(x.descs, x.src.size, dst0.size),
                run=lambda ctx, b, s, d, stream: ctx.iff_run(b, s, d, stream), verify=verify)


# ---------------------------------------------------------------- DSD files (dsd_file_cases)
def _dsd_file():
    """Four files, Y's with other audio: a DSF file of 100 chunks into (W, P) = (2, 0), a DFF file behind junk chunks into (6, 2) (Y:
    another rate in the same four bytes), a DSF file of two plane pairs and 2100 chunks -- more than a piece of the conversion -- into
    (8, 4) from chunk 3 on, and a DFF file into (1, 0) (Y: its compression type is DST -- unsupported, no audio)."""
    import dsd_file_cases as DC
    import dsd_file_textbook as FX
    p = DC.planes
    between = [DC.junk(b"DIIN", 11), DC.junk(b"COMT", 1)]
    files = {"X": [FX.dsf(*p(100, 1)), FX.dff(*p(64, 2), between=between), FX.dsf(*p(2100, 3)), FX.dff(*p(33, 4))],
             "Y": [FX.dsf(*p(100, 101)), FX.dff(*p(64, 102), between=between, rate=5644800), FX.dsf(*p(2100, 103)), FX.dff(*p(33, 104), cmpr=b"DST ")]}
    formats = [dict(W=2, P=0), dict(W=6, P=2), dict(W=8, P=4, chunk_first=3), dict(W=1, P=0)]
    streams = {w: [DC.stream(f, **kw) for f, kw in zip(files[w], formats)] for w in "XY"}
    jobs = {w: DC.Job(streams[w]) for w in "XY"}
    x, y = jobs["X"], jobs["Y"]
    assert x.dst_bytes == y.dst_bytes
    _same_tables((x.descs, y.descs))
    assert [m["status"] for m in x.models] == [FX.OK] * 4 and [m["status"] for m in y.models] == [FX.OK] * 3 + [FX.UNSUPPORTED]
    dst0 = np.full(x.dst_bytes, DC.FILL, dtype=np.uint8)
    summary = {w: [{k: m[k] for k in FX.FIELDS} for m in jobs[w].models] for w in "XY"}

    def verify(ctx, b, which):
        job = jobs[which]
        DC.assert_same(ctx.dsd_file_results(b, len(job.streams)), job.want_dst, job, what=which)   # (the arena is the caller's to compare)

    return Pair("dsd_file", {w: jobs[w].src.copy() for w in "XY"}, dst0, {w: jobs[w].want_dst.copy() for w in "XY"},
                [(int(d["dst_offset"]), int(d["dst_bytes_capacity"])) for d in x.descs], summary,
                check=lambda: capi.dsd_file_batch_check(x.descs, x.src.size, dst0.size),
                create=lambda ctx: ctx.dsd_file_batch(x.descs, x.src.size, dst0.size),
                run=lambda ctx, b, s, d, stream: ctx.dsd_file_run(b, s, d, stream), verify=verify)


_BUILDERS = {"flac": _flac, "alac": _alac, "raop": _raop, "ohm_rx": _ohm_rx, "ogg": _ogg, "mp4": _mp4, "iff": _iff, "dsd_file": _dsd_file}


@functools.lru_cache(maxsize=None)
def pair(family):
    return _BUILDERS[family]()
