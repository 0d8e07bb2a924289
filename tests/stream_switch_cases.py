"""The batches of tests/test_gpu_stream_switch.py (on the device) and tests/test_stream_switch_cases.py (the tables and the models
alone, on the CPU): for each of the fifteen families whose batch keeps per-run device records (flac, alac, raop, ohm_rx, ogg, mp4, iff,
dsd_file; mp4f, cenc, cbcs, vorbis, ts, adts, raop_rx)
ONE set of tables and TWO source arenas of equal size, X and Y, with what the family's textbook model says a run over each must leave:
the whole destination arena (pre-filled, with guards), the results, the packet or sample tables.  A run of the batch over X and a run
over Y on another stream share the batch's records; every stream's output differs between X and Y, so that a mix-up of the two runs
cannot produce the right bytes by accident.

Every pair is made by the family's own case module (the writers, the Job, the comparison): X and Y are two Jobs over inputs of equal
lengths, and the builder asserts that their tables came out byte for byte the same.  Two to four streams of a few hundred bytes to a
few KiB (FLAC, MPEG-4 and fragmented MPEG-4 have one longer stream each; their builders say why), at least one of them busy in every
phase.  Built once and kept.

For the seven newer families Y is not X with other payload bytes alone: it changes what the per-run records HOLD -- fewer rows, runs,
records or frames in one stream (what run X wrote there must be back at the table's fill), a refused sample, a lost key's worth of
output, packets passed over -- and their models give the WHOLE tables, fill and guard rows included.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from ohpipeline_amd import capi

FAMILIES = ("flac", "alac", "raop", "ohm_rx", "ogg", "mp4", "iff", "dsd_file", "mp4f", "cenc", "cbcs", "vorbis", "ts", "adts", "raop_rx")
BOTH_ROUTES = ("mp4f", "cenc", "cbcs", "vorbis", "ts", "adts", "raop_rx")           # the families run on the plain route (kernel variant 1 at create) too


class Pair:
    """family; src["X"], src["Y"]: the source arenas (uint8, equal sizes); dst0: the destination arena before a run (None: the
    family has none); want["X"], want["Y"]: the model's arena after a run (None likewise); ranges: (offset, bytes) of every stream's
    output in the destination arena; summary[which]: the model's results in a form that compares with ==; tables[which]: the model's
    tables as bytes (a family without an arena has nothing else; the newer families with one give them too).  check(): the library's
    own validation of the tables, without a device.
    create(ctx) -> batch; run(ctx, batch, d_src, d_dst, stream); verify(ctx, batch, which): the results and tables the batch holds
    are the model's for `which` (waits for the last run).  route(ctx, batch) -> 1 or 2, which kernels the batch was planned onto (None:
    the family is run on the launches' route alone).  sample_types: None -- the arena is compared byte for byte -- or, for every range
    in turn, the dtype of the samples it holds (Vorbis: the device rounds a float32 transform, the model a float64 one, and a sample
    may come out 1 LSB apart); written[which]: then, the bytes of the arena the model writes in that run, as a mask."""

    def __init__(self, family, src, dst0, want, ranges, summary, check, create, run, verify, tables=None, route=None, sample_types=None, written=None):
        self.family, self.src, self.dst0, self.want, self.ranges, self.summary = family, src, dst0, want, ranges, summary
        self.check, self.create, self.run, self.verify, self.tables, self.route = check, create, run, verify, tables, route
        self.sample_types, self.written = sample_types, written
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


# ---------------------------------------------------------------- fragmented MPEG-4 (mp4f_cases), clear and protected (cenc_cases, cbcs_cases)
def _other_bytes(samples, salt):
    """samples of the same sizes with other bytes in them"""
    return [bytes((b * 5 + 11 * k + 3 * j + salt) & 0xff for j, b in enumerate(s)) for k, s in enumerate(samples)]


def _trun_size_at(m, nth, k):
    """where sample k's size stands in the nth trun of a file whose truns carry a data offset, durations and sizes"""
    return m.find("trun", nth)[1] + 12 + 8 * k + 4


def _renamed(data, at, name=b"free"):
    """the box whose header begins at `at` under another name: the walk steps over it"""
    data = bytes(data)
    return data[:at + 4] + name + data[at + 8:]


def _frag_tables(family, jobs, check, create, run, results, route):
    """What the three fragmented MPEG-4 families share: X and Y are two Jobs of one module (FC.Job, CC.Job, BC.Job) over files of equal
    lengths and equal capacities; the run, packet and sample tables are compared whole, fill rows and guard rows included."""
    import mp4f_cases as FC
    x, y = jobs["X"], jobs["Y"]
    assert (x.n_packets, x.n_runs, x.dst_bytes) == (y.n_packets, y.n_runs, y.dst_bytes)
    _same_tables((x.descs, y.descs))
    dst0 = np.full(x.dst_bytes, FC.FILL, dtype=np.uint8)
    summary = {w: jobs[w].want_results.tobytes() for w in "XY"}
    tables = {w: (jobs[w].want_runs.tobytes(), jobs[w].want_packets.tobytes(), jobs[w].want_samples.tobytes()) for w in "XY"}

    def verify(ctx, b, which):
        job = jobs[which]
        res, runs, packets, samples = results(ctx, b, len(job.streams), job.n_packets, job.n_runs)
        FC.assert_same(res, runs, packets, samples, job.want_dst, job, what=which)          # (the arena is the caller's to compare)

    return Pair(family, {w: jobs[w].src.copy() for w in "XY"}, dst0, {w: jobs[w].want_dst.copy() for w in "XY"},
                [(int(d["dst_offset"]), int(d["dst_capacity"])) for d in x.descs], summary,
                check=lambda: check(x, x.src.size, dst0.size), create=lambda ctx: create(ctx, x, x.src.size, dst0.size), run=run, verify=verify,
                tables=tables, route=route)


FC_TILE = 1024           # mp4frag::kTile


def _mp4f():
    """Three gathered files, Y's samples of the same sizes with other bytes.  A file of 600 + 464 samples in two runs (two tiles of the
    expansion: the second begins inside the second run); a file of three runs whose last moof is called `free` in Y (the walk steps over
    it: X has a run and four rows more, which Y must leave as the batch's fill); an Apple Lossless file in which Y's fourth size stands
    above the packet limit (refused, first_bad_sample, and every later sample of its run with it).  Capacities are X's, the larger."""
    import mp4f_cases as FC

    def files(w):
        def made(counts, seed, codec=FC.FLAC):
            fragments = []
            for k, n in enumerate(counts):
                samples = FC.pattern_samples(n, seed + k)
                if w == "Y":
                    samples = _other_bytes(samples, seed)
                fragments.append(FC.fragment([FC.run(samples, [1 + (j * 5 + k) % 7 for j in range(n)])], sequence=k + 1))
            return FC.mux(FC.init_segment(codec), fragments, codec=codec)
        return [made([600, FC_TILE - 600 + 40], 11), made([5, 6, 4], 21), made([7, 8], 31, FC.ALAC)]

    whole = {w: files(w) for w in "XY"}
    assert [len(m.data) for m in whole["X"]] == [len(m.data) for m in whole["Y"]] and whole["X"][0].n > FC_TILE
    y = whole["Y"]
    data_y = [y[0].data, _renamed(y[1].data, y[1].find("moof", 2)[0]), FC.patched(y[2], _trun_size_at(y[2], 0, 3), 1 << 20)]
    jobs = {"X": FC.Job([FC.stream(m) for m in whole["X"]]),
            "Y": FC.Job([FC.stream(raw, capacity=m.n, run_capacity=len(m.runs), dst_capacity=len(m.data)) for raw, m in zip(data_y, whole["X"])])}
    mx, my = jobs["X"].models, jobs["Y"].models
    assert [m["status"] for m in mx + my] == [0] * 6
    assert (mx[1]["runs"], mx[1]["samples"]) == (3, 15) and (my[1]["runs"], my[1]["samples"]) == (2, 11)
    assert mx[2]["samples_refused"] == 0 and my[2]["samples_refused"] > 0 and my[2]["first_bad_sample"] == 3
    return _frag_tables("mp4f", jobs, lambda j, s, d: capi.mp4f_batch_check(j.descs, j.n_packets, j.n_runs, s, d),
                        lambda ctx, j, s, d: ctx.mp4f_batch(j.descs, j.n_packets, j.n_runs, s, d),
                        lambda ctx, b, s, d, stream: ctx.mp4f_run(b, s, d, stream), lambda ctx, *a: ctx.mp4f_results(*a),
                        lambda ctx, b: ctx.mp4f_paths(b)["route"])


def _cut_to(longer, n):
    """a file that goes on for longer than n bytes, cut there: inside its last fragment"""
    assert len(longer.data) > n > longer.segment_ends[-2] if len(longer.segment_ends) > 1 else len(longer.data) > n > longer.init_bytes
    return longer.data[:n]


def _cenc():
    """Four files under four keys, Y's with other plaintext of the same sizes under the same keys and IVs: FLAC with 8-byte IVs (Y: a
    file that goes on for two samples more, cut where X's ends -- inside its last fragment's sample 8: refused, and first_bad_sample
    says so); Apple Lossless with 16-byte IVs (Y: the tenc says is_protected = 0: X decrypts it, Y copies it); a file whose senc
    stands in front of the truns; and a stream created WITHOUT its key in both runs -- X's file is protected (CENC_NO_KEY, nothing
    gathered), Y's tenc says it is not (copied)."""
    import cenc_cases as CC
    import mp4f_cases as FC
    sizes = [[40, 17, 0, 33, 100, 64, 16, 1, 90], [50, 64, 31, 7, 48, 80, 15], [16, 200, 5, 77, 32, 9, 60, 41], [30, 45, 12, 70, 8]]
    counts = [[4, 5], [3, 4], [5, 3], [2, 3]]
    how = [dict(codec=FC.FLAC, iv_size=8), dict(codec=FC.ALAC, iv_size=16), dict(codec=FC.FLAC, iv_size=8, senc="front"), dict(codec=FC.FLAC, iv_size=16)]
    clear = dict(sinf_options=dict(is_protected=0, iv_size=16))

    def made(k, seed, sizes_k=None, counts_k=None, **more):
        return CC.simple(counts_k or counts[k], sizes=sizes_k or sizes[k], seed=seed, key=CC.key_of(k), kid=CC.kid_of(k), **how[k], **more)

    x = [made(k, 40 + k) for k in range(4)]
    y = [made(0, 50, sizes[0] + [70, 21], [4, 7]), made(1, 51, **clear), made(2, 52), made(3, 53, **clear)]
    data_y = [_cut_to(y[0], len(x[0].data))] + [m.data for m in y[1:]]
    assert [len(d) for d in data_y] == [len(m.data) for m in x]
    jobs = {"X": CC.Job([CC.stream(m, have_key=k != 3) for k, m in enumerate(x)]),
            "Y": CC.Job([CC.stream(raw, capacity=m.n, run_capacity=len(m.runs), dst_capacity=len(m.data), key=m.key, kid=m.kid, have_key=k != 3)
                         for k, (raw, m) in enumerate(zip(data_y, x))])}
    sx, sy = ([int(r["mp4f"]["status"]) for r in jobs[w].want_results] for w in "XY")
    assert sx == [0, 0, 0, capi.CENC_NO_KEY] and sy == [0, 0, 0, 0], (sx, sy)
    cut = jobs["Y"].want_results[0]["mp4f"]
    assert (int(cut["samples"]), int(cut["samples_refused"]), int(cut["first_bad_sample"]), int(cut["samples_available"])) == (11, 1, 8, 8)     # (the cut falls in sample 8)
    assert not jobs["X"].want_results["mp4f"]["samples_refused"].any()
    assert [int(r["is_protected"]) for r in jobs["X"].want_results] == [1, 1, 1, 1] and [int(r["is_protected"]) for r in jobs["Y"].want_results][1:] == [0, 1, 0]
    return _frag_tables("cenc", jobs, lambda j, s, d: capi.cenc_batch_check(j.descs, j.n_packets, j.n_runs, s, d),
                        lambda ctx, j, s, d: ctx.cenc_batch(j.descs, j.n_packets, j.n_runs, s, d),
                        lambda ctx, b, s, d, stream: ctx.cenc_run(b, s, d, stream), lambda ctx, *a: ctx.cenc_results(*a),
                        lambda ctx, b: ctx.cenc_paths(b)["route"])


def _cbcs():
    """Four files under four keys, Y's with other plaintext: a `cbcs` stream with the 1:9 pattern and a constant IV (no senc); a
    `cenc`-scheme stream with subsample entries (Y: a file that goes on for longer, cut where X's ends -- inside its last fragment:
    a sample refused, six rows where X has seven);
    a `cbcs` stream whose samples have three entries each in X and, from the third sample on, one in Y (the senc is shorter by what
    the samples are longer: the subsample table of run Y is shorter, and nothing of run X's rows may show through); and a stream
    created WITHOUT its key in both runs, protected in X (CENC_NO_KEY) and not in Y (copied)."""
    import cbcs_cases as BC
    three = [[(3, 32), (0, 17), (5, 48)], [(1, 16), (2, 40), (0, 0)], [(0, 64), (7, 9), (4, 16)], [(2, 33), (0, 80), (1, 1)], [(6, 16), (3, 3), (0, 32)], [(0, 48), (1, 20), (9, 16)]]
    one = three[:2] + [[(sum(c + p for c, p in e) - 32 + 12, 32)] for e in three[2:]]                # (two entries of six bytes fewer, twelve bytes more)
    subs = [[(4, 16 * k + 5), (0, 33)] for k in range(1, 8)]
    size_of = lambda entries: [sum(c + p for c, p in e) for e in entries]
    const = bytes(range(0x30, 0x40))

    def files(w):
        s = 60 if w == "X" else 70
        a = BC.build([16 * 25 + 3, 7, 16 * 11, 160, 45], counts=[2, 3], constant_iv=const, pattern=(1, 9), senc=None, seed=s, key=BC.key_of(0), kid=BC.kid_of(0))
        more = subs + [[(4, 50), (0, 33)]] * 2 if w == "Y" else subs
        b = BC.build(size_of(more), counts=[3, len(more) - 3], scheme=BC.CENC, iv_size=8, layout=BC.split_layout(more), seed=s + 1, key=BC.key_of(1), kid=BC.kid_of(1))
        parts = three if w == "X" else one
        c = BC.build(size_of(parts), counts=[2, 4], iv_size=16, pattern=(1, 1), layout=BC.split_layout(parts), seed=s + 2, key=BC.key_of(2), kid=BC.kid_of(2))
        d = BC.build([30, 45, 12, 70, 8], counts=[2, 3], iv_size=16, listed=False, seed=s + 3, key=BC.key_of(3), kid=BC.kid_of(3))
        return [a, b, c, d]

    x, y = files("X"), files("Y")
    open_at = BC.at_of(y[3].data, b"tenc") + 8 + 6                                                     # (the tenc's is_protected byte)
    assert y[3].data[open_at] == 1
    data_y = [y[0].data, _cut_to(y[1], len(x[1].data)), y[2].data, y[3].data[:open_at] + b"\0" + y[3].data[open_at + 1:]]
    assert [len(d) for d in data_y] == [len(m.data) for m in x]
    jobs = {"X": BC.Job([BC.stream(m, have_key=k != 3) for k, m in enumerate(x)]),
            "Y": BC.Job([BC.stream(raw, capacity=m.n, run_capacity=len(m.runs), dst_capacity=len(m.data), key=m.key, kid=m.kid, have_key=k != 3, sub_capacity=m.subsamples)
                         for k, (raw, m) in enumerate(zip(data_y, x))])}
    assert jobs["X"].n_subsamples == jobs["Y"].n_subsamples
    sx, sy = ([int(r["cenc"]["mp4f"]["status"]) for r in jobs[w].want_results] for w in "XY")
    assert sx == [0, 0, 0, capi.CENC_NO_KEY] and sy == [0, 0, 0, 0], (sx, sy)
    cut = jobs["Y"].want_results[1]["cenc"]["mp4f"]
    assert (int(cut["samples"]), int(cut["samples_refused"]), int(cut["samples_available"])) == (9, 1, 6) and not jobs["X"].want_results["cenc"]["mp4f"]["samples_refused"].any()
    nx, ny = ([int(r["subsamples"]) for r in jobs[w].want_results] for w in "XY")
    assert nx == [0, 14, 18, 0] and ny == [0, 14, 10, 0], (nx, ny)
    return _frag_tables("cbcs", jobs, lambda j, s, d: capi.cbcs_batch_check(j.descs, j.n_packets, j.n_runs, j.n_subsamples, s, d),
                        lambda ctx, j, s, d: ctx.cbcs_batch(j.descs, j.n_packets, j.n_runs, j.n_subsamples, s, d),
                        lambda ctx, b, s, d, stream: ctx.cbcs_run(b, s, d, stream), lambda ctx, *a: ctx.cbcs_results(*a),
                        lambda ctx, b: ctx.cbcs_paths(b)["route"])


# ---------------------------------------------------------------- Ogg Vorbis packets (vorbis_cases, vorbis_frames.batch_tables)
VORBIS_SPECTRA = 4       # the packets a stream whose spectra verify() compares with the model's, at the least


def _vorbis():
    """Three streams of tests/vorbis_cases.py, each with ONE setup image for both runs: mono_64_128 packets [0, 9) and [30, 39) packed
    16-bit, six_128_512 [0, 6) and [8, 14) in 32-bit planes, stereo_256_2048 [0, 5) and [20, 25) packed 16-bit.  Every pair of packets
    is padded with zeros to the longer one's length (the model decodes the padded bytes too: a packet that ends early reads zeros
    either way).  In Y the mono stream's packet 3 is vorbis_cases.BAD_MODE and the six-channel stream's packet 2 a header packet,
    both padded: packets that were OK in run X are passed over in run Y, and nothing of their floors, residues or spectra may show.
    max_samples cuts the mono stream's last packet short in X.  The PCM is the one thing here that is not bit-exact against the model
    (tests/test_gpu_vorbis_textbook.py): sample_types and written say where samples lie and which of them a run writes."""
    import vorbis_cases as VC
    import vorbis_frames as VF
    import vorbis_textbook as TB
    shapes = [("mono_64_128", (0, 30), 9), ("six_128_512", (0, 8), 6), ("stereo_256_2048", (0, 20), 5)]
    planar = [False, True, False]
    packets = {"X": [], "Y": []}
    for k, (name, (a, b), n) in enumerate(shapes):
        st = VC.stream(name)
        xs, ys = list(st.packets[a:a + n]), list(st.packets[b:b + n])
        if k == 0:
            ys[3] = VC.BAD_MODE
        if k == 1:
            ys[2] = b"\x05vorbis"
        xs, ys = _padded(xs, ys)
        packets["X"].append(xs)
        packets["Y"].append(ys)
    streams = {w: [VF.Stream(VC.stream(name).ident, VC.stream(name).setup, p) for (name, _, _), p in zip(shapes, packets[w])] for w in "XY"}
    uncut = [TB.decode_stream(s.model, s.packets) for s in streams["X"]]
    whole = [pcm.shape[1] for _, _, pcm in uncut]
    caps = [whole[0] - 7] + [n * s.model.bs[1] // 2 for (_, _, n), s in list(zip(shapes, streams["X"]))[1:]]
    tables, dst_bytes = {}, 0
    for w in "XY":
        parts = [VF.batch_tables(capi, [s], planar=p, max_samples=[cap]) for s, p, cap in zip(streams[w], planar, caps)]
        # one batch of the three: batch_tables lays streams of one output form, so the three are laid one behind the other here
        blob, descs, rows, src, at = [], [], [], bytearray(), 0
        for image, d, pk, s, n, _ in parts:
            d, pk = d.copy(), pk.copy()
            d["image_offset"], d["first_packet"], d["dst_offset"] = sum(im.size for im in blob), sum(r.size for r in rows), at + 8
            pk["src_offset"] += len(src)
            blob.append(image)
            descs.append(d)
            rows.append(pk)
            src += s.tobytes()[:-4] + b"\xee" * (-(s.size - 4) % 4)
            at += 8 + ((n + 3) & ~3)                                       # eight guard bytes in front of every stream's share
        tables[w] = (np.concatenate(blob), np.concatenate(descs), np.concatenate(rows), _u8(bytes(src) + bytes(4)))
        dst_bytes = at + 8
    _same_tables(*[(tables["X"][k], tables["Y"][k]) for k in range(3)])
    blob, descs, rows = tables["X"][:3]
    src = {w: tables[w][3] for w in "XY"}
    dst0 = np.full(dst_bytes, 0xA5, dtype=np.uint8)
    models = {w: [TB.decode_stream(s.model, s.packets, cap) for s, cap in zip(streams[w], caps)] for w in "XY"}
    want, written, ranges, sample_types = {}, {}, [], []
    for w in "XY":
        arena, mask = dst0.copy(), np.zeros(dst_bytes, dtype=bool)
        for d, s, p, (recs, _, pcm) in zip(descs, streams[w], planar, models[w]):
            at, ch, n = int(d["dst_offset"]), s.model.channels, pcm.shape[1]
            if p:
                stride = int(d["dst_plane_stride"])
                for c in range(ch):
                    arena[at + c * stride:at + c * stride + 4 * n] = np.frombuffer(pcm[c].astype("<i4").tobytes(), dtype=np.uint8)
                    mask[at + c * stride:at + c * stride + 4 * n] = True
            else:
                arena[at:at + 2 * ch * n] = np.frombuffer(VC.pcm_s16be(pcm), dtype=np.uint8)
                mask[at:at + 2 * ch * n] = True
        want[w], written[w] = arena, mask
    for d, s, p, cap in zip(descs, streams["X"], planar, caps):
        ranges.append((int(d["dst_offset"]), cap * s.model.channels * (4 if p else 2)))
        sample_types.append("<i4" if p else ">i2")
    records = {w: [tuple(int(v) for v in r) for recs, _, _ in models[w] for r in recs] for w in "XY"}
    summary = {}
    for w in "XY":
        rows_w = []
        for recs, _, pcm in models[w]:
            ok = next((k for k, r in enumerate(recs) if r[0] != TB.OK), len(recs))
            rows_w.append((ok, recs[ok][0] if ok < len(recs) else 0, pcm.shape[1]))
        summary[w] = rows_w
    mx = models["X"]
    assert [s[:2] for s in summary["X"]] == [(9, 0), (6, 0), (5, 0)] and [s[0] for s in summary["Y"]] == [3, 2, 5] and all(s[1] for s in summary["Y"][:2])
    assert 0 < mx[0][0][-1][3] == uncut[0][0][-1][3] - 7 and sum(r[3] for r in mx[0][0]) == caps[0]      # (max_samples cut the mono stream's last packet)
    first = np.concatenate([[0], np.cumsum([len(p) for p in packets["X"]])])

    def verify(ctx, b, which):
        res, pres = ctx.vorbis_results(b, len(descs), len(rows))
        got = [(int(r["status"]), int(r["mode"]), int(r["blocksize"]), int(r["samples"]), int(r["position"])) for r in pres]
        assert got == records[which] and not pres["reserved"].any(), (which, got, records[which])
        got = [(int(r["packets_ok"]), int(r["first_bad_status"]), int(r["samples"])) for r in res]
        assert got == summary[which] and not res["reserved"].any(), (which, got, summary[which])
        for i, (recs, spectra, _) in enumerate(models[which]):
            checked = 0
            for k, spec in enumerate(spectra):
                if spec is None:
                    continue
                for c in range(spec.shape[0]):
                    mine = ctx.vorbis_spectrum(b, int(first[i]) + k, c, recs[k][2] // 2)
                    assert mine.tobytes() == spec[c].tobytes(), (which, i, k, c)
                checked += 1
            assert checked >= VORBIS_SPECTRA, (which, i, checked)

    return Pair("vorbis", src, dst0, want, ranges, summary,
                check=lambda: capi.vorbis_batch_check(descs, rows, blob, src["X"].size, dst_bytes),
                create=lambda ctx: ctx.vorbis_batch(descs, rows, blob, src["X"].size, dst_bytes),
                run=lambda ctx, b, s, d, stream: ctx.vorbis_run(b, s, d, stream), verify=verify,
                tables={w: (np.array(records[w], dtype="<i8").tobytes(),) for w in "XY"},
                route=lambda ctx, b: ctx.vorbis_paths(b)["route"], sample_types=sample_types, written=written)


# ---------------------------------------------------------------- MPEG transport streams and ADTS (ts_cases)
def _ts():
    """Three streams, Y's with other elementary bytes: three PES packets (Y: the counter of the fourth audio packet jumps); four PES
    packets (Y: the sync byte of a packet in the middle is lost -- it is stepped over, and the counter jumps behind it); four PES
    packets in X and three in Y in as many transport packets: the fourth record of that stream must be the table's fill in run Y."""
    import ts_cases as TC

    def packets(w):
        rng = TC.Lcg(301 if w == "X" else 302)
        a = TC.head_packets() + TC.audio_run(rng, n_pes=3)[0]
        b = TC.head_packets() + TC.audio_run(rng, n_pes=4, es_bytes=(200, 500, 90, 333))[0]
        c = TC.head_packets() + TC.audio_run(rng, n_pes=4 if w == "X" else 3, es_bytes=(300, 41, 700, 100) if w == "X" else (300, 900, 100))[0]
        if w == "Y":
            a[5] = a[5][:3] + bytes([a[5][3] & 0xF0 | (a[5][3] + 5) & 15]) + a[5][4:]
            b[5] = b"\x48" + b[5][1:]
        return [a, b, c]

    data = {w: [b"".join(p) for p in packets(w)] for w in "XY"}
    assert [len(d) for d in data["X"]] == [len(d) for d in data["Y"]]
    caps = [max(len(TC.TX.demux(data[w][i], 0, 0, 0, 0)["pes"]) for w in "XY") for i in range(3)]
    jobs = {w: TC.Job([TC.stream(d, pes_capacity=cap) for d, cap in zip(data[w], caps)]) for w in "XY"}
    x, y = jobs["X"], jobs["Y"]
    _same_tables((x.descs, y.descs), (x.dst0, y.dst0))
    assert x.n_pes == y.n_pes and [len(m["pes"]) for m in x.models] == [3, 4, 4] and [len(m["pes"]) for m in y.models] == [3, 4, 3]
    assert [m["cc_jumps"] for m in x.models] == [0, 0, 0] and y.models[0]["cc_jumps"] > 0 and (x.models[1]["bad_sync"], y.models[1]["bad_sync"]) == (0, 1)

    def results_of(job):
        res, pes = np.zeros(len(job.streams), dtype=capi.TS_STREAM_RESULT), np.zeros(job.n_pes, dtype=capi.TS_PES)       # (the table's fill is zeros)
        for i, (d, m) in enumerate(zip(job.descs, job.models)):
            for f in TC.RESULT_FIELDS:
                res[i][f] = m[f]
            res[i]["pes_packets"], res[i]["bytes_delivered"] = len(m["pes"]), len(m["run"])
            for k, rec in enumerate(m["pes"][:int(d["pes_capacity"])]):
                for f in TC.PES_FIELDS:
                    pes[int(d["pes_first"]) + k][f] = rec[f]
        return res, pes

    want = {w: results_of(jobs[w]) for w in "XY"}

    def verify(ctx, b, which):
        res, pes = ctx.ts_results(b, len(x.streams), x.n_pes)
        TC.assert_same(res, pes, jobs[which].want.tobytes(), jobs[which])                                                 # (the arena is the caller's to compare)
        assert res.tobytes() == want[which][0].tobytes(), (which, res, want[which][0])
        assert pes.tobytes() == want[which][1].tobytes(), (which, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(pes, want[which][1])]).tolist())

    return Pair("ts", {w: jobs[w].src.copy() for w in "XY"}, x.dst0.copy(), {w: jobs[w].want.copy() for w in "XY"},
                [(int(d["dst_offset"]), int(d["dst_capacity"])) for d in x.descs], {w: want[w][0].tobytes() for w in "XY"},
                check=lambda: capi.ts_batch_check(x.descs, x.n_pes, x.src.size, x.dst0.size),
                create=lambda ctx: ctx.ts_batch(x.descs, x.n_pes, x.src.size, x.dst0.size),
                run=lambda ctx, b, s, d, stream: ctx.ts_run(b, s, d, stream), verify=verify, tables={w: (want[w][1].tobytes(),) for w in "XY"},
                route=lambda ctx, b: ctx.ts_paths(b)["route"])


def _adts():
    """Three streams and no destination arena: the frame table and the results are what a run leaves.  Y has other payloads; junk between
    two frames where X has a frame of that length (an interruption, skipped bytes); a header whose length field is wrong, so that the
    chain loses its footing there and the table has fewer frames -- the surplus rows must be the table's fill; and a stream that is
    recognised from its second frame on where X's begins at byte 0."""
    import ts_cases as TC

    def streams(w):
        rng = TC.Lcg(77 if w == "X" else 78)
        f = [TC.adts_frame(TC.clean(rng.bytes(n)), protection_absent=bool(k % 3)) for k, n in enumerate((40, 100, 33, 64, 2, 250, 90, 17))]
        a, b, c = list(f[:5]), list(f[3:8]), list(f[1:6])
        if w == "Y":
            a[2] = TC.clean(rng.bytes(len(a[2])))
            b[2] = TC.adts_frame(TC.clean(rng.bytes(len(b[2]) - 7)), length=len(b[2]) + 9)[:len(b[2])]
            c[0] = TC.clean(rng.bytes(len(c[0])))
        return [b"".join(a), b"".join(b), b"".join(c)]

    data = {w: streams(w) for w in "XY"}
    assert [len(d) for d in data["X"]] == [len(d) for d in data["Y"]]
    caps = [max(len(TC.TX.adts_chain(data[w][i], 0)["frames"]) for w in "XY") for i in range(3)]
    jobs = {w: TC.AdtsJob([TC.adts_stream(d, frame_capacity=cap) for d, cap in zip(data[w], caps)]) for w in "XY"}
    x, y = jobs["X"], jobs["Y"]
    _same_tables((x.descs, y.descs))
    assert x.n_frames == y.n_frames and x.src.size == y.src.size
    assert [len(m["frames"]) for m in x.models] == [5, 5, 5] and all(len(my["frames"]) < 5 for my in y.models)
    assert [m["interruptions"] for m in x.models] == [0, 0, 0] and y.models[0]["interruptions"] == 1 and y.models[2]["first_frame_offset"] > 0

    def results_of(job):
        res, frames = np.zeros(len(job.streams), dtype=capi.ADTS_STREAM_RESULT), np.zeros(job.n_frames, dtype=capi.ADTS_FRAME)   # (the table's fill is zeros)
        for i, (d, m) in enumerate(zip(job.descs, job.models)):
            for f in TC.ADTS_RESULT_FIELDS:
                res[i][f] = m[f]
            res[i]["frames"] = len(m["frames"])
            for k, rec in enumerate(m["frames"][:int(d["frame_capacity"])]):
                for f in TC.FRAME_FIELDS:
                    frames[int(d["frame_first"]) + k][f] = rec[f]
        return res, frames

    want = {w: results_of(jobs[w]) for w in "XY"}

    def verify(ctx, b, which):
        res, frames = ctx.adts_results(b, len(x.streams), x.n_frames)
        TC.assert_same_adts(res, frames, jobs[which])
        assert res.tobytes() == want[which][0].tobytes(), (which, res, want[which][0])
        assert frames.tobytes() == want[which][1].tobytes(), (which, np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(frames, want[which][1])]).tolist())

    return Pair("adts", {w: jobs[w].src.copy() for w in "XY"}, None, {"X": None, "Y": None}, [], {w: want[w][0].tobytes() for w in "XY"},
                check=lambda: capi.adts_batch_check(x.descs, x.n_frames, x.src.size),
                create=lambda ctx: ctx.adts_batch(x.descs, x.n_frames, x.src.size),
                run=lambda ctx, b, s, d, stream: ctx.adts_run(b, s, stream), verify=verify, tables={w: (want[w][1].tobytes(),) for w in "XY"},
                route=lambda ctx, b: ctx.adts_paths(b)["route"])


# ---------------------------------------------------------------- the RAOP receiver (raop_rx_cases.Job)
def _raop_rx():
    """Three streams and no destination arena: the records, the packet rows and the results are what a run leaves.  X: every frame in
    order, some of them as resend responses on the control port.  Y: datagrams of the same lengths on the same ports with other
    payloads -- a sync datagram where X has a resent frame, a frame missing (the frames behind it wait), the late resend that fills
    the gap, a resend of a frame long out (a duplicate); a stream that ends inside a repair, with a duplicate of its first waiting
    frame (a resend request: n_ranges, n_pending); and a stream that starts from a running state, with a sync datagram that changes
    the delay and a late resend."""
    import raop_rx_cases as RC
    A, R, S = RC.A, RC.R, RC.S
    sizes = [(9, 30, 4, 100, 7, 41, 250, 5, 12, 64), (16, 1, 80, 33, 200, 8), (4, 120, 6, 50, 77)]

    def grams(w):
        rng = RC.Lcg(61 if w == "X" else 67)
        p = [[rng.bytes(n) for n in row] for row in sizes]
        if w == "X":
            a = [A(10), A(11), R(12), A(13), A(14), R(15), A(16), A(17), R(18), A(19)]
            b = [A(100), A(101), A(102), A(103), A(104), A(105)]
            c = [R(200), A(201), A(202), R(203), A(204)]
        else:
            a = [A(10), A(11), S(5000, 11025), A(13), A(14), R(12), A(15), A(16), R(14), A(17)]
            b = [A(100), A(101), A(103), A(104), A(103), A(106)]
            c = [S(7000, 11025 + 500), A(200), A(202), R(201), A(203)]
        out = []
        for made, payloads in zip((a, b, c), p):
            row = []
            for (gram, port), body in zip(made, payloads):
                sync = port == RC.RX.CONTROL and gram[1] & 0x7f == 0x54
                head = len(gram) - 4                                       # (the builders' own four payload bytes are replaced)
                row.append((gram if sync else gram[:head] + body, port))
            out.append(row)
        return out

    made = {w: grams(w) for w in "XY"}
    states = [None, None, RC.running_state(199, latency=11025)]
    jobs = {w: RC.Job([RC.stream(g, state, max_frames=5) for g, state in zip(made[w], states)]) for w in "XY"}
    x, y = jobs["X"], jobs["Y"]
    _same_tables((x.d_streams, y.d_streams), (x.d_grams, y.d_grams))
    X = RC.RX
    assert all(r["disposition"] == X.OUTPUT for recs in x.recs for r in recs) and all(not r["ranges"] and not r["n_pending"] for r in x.results)
    assert [r["disposition"] for r in y.recs[0]] == [X.OUTPUT, X.OUTPUT, X.SYNC] + [X.OUTPUT] * 5 + [X.DUPLICATE, X.OUTPUT]
    assert [r["order"] for r in y.recs[0]][3:6] == [3, 4, 2]                           # (the late resend goes out in front of the two that waited)
    assert [r["disposition"] for r in y.recs[1]] == [X.OUTPUT, X.OUTPUT, X.PENDING, X.PENDING, X.DUPLICATE, X.PENDING]
    assert y.results[1]["n_pending"] == 3 and y.results[1]["ranges"] == [(102, 102), (105, 105)]
    assert [r["disposition"] for r in y.recs[2]] == [X.SYNC] + [X.OUTPUT] * 4 and y.recs[2][1]["events"] & X.DELAY and [r["order"] for r in y.recs[2]][1:] == [0, 2, 1, 3]
    summary = {w: jobs[w].want_results.tobytes() for w in "XY"}
    tables = {w: (jobs[w].want_records.tobytes(), jobs[w].want_rows.tobytes()) for w in "XY"}

    def verify(ctx, b, which):
        job = jobs[which]
        sres, recs = ctx.raop_rx_results(b, len(job.streams), len(job.table))
        RC.assert_same(sres, recs, ctx.raop_rx_packets(b, len(job.table)), job)

    return Pair("raop_rx", {w: _u8(jobs[w].src) for w in "XY"}, None, {"X": None, "Y": None}, [], summary,
                check=lambda: capi.raop_rx_batch_check(x.d_streams, x.d_grams, len(x.src)),
                create=lambda ctx: ctx.raop_rx_batch(x.d_streams, x.d_grams, len(x.src)),
                run=lambda ctx, b, s, d, stream: ctx.raop_rx_run(b, s, stream), verify=verify, tables=tables,
                route=lambda ctx, b: ctx.batch_paths(b)["raop_rx_route"])


_BUILDERS = {"flac": _flac, "alac": _alac, "raop": _raop, "ohm_rx": _ohm_rx, "ogg": _ogg, "mp4": _mp4, "iff": _iff, "dsd_file": _dsd_file,
             "mp4f": _mp4f, "cenc": _cenc, "cbcs": _cbcs, "vorbis": _vorbis, "ts": _ts, "adts": _adts, "raop_rx": _raop_rx}


@functools.lru_cache(maxsize=None)
def pair(family):
    return _BUILDERS[family]()
