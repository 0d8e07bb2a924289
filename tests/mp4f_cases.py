"""What the fragmented MPEG-4 tests share: a fragment muxer of the tests' own (on tests/mp4_cases.py's box and Node) that wraps FLAC
frames (the golden/flac fixtures, cut at the spans tests/flac_cases.py knows) and Apple Lossless packets (tests/alac_cases.py), or arithmetic patterns, into
an initialisation segment and media segments, and keeps ITS OWN RECORD of every sample's place, size, first frame and run and of every
run -- the truth the model (tests/mp4f_textbook.py) and the product are held to, made by no parser --; the named good and malformed
files; the fixed-seed damage; and the batches: the arenas, the descriptors, and what the model says every output must be."""
import struct

import numpy as np

import alac_cases as AC
import mp4_cases as MC
import mp4f_textbook as FX

FILL, GUARD_ROWS, GUARD_BYTES = 0xa5, 3, 32
Node, full, box, Lcg = MC.Node, MC.full, MC.box, AC.Lcg
ALAC, FLAC = b"alac", b"fLaC"
M64 = (1 << 64) - 1


def streaminfo(min_block=4096, max_block=4096, rate=44100, channels=2, bits=16, total=0, md5=bytes(16), min_frame=0, max_frame=0):
    v = 0
    for value, width in ((min_block, 16), (max_block, 16), (min_frame, 24), (max_frame, 24), (rate, 20), (channels - 1, 3), (bits - 1, 5), (total, 36)):
        v = (v << width) | value
    return v.to_bytes(18, "big") + md5


def dfla(info, more=(), version_flags=0, last=True):
    """the dfLa box: STREAMINFO, then `more` = [(type, payload)]; the last block carries the flag unless last is False"""
    blocks = [(0, info)] + list(more)
    body = struct.pack(">I", version_flags)
    for k, (kind, payload) in enumerate(blocks):
        flag = 0x80 if last and k + 1 == len(blocks) else 0
        body += bytes([flag | kind]) + len(payload).to_bytes(3, "big") + payload
    return Node(b"dfLa", body)


PATTERN_INFO = streaminfo()
PATTERN_COOKIE = MC.PATTERN_COOKIE


class Fragmented(MC.Muxed):
    """data; marks; per sample offsets / sizes / first_frames / frames / run_of; runs [(place, first_frame, first_sample, samples,
    bytes)]; init_bytes (where the first media segment begins); segment_ends (the end of every media segment); codec; track_id;
    timescale; duration; total_frames; info (the STREAMINFO fields) or cfg (the Apple Lossless configuration)"""


def entry_node(codec, inner, channels, bits, rate, extra=()):
    return MC.sample_entry(codec, channels, bits, rate, [Node(b"free", b"pad")] + list(extra) + ([inner] if inner is not None else []))


def init_segment(codec=FLAC, *, info=PATTERN_INFO, cookie=PATTERN_COOKIE, track_id=1, timescale=44100, mdhd_duration=0, mdhd_version=0, tkhd_version=0,
                 trex=None, mehd=None, mvex=True, mvex_first=False, other_track=None, moov_form=32, stsz_samples=0, inner=True, entry_channels=2,
                 entry_bits=16, drop=(), dfla_options=None, trex_other_first=False, moov_extra=(), entry=None):
    """-> [Node]: ftyp and moov.  trex: None or (duration, size); mehd: None or (version, duration); other_track: None, "before" or
    "after" (an mp4a trak, track 2); drop: of "tkhd", "mdhd", "stsd"."""
    if codec == ALAC:
        inner_node = Node(b"alac", bytes(4) + cookie) if inner else None
    else:
        inner_node = dfla(info, **(dfla_options or {})) if inner else None
    if isinstance(inner, Node):
        inner_node = inner
    entry = entry if entry is not None else entry_node(codec, inner_node, entry_channels, entry_bits, timescale)

    def tkhd(ident):
        return full(b"tkhd", struct.pack(">QQI", 0, 0, ident) + bytes(60), 1) if tkhd_version else full(b"tkhd", struct.pack(">III", 0, 0, ident) + bytes(68))

    def trak(ident, sample_entry, scale):
        mdhd = full(b"mdhd", struct.pack(">QQIQHH", 0, 0, scale, mdhd_duration, 0x55c4, 0), 1) if mdhd_version else \
            full(b"mdhd", struct.pack(">IIIIHH", 0, 0, scale, mdhd_duration, 0x55c4, 0))
        stbl = ([] if "stsd" in drop else [full(b"stsd", struct.pack(">I", 1) + sample_entry.emit(0, []))]) + \
            [full(b"stts", struct.pack(">I", 0)), full(b"stsc", struct.pack(">I", 0)), full(b"stsz", struct.pack(">II", 0, stsz_samples) + bytes(4 * stsz_samples)),
             full(b"stco", struct.pack(">I", 0))]
        mdia = ([] if "mdhd" in drop else [mdhd]) + [full(b"hdlr", bytes(8) + b"soun" + bytes(13)), Node(b"minf", [full(b"smhd", bytes(4)), Node(b"stbl", stbl)])]
        return Node(b"trak", ([] if "tkhd" in drop else [tkhd(ident)]) + [Node(b"mdia", mdia)])

    mine = trak(track_id, entry, timescale)
    other = trak(track_id + 1, MC.sample_entry(b"mp4a", 2, 16, 44100, [Node(b"esds", bytes(20))]), 44100)
    traks = {None: [mine], "before": [other, mine], "after": [mine, other]}[other_track]
    kids = []
    if mehd is not None:
        kids.append(full(b"mehd", struct.pack(">Q" if mehd[0] else ">I", mehd[1]), mehd[0]))
    trexes = [full(b"trex", struct.pack(">IIIII", track_id + 1, 1, 77, 99, 0))] if trex_other_first or other_track else []
    if trex is not None:
        trexes.append(full(b"trex", struct.pack(">IIIII", track_id, 1, trex[0], trex[1], 0)))
    extends = [Node(b"mvex", kids + trexes)] if mvex else []
    body = [full(b"mvhd", bytes(96))] + list(moov_extra) + (extends + traks if mvex_first else traks + extends)
    return [Node(b"ftyp", b"iso6\x00\x00\x00\x01iso6dash"), Node(b"moov", body, moov_form)]


def run(samples, durations, *, fields="all", data_offset=True, gap=0, first_sample_flags=False, extras=0):
    """a trun to be.  fields: "all", "size", "duration", "none" -- which of the two an entry carries; extras: 0x400 | 0x800 (sample
    flags, composition offsets) carried besides; gap: stray bytes in front of the run's data (with data_offset only)"""
    assert len(samples) == len(durations) and (data_offset or gap == 0)
    return dict(samples=list(samples), durations=list(durations), fields=fields, data_offset=data_offset, gap=gap, first_sample_flags=first_sample_flags, extras=extras)


def fragment(runs, *, base="moof", tfdt=None, tfhd_size=None, tfhd_duration=None, other_traf=None, styp=False, sidx=False, moof_form=32, mdat_form=32,
             tfhd_extras=0, sequence=1):
    """a media segment to be.  base: "moof" (default-base-is-moof), "first" (no flag: the moof's start, for a first traf) or
    "explicit" (base_data_offset = the END of the segment's mdat, so that every data_offset is negative) or "data" (base_data_offset =
    where the first run's bytes lie, which may then go without a data_offset); tfdt: None or (version, time);
    other_traf: None, "before" or "after" -- a traf of track_id + 1 with a run of its own"""
    return dict(runs=runs, base=base, tfdt=tfdt, tfhd_size=tfhd_size, tfhd_duration=tfhd_duration, other_traf=other_traf, styp=styp, sidx=sidx,
                moof_form=moof_form, mdat_form=mdat_form, tfhd_extras=tfhd_extras, sequence=sequence)


def trun_node(r, offset):
    flags = {"all": 0x300, "size": 0x200, "duration": 0x100, "none": 0}[r["fields"]] | r["extras"] | (1 if r["data_offset"] else 0) | (4 if r["first_sample_flags"] else 0)
    body = struct.pack(">I", len(r["samples"]))
    if r["data_offset"]:
        body += struct.pack(">i", offset)
    if r["first_sample_flags"]:
        body += struct.pack(">I", 0x02000000)
    for k, (sample, duration) in enumerate(zip(r["samples"], r["durations"])):
        if flags & 0x100:
            body += struct.pack(">I", duration)
        if flags & 0x200:
            body += struct.pack(">I", len(sample))
        if flags & 0x400:
            body += struct.pack(">I", 0x01010000 + k)
        if flags & 0x800:
            body += struct.pack(">I", 3 * k)
    return Node(b"trun", bytes([0]) + flags.to_bytes(3, "big") + body)


def mux(init, fragments, *, track_id=1, trex=None, codec=FLAC, tail=(), **record):
    """-> Fragmented.  init: the Nodes of init_segment(); trex: the defaults it declared, for the record"""
    marks, data, at = [], b"", 0
    for node in init:
        piece = node.emit(at, marks)
        data += piece
        at += len(piece)
    init_bytes = at
    offsets, sizes, first_frames, frames, run_of, runs, segment_ends = [], [], [], [], [], [], []
    frame = 0
    for f in fragments:
        for node in ([Node(b"styp", b"msdh\x00\x00\x00\x00msdh")] if f["styp"] else []) + ([full(b"sidx", bytes(28))] if f["sidx"] else []):
            piece = node.emit(at, marks)
            data += piece
            at += len(piece)
        other_data = b"\xdd" * 50
        # mdat: the other traf's bytes where it comes first, then the runs one after the other
        payload, places = bytearray(), []
        if f["other_traf"] == "before":
            payload += other_data
        for r in f["runs"]:
            payload += b"\xee" * r["gap"]
            places.append(len(payload))
            payload += b"".join(r["samples"])
        if f["other_traf"] == "after":
            other_at = len(payload)
            payload += other_data
        else:
            other_at = 0

        def moof(moof_at, mdat_payload_at):
            mdat_end = mdat_payload_at + len(payload)
            base = {"moof": moof_at, "first": moof_at, "explicit": mdat_end, "data": mdat_payload_at + (places[0] if places else 0)}[f["base"]]
            tf = {"moof": 0x20000, "first": 0, "explicit": 1, "data": 1}[f["base"]] | f["tfhd_extras"] | (0x8 if f["tfhd_duration"] is not None else 0) | (0x10 if f["tfhd_size"] is not None else 0)
            body = struct.pack(">I", track_id)
            if tf & 1:
                body += struct.pack(">Q", base)
            if tf & 2:
                body += struct.pack(">I", 1)
            if tf & 8:
                body += struct.pack(">I", f["tfhd_duration"])
            if tf & 0x10:
                body += struct.pack(">I", f["tfhd_size"])
            if tf & 0x20:
                body += struct.pack(">I", 0x01010000)
            kids = [Node(b"tfhd", bytes([0]) + tf.to_bytes(3, "big") + body)]
            if f["tfdt"] is not None:
                kids.append(full(b"tfdt", struct.pack(">Q" if f["tfdt"][0] else ">I", f["tfdt"][1]), f["tfdt"][0]))
            kids += [trun_node(r, mdat_payload_at + place - base) for r, place in zip(f["runs"], places)]
            mine = Node(b"traf", kids)
            other = Node(b"traf", [Node(b"tfhd", bytes([0]) + (0x20000).to_bytes(3, "big") + struct.pack(">I", track_id + 1)),
                                   trun_node(run([other_data], [1024]), mdat_payload_at + other_at - moof_at)])
            trafs = {None: [mine], "before": [other, mine], "after": [mine, other]}[f["other_traf"]]
            return Node(b"moof", [full(b"mfhd", struct.pack(">I", f["sequence"]))] + trafs, f["moof_form"]), base

        size = len(moof(0, 0)[0].emit(0, []))
        mdat_payload_at = at + size + (16 if f["mdat_form"] == 64 else 8)
        node, base = moof(at, mdat_payload_at)
        data += node.emit(at, marks)
        data += Node(b"mdat", bytes(payload), f["mdat_form"]).emit(at + size, marks)
        # the record
        size_default = f["tfhd_size"] if f["tfhd_size"] is not None else trex[1] if trex else None
        duration_default = f["tfhd_duration"] if f["tfhd_duration"] is not None else trex[0] if trex else None
        next_place = None
        for k, (r, place) in enumerate(zip(f["runs"], places)):
            if not r["samples"]:
                continue
            first_of_traf = not any(q["samples"] for q in f["runs"][:k])
            if r["fields"] in ("duration", "none"):
                assert all(len(s) == size_default for s in r["samples"]), "a run without sizes holds samples of the default size"
            if r["fields"] in ("size", "none"):
                assert all(d == duration_default for d in r["durations"]), "a run without durations holds samples of the default duration"
            if not r["data_offset"]:          # the run's bytes lie where the format says they do: the muxer put them there
                assert mdat_payload_at + place == (base if first_of_traf else next_place), "a run without data_offset follows its predecessor"
            if first_of_traf and f["tfdt"] is not None:
                frame = f["tfdt"][1]
            spot = mdat_payload_at + place
            runs.append((spot, frame, len(offsets), len(r["samples"]), sum(len(s) for s in r["samples"])))
            for sample, duration in zip(r["samples"], r["durations"]):
                offsets.append(spot)
                sizes.append(len(sample))
                first_frames.append(frame)
                frames.append(duration)
                run_of.append(len(runs) - 1)
                spot += len(sample)
                frame = (frame + duration) & M64
            next_place = spot
        at = mdat_payload_at + len(payload)
        segment_ends.append(at)
    for node in tail:
        piece = node.emit(at, marks)
        data += piece
        at += len(piece)
    return Fragmented(data=data, marks=marks, offsets=offsets, sizes=sizes, first_frames=first_frames, frames=frames, run_of=run_of, runs=runs, n=len(offsets),
                      init_bytes=init_bytes, segment_ends=segment_ends, codec=codec, track_id=track_id, total_frames=sum(frames) & M64, **record)


def pattern_samples(n, seed=1, size=None):
    rng = Lcg(seed)
    return [bytes((k * 7 + j * 13 + seed) & 0xff for j in range(size if size is not None else 1 + rng.next() % 90)) for k in range(n)]


def simple(counts, *, codec=FLAC, seed=1, fields="all", trex=None, durations=None, init=None, size=None, **fragment_options):
    """a pattern file: one fragment a count, one run a fragment"""
    fragments = []
    for k, n in enumerate(counts):
        d = [durations if durations is not None else 1 + (j * 5 + k) % 7 for j in range(n)]
        fragments.append(fragment([run(pattern_samples(n, seed + k, size), d, fields=fields)], sequence=k + 1, **fragment_options))
    return mux(init_segment(codec, trex=trex, **(init or {})), fragments, trex=trex, codec=codec)


def flac_file(name, per_fragment=3, **init):
    """a golden FLAC fixture as a fragmented file: a sample a frame, per_fragment frames a fragment; .pcm_md5 and .info from the file"""
    import flac_cases as FC
    import flac_textbook as T
    fx = FC.fixture(name)
    spans = FC.frame_spans(name)
    res, _ = FC.model(FC.whole(fx))
    samples = [fx.data[a:b] for a, b in spans]
    durations = [f.header.blocksize for f in res.frames]
    fragments = [fragment([run(samples[k:k + per_fragment], durations[k:k + per_fragment])], tfdt=(1, sum(durations[:k])), sequence=k // per_fragment + 1)
                 for k in range(0, len(samples), per_fragment)]
    info = fx.data[8:42]
    m = mux(init_segment(FLAC, info=info, timescale=fx.info["sample_rate"], entry_channels=fx.info["channels"], entry_bits=fx.info["bits"],
                         mehd=(0, fx.info["total_samples"]), **init), fragments, codec=FLAC)
    m.fixture, m.info = fx, fx.info
    return m


def alac_file(name, per_fragment=4, **init):
    fx = AC.load_fixture(name)
    fl, total, n = fx["cfg"]["frame_length"], fx["meta"]["frames"], len(fx["packets"])
    durations = [fl] * (n - 1) + [total - fl * (n - 1)]
    fragments = [fragment([run(fx["packets"][k:k + per_fragment], durations[k:k + per_fragment])], sequence=k // per_fragment + 1) for k in range(0, n, per_fragment)]
    cfg = fx["cfg"]
    m = mux(init_segment(ALAC, cookie=fx["cookie"], timescale=cfg["sample_rate"], entry_channels=cfg["channels"], entry_bits=cfg["bit_depth"], **init), fragments, codec=ALAC)
    m.fixture, m.cfg = fx, cfg
    return m


def named_good():
    """-> {name: Fragmented}: every way a good file is written"""
    out = {}
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049):
        out[f"run_of_{n}"] = simple([n], seed=n)
    out["all_default_tfhd"] = simple([5, 70], fields="none", durations=1024, size=33, tfhd_size=33, tfhd_duration=1024)
    out["all_default_with_flags_and_offsets"] = mux(init_segment(), [fragment([run(pattern_samples(9, 2, 21), [512] * 9, fields="none", extras=0xc00, first_sample_flags=True)],
                                                                             tfhd_size=21, tfhd_duration=512, tfhd_extras=0x22)])
    out["size_only"] = mux(init_segment(), [fragment([run(pattern_samples(70, 3), [4096] * 70, fields="size", extras=0x400)], tfhd_duration=4096)])
    out["duration_only"] = mux(init_segment(), [fragment([run(pattern_samples(70, 4, 17), [1 + k % 5 for k in range(70)], fields="duration", extras=0x800)], tfhd_size=17)])
    out["trex_defaults_only"] = simple([6, 7], fields="none", durations=4096, size=40, trex=(4096, 40))
    out["trex_beaten_by_tfhd"] = simple([6], fields="none", durations=1000, size=12, trex=(4096, 40), tfhd_size=12, tfhd_duration=1000)
    two = [run(pattern_samples(5, 5), [100] * 5), run(pattern_samples(66, 6), [200] * 66, gap=7)]
    out["two_truns_with_data_offset"] = mux(init_segment(), [fragment(two), fragment(two, sequence=2)])
    follow = [run(pattern_samples(5, 5), [100] * 5), run(pattern_samples(66, 6), [200] * 66, data_offset=False), run(pattern_samples(3, 7), [300] * 3, data_offset=False)]
    out["two_truns_without_data_offset"] = mux(init_segment(), [fragment(follow), fragment(follow, sequence=2)])
    out["first_trun_at_the_base"] = mux(init_segment(), [fragment(follow[1:], base="data"), fragment(follow[1:], base="data", sequence=2)])
    out["negative_data_offset"] = mux(init_segment(), [fragment(two, base="explicit"), fragment(two, base="explicit", sequence=2)])
    out["default_base_is_moof"] = simple([9, 9], base="moof")
    out["no_base_flag_first_traf"] = simple([9, 9], base="first")
    out["empty_trun_between"] = mux(init_segment(), [fragment([run(pattern_samples(4, 8), [10] * 4), run([], []), run(pattern_samples(4, 9), [20] * 4)])])
    out["tfdt_v0"] = mux(init_segment(), [fragment([run(pattern_samples(4, 1), [10] * 4)], tfdt=(0, 0)), fragment([run(pattern_samples(4, 2), [10] * 4)], tfdt=(0, 40))])
    out["tfdt_v1_with_a_gap"] = mux(init_segment(), [fragment([run(pattern_samples(4, 1), [10] * 4)], tfdt=(1, 1 << 33)),
                                                     fragment([run(pattern_samples(4, 2), [10] * 4), run(pattern_samples(4, 3), [10] * 4)], tfdt=(1, (1 << 33) + 1000)),
                                                     fragment([run(pattern_samples(2, 4), [10] * 2)])])
    out["tfdt_absent"] = simple([4, 4, 4])
    out["two_tracks_taken_first"] = mux(init_segment(other_track="after"), [fragment([run(pattern_samples(7, 1), [10] * 7)], other_traf="after"),
                                                                            fragment([run(pattern_samples(7, 2), [10] * 7)], other_traf="after", base="first")])
    out["two_tracks_taken_second"] = mux(init_segment(other_track="before", trex=(10, 0)), [fragment([run(pattern_samples(7, 1), [10] * 7)], other_traf="before"),
                                                                                           fragment([run(pattern_samples(7, 2), [10] * 7)], other_traf="before", base="explicit")], trex=(10, 0))
    out["box_sizes_64"] = mux(init_segment(moov_form=64), [fragment([run(pattern_samples(7, 1), [10] * 7)], moof_form=64, mdat_form=64)])
    out["mehd_sidx_styp"] = mux(init_segment(mehd=(1, 123456789012), mvex_first=True), [fragment([run(pattern_samples(7, k), [10] * 7)], styp=True, sidx=True) for k in (1, 2)],
                                tail=[Node(b"mfra", bytes(16))])
    out["mdhd_duration_beats_mehd"] = mux(init_segment(mehd=(0, 77), mdhd_duration=1234, mdhd_version=1, tkhd_version=1, track_id=0x01020304),
                                          [fragment([run(pattern_samples(3, 1), [10] * 3)])], track_id=0x01020304)
    out["init_segment_alone"] = mux(init_segment(), [])
    out["init_segment_alone_no_mvex_no_samples"] = mux(init_segment(mvex=False), [])
    out["alac_patterns"] = simple([5, 6], codec=ALAC)
    for channels, bits in ((c, b) for c in range(1, 9) for b in (8, 16, 24)):
        out[f"flac_{channels}ch_{bits}bit"] = simple([3], init=dict(info=streaminfo(channels=channels, bits=bits, max_block=16), entry_channels=channels, entry_bits=bits), size=40)
    out["flac_more_metadata"] = simple([3], init=dict(dfla_options=dict(more=[(4, b"vorbis comment"), (1, bytes(9))])))
    out["flac_metadata_without_last_flag"] = simple([3], init=dict(dfla_options=dict(more=[(1, bytes(5))], last=False)))
    return out


def named_capacities():
    """-> {name: (Fragmented, run_capacity, packet_capacity)}: more runs than run_capacity, more samples than packet_capacity"""
    varied = mux(init_segment(), [fragment([run(pattern_samples(20, k), [1 + (j + k) % 4 for j in range(20)]), run(pattern_samples(11, k + 9), [7] * 11, data_offset=False)],
                                           sequence=k) for k in range(1, 5)])
    return {"more_runs_than_capacity": (varied, 3, varied.n), "more_samples_than_capacity": (varied, len(varied.runs), 45),
            "both": (varied, 5, 25), "no_room": (varied, 0, 0), "rows_but_no_runs": (varied, 0, 10)}


def limit_edges():
    """-> {name: (Fragmented, the codec's limit)}: the second sample is exactly as large as the codec lets a sample be, the third a byte
    larger (refused, as the fourth is not: a run's samples lie one behind the other whatever becomes of them)"""
    out = {}
    for channels, bits in ((1, 8), (2, 16), (8, 24)):
        limit = 16 * channels * (bits // 8 + 1) + 64
        m = mux(init_segment(info=streaminfo(channels=channels, bits=bits, max_block=16), entry_channels=channels, entry_bits=bits),
                [fragment([run([bytes(5), bytes(limit), bytes(limit + 1), bytes(7)], [16] * 4)])])
        out[f"flac_{channels}ch_{bits}bit"] = (m, limit)
    limit = 4096 * 2 * 5 + 64                      # PATTERN_COOKIE: frame length 4096, stereo
    out["alac"] = (mux(init_segment(ALAC), [fragment([run([bytes(5), bytes(limit), bytes(limit + 1), bytes(7)], [4096] * 4)])], codec=ALAC), limit)
    return out


def patched(m, at, value, width=4):
    return MC.patched(m, at, value, width)


def named_malformed():
    """-> {name: (bytes, status, error_offset, codecs)}: one thing wrong each, for every status and every rule"""
    X = FX
    good = mux(init_segment(trex=(10, 20)), [fragment([run(pattern_samples(5, 1), [10] * 5)], tfdt=(0, 0)), fragment([run(pattern_samples(5, 2), [10] * 5)], sequence=2)], trex=(10, 20))
    moov, trak, tkhd, mdhd, stsd, trex = (good.find(k) for k in ("moov", "trak", "tkhd", "mdhd", "stsd", "trex"))
    moof, traf, tfhd, tfdt, trun = (good.find(k) for k in ("moof", "traf", "tfhd", "tfdt", "trun"))
    moof2, trun2 = good.find("moof", 1), good.find("trun", 1)
    out = {}

    def add(name, data, status, at, codecs=3):
        out[name] = (bytes(data), status, at, codecs)

    def made(status, find, nth=0, at=None, **kw):
        """a file of its own: init_segment(**init) and fragments; the error lies at the nth box called `find`, or where at(file) says"""
        m = mux(init_segment(**kw.pop("init", {})), kw.pop("fragments", [fragment([run(pattern_samples(5, 1), [10] * 5)])]), **kw)
        return m.data, status, (m.find(find, nth)[0] if at is None else at(m))

    add("not_mp4", good.data[:4] + b"RIFF" + good.data[8:], X.NOT_MP4, 0)
    add("seven_bytes", good.data[:7], X.TRUNCATED, 0)
    add("cut_in_moov", good.data[:moov[2] - 40], X.TRUNCATED, moov[0])
    add("no_moov", good.data[:moov[0]], X.TRUNCATED, moov[0])
    add("moof_in_front_of_moov", good.data[:moov[0]] + good.data[moof[0]:moof[2]] + good.data[moov[0]:], X.INVALID, moov[0])
    add("not_codec_mp4a", *made(X.NOT_CODEC, "moov", init=dict(codec=b"mp4a", inner=False)))
    add("flac_asked_alac_there", good.data, X.NOT_CODEC, moov[0], 1)
    add("alac_asked_flac_there", mux(init_segment(ALAC), []).data, X.NOT_CODEC, moov[0], 2)
    add("enca", *made(X.UNSUPPORTED, "stsd", init=dict(codec=b"enca", inner=False), at=lambda m: m.find("stsd")[1] + 8))
    add("not_fragmented", *made(X.NOT_FRAGMENTED, "moov", init=dict(mvex=False, stsz_samples=3), fragments=[]))
    add("flac_entry_of_27_bytes", *made(X.INVALID, "stsd", init=dict(entry=Node(FLAC, bytes(27))), at=lambda m: m.find("stsd")[1] + 8))
    add("no_dfla", *made(X.UNSUPPORTED, "stsd", init=dict(inner=False), at=lambda m: m.find("stsd")[1] + 8))
    add("dfla_version_1", *made(X.UNSUPPORTED, "stsd", init=dict(dfla_options=dict(version_flags=1 << 24)), at=lambda m: dfla_at(m)))
    add("dfla_first_block_not_streaminfo", *made(X.INVALID, "stsd", init=dict(inner=Node(b"dfLa", bytes(4) + bytes([0x84]) + (34).to_bytes(3, "big") + bytes(34))), at=lambda m: dfla_at(m)))
    add("dfla_streaminfo_of_33", *made(X.INVALID, "stsd", init=dict(inner=Node(b"dfLa", bytes(4) + bytes([0x80]) + (33).to_bytes(3, "big") + bytes(33))), at=lambda m: dfla_at(m)))
    add("dfla_block_leaves_the_box", *made(X.INVALID, "stsd", init=dict(dfla_options=dict(more=[(1, bytes(5))])), at=lambda m: dfla_at(m)))
    data = bytearray(out["dfla_block_leaves_the_box"][0])
    at = dfla_at_bytes(data)
    data[at + 8 + 4 + 38 + 1:at + 8 + 4 + 38 + 4] = (6).to_bytes(3, "big")
    out["dfla_block_leaves_the_box"] = (bytes(data), X.INVALID, at, 3)
    add("dfla_empty", *made(X.INVALID, "stsd", init=dict(inner=Node(b"dfLa", bytes(4))), at=lambda m: dfla_at(m)))
    add("dfla_of_3_bytes", *made(X.INVALID, "stsd", init=dict(inner=Node(b"dfLa", bytes(3))), at=lambda m: dfla_at(m)))
    add("flac_12_bit", *made(X.UNSUPPORTED, "stsd", init=dict(info=streaminfo(bits=12)), at=lambda m: dfla_at(m)))
    add("no_tkhd", *made(X.INVALID, "trak", init=dict(drop=("tkhd",))))
    add("no_mdhd", *made(X.INVALID, "trak", init=dict(drop=("mdhd",))))
    add("no_stsd", *made(X.NOT_CODEC, "moov", init=dict(drop=("stsd",))))
    add("tkhd_version_2", patched(good, tkhd[1], 2, 1), X.INVALID, tkhd[0])
    add("mdhd_timescale_0", patched(good, mdhd[1] + 12, 0), X.INVALID, mdhd[0])
    add("trex_short", patched(good, trex[0], 8 + 20), X.INVALID, trex[0])
    add("mehd_version_2", *made(X.INVALID, "mehd", init=dict(mehd=(0, 5))))
    data = bytearray(out["mehd_version_2"][0])
    data[out["mehd_version_2"][2] + 8] = 2
    out["mehd_version_2"] = (bytes(data), X.INVALID, out["mehd_version_2"][2], 3)
    add("box_size_7", patched(good, trak[0], 7), X.INVALID, trak[0])
    add("child_past_parent", patched(good, trun[0], trun[2] - trun[0] + 1), X.INVALID, trun[0])
    add("size_0_inside", patched(good, tfhd[0], 0), X.INVALID, tfhd[0])
    add("traf_without_tfhd", good.data[:tfhd[0] + 4] + b"free" + good.data[tfhd[0] + 8:], X.INVALID, tfdt[0])
    bare = mux(init_segment(), [fragment([])])
    t = bare.find("tfhd")
    add("traf_with_nothing_but_free", bare.data[:t[0] + 4] + b"free" + bare.data[t[0] + 8:], X.INVALID, bare.find("traf")[0])
    add("tfhd_short", patched(good, tfhd[1], 0x20039, 4), X.INVALID, tfhd[0])
    add("tfdt_version_2", patched(good, tfdt[1], 2, 1), X.INVALID, tfdt[0])
    add("trun_entries_leave_the_box", patched(good, trun[1] + 4, 6), X.INVALID, trun[0])
    add("trun_short", patched(good, trun[1], 0x305, 4), X.INVALID, trun[0])
    add("no_size_anywhere", *made(X.INVALID, "trun", fragments=[fragment([run(pattern_samples(3, 1, 9), [10] * 3, fields="duration")], tfhd_size=9)]))
    data = bytearray(out["no_size_anywhere"][0])
    m = mux(init_segment(), [fragment([run(pattern_samples(3, 1, 9), [10] * 3, fields="duration")], tfhd_size=9)])
    t = m.find("tfhd")
    data[t[1] + 1:t[1] + 4] = (0x20020).to_bytes(3, "big")           # the default size becomes default flags
    out["no_size_anywhere"] = (bytes(data), X.INVALID, m.find("trun")[0], 3)
    m = mux(init_segment(), [fragment([run(pattern_samples(3, 1), [10] * 3, fields="size")], tfhd_duration=10)])
    t = m.find("tfhd")
    data = bytearray(m.data)
    data[t[1] + 1:t[1] + 4] = (0x20020).to_bytes(3, "big")
    add("no_duration_anywhere", data, X.INVALID, m.find("trun")[0])
    m = mux(init_segment(other_track="before"), [fragment([run(pattern_samples(3, 1), [10] * 3)], other_traf="before", base="first")])
    add("second_traf_without_a_base", m.data, X.UNSUPPORTED, m.find("tfhd", 1)[0])
    add("too_many_samples_in_a_trun", patched(patched(good, trun2[1] + 4, (1 << 16) + 1), trun2[1], 0x1, 4), X.UNSUPPORTED, trun2[0])
    # 257 truns of 2^16 samples of the trex's size and duration (the entries become slack in the box): the last is one too many
    many = mux(init_segment(trex=(10, 0)), [fragment([run([b"x"], [10])], sequence=k + 1) for k in range(257)], trex=(10, 0))
    data = bytearray(many.data)
    for k in range(257):
        t = many.find("trun", k)
        data[t[1]:t[1] + 8] = struct.pack(">II", 0x1, 1 << 16)
    add("too_many_samples", data, X.UNSUPPORTED, many.find("trun", 256)[0])
    alone = mux(init_segment(), [])          # (its marks: every box the walk counts -- the sample entry's own are counted apart)
    add("too_many_boxes", mux(init_segment(), [], tail=[Node(b"free", b"")] * 65536).data, X.INVALID, len(alone.data) + 8 * (65536 - len(alone.marks)))
    return out


def dfla_at_bytes(data):
    return bytes(data).index(b"dfLa") - 4


def dfla_at(m):
    return dfla_at_bytes(m.data)


def damaged(count, seed=20262):
    """-> [bytes]: fixed-seed damage to good files.  Even k: a word of a fragment's sample data or of a box nothing reads (free, mfhd,
    sidx, styp, hdlr) is overwritten -- such a file stays OK; odd k: a box's size field inside moov or moof is set to 0, 1 or 7, or a
    trun's sample count is inflated past its box -- such a file is refused.  The first k of damaged(n) are damaged(k)."""
    goods = [m for name, m in named_good().items() if m.n and not name.startswith("run_of_1") and not name.startswith("run_of_2")]
    rng = Lcg(seed)
    out = []
    for k in range(count):
        m = goods[rng.next() % len(goods)]
        data = bytearray(m.data)
        if k % 2 == 0:
            quiet = [x for x in m.marks if x[0].split("/")[-1] in ("mdat", "free", "mfhd", "sidx", "styp", "hdlr", "smhd", "mvhd") and x[3] - x[2] >= 4]
            x = quiet[rng.next() % len(quiet)]
            at = x[2] + rng.next() % (x[3] - x[2] - 3)
            data[at:at + 4] = (rng.next() & 0xffffffff).to_bytes(4, "big")
        else:
            inside = [x for x in m.marks if x[0].startswith(("moov/", "moof/"))]
            truns = [x for x in inside if x[0].endswith("/trun")]
            if rng.next() % 3 == 0 and truns:
                x = truns[rng.next() % len(truns)]
                data[x[2] + 4:x[2] + 8] = (0x20000000 + rng.next() % 1000).to_bytes(4, "big")
            else:
                x = inside[rng.next() % len(inside)]
                data[x[1]:x[1] + 4] = (0, 1, 7)[rng.next() % 3].to_bytes(4, "big")
        out.append(bytes(data))
    return out


def check_against_record(model, m, packet_capacity=None, run_capacity=None, src_offset=0):
    """the model's outputs against the muxer's own record (every sample inside the file, none above the limit)"""
    assert model["status"] == FX.OK, model
    rows = m.n if packet_capacity is None else packet_capacity
    assert model["samples"] == m.n and model["runs"] == len(m.runs) and model["track_id"] == m.track_id
    assert model["run_rows"] == m.runs[:len(model["run_rows"])] and (run_capacity is not None or len(model["run_rows"]) == len(m.runs))
    assert model["rows"] == list(zip(m.offsets, m.sizes))[:len(model["rows"])]
    assert model["samples_rows"] == list(zip(m.first_frames, m.frames, m.run_of))[:len(model["rows"])]
    if run_capacity is None:
        assert len(model["rows"]) == min(rows, m.n)
    assert model["frames"] == m.total_frames and model["codec"] == FX.code(m.codec)
    assert model["first_moof_offset"] == (m.find("moof")[0] if m.segment_ends else 0) and model["moov_offset"] == m.find("moov")[0]


# ---- batches
def stream(data, capacity=None, run_capacity=None, codecs=3, gather=True, gather_first_row=0, dst_capacity=None):
    if isinstance(data, Fragmented):
        return dict(data=data.data, capacity=data.n if capacity is None else capacity, run_capacity=len(data.runs) if run_capacity is None else run_capacity,
                    codecs=codecs, gather=gather, gather_first_row=gather_first_row, dst_capacity=len(data.data) if dst_capacity is None else dst_capacity)
    return dict(data=bytes(data), capacity=8 if capacity is None else capacity, run_capacity=4 if run_capacity is None else run_capacity, codecs=codecs,
                gather=gather, gather_first_row=gather_first_row, dst_capacity=len(data) if dst_capacity is None else dst_capacity)


class Job:
    """streams: [stream(...)].  The source arena holds the files one after the other, stream i at an address that is `align(i)` mod
    16, stray bytes between them; the destination arena holds a range a stream at `dst_align(i)` mod 16 with GUARD_BYTES between them.
    All three tables have GUARD_ROWS rows in front of, between and behind the streams' ranges.  `want_*`: the model's outputs with
    0xA5 in every byte no run writes."""

    def __init__(self, streams, align=lambda i: (5 * i + 1) % 16, dst_align=lambda i: (7 * i + 3) % 16):
        from ohpipeline_amd import capi
        self.streams = streams
        src = bytearray()
        self.descs = np.zeros(len(streams), dtype=capi.MP4F_STREAM_DESC)
        row = run_row = GUARD_ROWS
        dst = GUARD_BYTES
        for i, s in enumerate(streams):
            while len(src) % 16 != align(i) % 16:
                src.append(0xee)
            while dst % 16 != dst_align(i) % 16:
                dst += 1
            d = self.descs[i]
            d["src_offset"], d["src_bytes"], d["codecs"], d["flags"] = len(src), len(s["data"]), s["codecs"], 1 if s["gather"] else 0
            d["packet_first"], d["packet_capacity"], d["run_first"], d["run_capacity"] = row, s["capacity"], run_row, s["run_capacity"]
            d["gather_first_row"], d["dst_offset"], d["dst_capacity"] = s["gather_first_row"], dst, s["dst_capacity"]
            src += s["data"]
            row += s["capacity"] + GUARD_ROWS
            run_row += s["run_capacity"] + GUARD_ROWS
            dst += s["dst_capacity"] + GUARD_BYTES
        while len(src) % 4:
            src.append(0xee)
        self.n_packets, self.n_runs, self.dst_bytes = (row, run_row, dst) if streams else (0, 0, 0)
        self.src = np.frombuffer(bytes(src), dtype=np.uint8).copy()
        self.models = [FX.demux(s["data"], s["codecs"], s["capacity"], s["run_capacity"], s["gather"], s["gather_first_row"], s["dst_capacity"]) for s in streams]
        self.want_results = np.zeros(len(streams), dtype=capi.MP4F_STREAM_RESULT)
        self.want_packets = np.frombuffer(bytes([FILL]) * (16 * self.n_packets), dtype=capi.ALAC_PACKET).copy()
        self.want_samples = np.frombuffer(bytes([FILL]) * (16 * self.n_packets), dtype=capi.MP4_SAMPLE).copy()
        self.want_runs = np.frombuffer(bytes([FILL]) * (32 * self.n_runs), dtype=capi.MP4F_RUN).copy()
        self.want_dst = np.full(self.dst_bytes, FILL, dtype=np.uint8)
        for i, (d, m) in enumerate(zip(self.descs, self.models)):
            r = self.want_results[i]
            for k in FX.RESULT_FIELDS:
                r[k] = m[k]
            for k in FX.CONFIG_FIELDS:
                r["config"][k] = m["config"][k]
            for k in FX.FLAC_FIELDS:
                r["flac"][k] = np.frombuffer(m["flac"][k], dtype=np.uint8) if k == "md5" else m["flac"][k]
            first, base = int(d["packet_first"]), int(d["src_offset"])
            for s, (rowm, sm) in enumerate(zip(m["rows"], m["samples_rows"])):
                self.want_packets[first + s] = (base + rowm[0], rowm[1], 0) if rowm else (base, 0, 0)
                self.want_samples[first + s] = sm
            for k, (place, frame, first_sample, samples, total) in enumerate(m["run_rows"]):
                self.want_runs[int(d["run_first"]) + k] = ((base + place) & M64, frame, first_sample, samples, total)
            at = int(d["dst_offset"])
            self.want_dst[at:at + len(m["gathered"])] = np.frombuffer(m["gathered"], dtype=np.uint8)

    def driver_blob(self):
        """the job file of tests/cpp/mp4f_core_driver.cpp"""
        return struct.pack("<QQQQQ", len(self.streams), self.n_packets, self.n_runs, self.src.size, self.dst_bytes) + self.descs.tobytes() + self.src.tobytes()


def assert_same(results, runs, packets, samples, dst, job, what=""):
    assert len(results) == len(job.want_results)
    for i, (got, want) in enumerate(zip(results, job.want_results)):
        if got.tobytes() != want.tobytes():
            diff = {k: (got[k], want[k]) for k in got.dtype.names if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes()}
            raise AssertionError(f"{what} stream {i}: result (got, want) {diff}")
    for name, got, want in (("run", runs, job.want_runs), ("packet", packets, job.want_packets), ("sample", samples, job.want_samples)):
        assert got.size == want.size, (what, name, got.size, want.size)
        if got.tobytes() != want.tobytes():
            k = next(k for k in range(got.size) if got[k].tobytes() != want[k].tobytes())
            raise AssertionError(f"{what} {name} row {k}: got {got[k]}, want {want[k]}")
    assert dst.size == job.want_dst.size
    if not np.array_equal(dst, job.want_dst):
        k = int(np.flatnonzero(dst != job.want_dst)[0])
        raise AssertionError(f"{what} destination byte {k}: got {dst[k]}, want {job.want_dst[k]}")


def cuts(m):
    """every prefix of a file that ends at a box boundary or a byte to either side of one"""
    ends = sorted({b + d for b in m.boundaries() for d in (-1, 0, 1) if 0 <= b + d < len(m.data)})
    return [m.data[:e] for e in ends]
