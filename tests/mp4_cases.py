"""What the MPEG-4 container tests share: a muxer that wraps Apple Lossless packets (the committed fixtures of tests/alac_cases.py,
or arithmetic patterns) into .m4a files and keeps ITS OWN RECORD of where it put every packet and which audio frame each begins at --
the truth the model and the product are held to, made by no parser --, the named good and malformed files, the fixed-seed damage, and
the batches: the source arena, the descriptors, and what the model (tests/mp4_textbook.py) says both tables and every result must be."""
import struct

import numpy as np

import alac_cases as AC
import alac_textbook as AT
import mp4_textbook as MX

FILL, GUARD_ROWS = 0xa5, 3
Lcg = AC.Lcg


def box(kind, payload, form=32):
    """form 32: the usual header; 64: size 1 and a 64-bit size; 0: size 0, "to the end of the stream" """
    if form == 64:
        return struct.pack(">I4sQ", 1, kind, 16 + len(payload)) + payload
    if form == 0:
        return struct.pack(">I4s", 0, kind) + payload
    return struct.pack(">I4s", 8 + len(payload), kind) + payload


class Node:
    """a box whose content is bytes or a list of Nodes; emit() writes it and notes where it and its payload went"""

    def __init__(self, kind, content, form=32):
        self.kind, self.content, self.form = kind, content, form

    def emit(self, at, marks, path=""):
        head = 16 if self.form == 64 else 8
        name = path + self.kind.decode("latin1")
        mark = [name, at, at + head, 0]
        marks.append(mark)
        if isinstance(self.content, bytes):
            payload = self.content
        else:
            payload, inner = b"", at + head
            for child in self.content:
                piece = child.emit(inner, marks, name + "/")
                payload += piece
                inner += len(piece)
        mark[3] = at + head + len(payload)
        return box(self.kind, payload, self.form)


def full(kind, payload, version=0, form=32):
    return Node(kind, bytes([version, 0, 0, 0]) + payload, form)


class Muxed:
    """data: the file.  offsets / sizes / first_frames / frames / chunk_of: per packet, the muxer's own record.  marks: [name, box start,
    payload start, box end] of every box written, names as paths ("moov/trak/mdia/minf/stbl/stsz")."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def find(self, name, nth=0):
        hits = [m for m in self.marks if m[0].split("/")[-1] == name]
        return hits[nth][1:]

    def boundaries(self):
        return sorted({m[1] for m in self.marks} | {m[3] for m in self.marks})


def chunk_plan(n, per_chunk):
    """per_chunk: samples a chunk as a list, its last value repeated -> (declared, actual) per chunk; only the last chunk may be short"""
    declared, actual, s = [], [], 0
    while s < n:
        want = per_chunk[min(len(declared), len(per_chunk) - 1)]
        declared.append(want)
        actual.append(min(want, n - s))
        s += actual[-1]
    return declared, actual


def sample_entry(kind, channels, bits, rate, children):
    body = bytes(6) + struct.pack(">H", 1) + bytes(8) + struct.pack(">HHHHI", channels, bits, 0, 0, (rate & 0xffff) << 16)
    return Node(kind, body + b"".join(c.emit(0, []) for c in children))


def mux(packets, cookie, *, per_chunk=None, frames=None, co64=False, moov_last=False, uniform=False, free_before_stbl=None, top_free=None,
        other_track=None, mdhd_version=0, moov_form=32, last_form=32, entry_kind=b"alac", gap=3, entry_per_chunk=False, timescale=None,
        stbl_extra=(), moov_extra=(), top_extra=(), drop=(), table_version=0, inner_kind=b"alac", inner_payload=None, stsc_override=None):
    """-> Muxed.  per_chunk: see chunk_plan (default: everything in one chunk).  other_track: None, "before" or "after" -- an mp4a trak
    on that side of the Apple Lossless one.  drop: names of stbl tables or "mdhd" to leave out.  gap: stray bytes in front of every
    chunk in mdat."""
    cfg = AT.parse_config(cookie)
    n = len(packets)
    frames = list(frames) if frames is not None else [cfg["frame_length"]] * n
    declared, actual = chunk_plan(n, per_chunk or [max(n, 1)])
    # mdat: the chunks one after the other, stray bytes in front of each
    payload, offsets, chunk_of, chunk_at, s = bytearray(), [], [], [], 0
    for c, count in enumerate(actual):
        payload += b"\xee" * gap
        chunk_at.append(len(payload))
        for _ in range(count):
            offsets.append(len(payload))
            chunk_of.append(c)
            payload += packets[s]
            s += 1
    first_frames = [sum(frames[:k]) for k in range(n)]
    # stsc: a run for every change of the declared count, or an entry a chunk
    runs = []
    for c, want in enumerate(declared):
        if entry_per_chunk or not runs or runs[-1][1] != want:
            runs.append((c + 1, want))
    if stsc_override is not None:
        runs = stsc_override
    stts = []
    for f in frames:
        if stts and stts[-1][1] == f:
            stts[-1][0] += 1
        else:
            stts.append([1, f])
    sizes = [len(p) for p in packets]
    if uniform:
        assert len(set(sizes)) <= 1
    v = table_version

    def tables(chunk_base):
        out = {}
        inner = inner_payload if inner_payload is not None else bytes(4) + cookie
        out["stsd"] = full(b"stsd", struct.pack(">I", 1) + sample_entry(entry_kind, cfg["channels"], cfg["bit_depth"], cfg["sample_rate"],
                                                                     [Node(b"free", b"pad"), Node(inner_kind, inner)]).emit(0, []))
        out["stts"] = full(b"stts", struct.pack(">I", len(stts)) + b"".join(struct.pack(">II", *e) for e in stts), v)
        out["stsc"] = full(b"stsc", struct.pack(">I", len(runs)) + b"".join(struct.pack(">III", fc, spc, 1) for fc, spc in runs), v)
        if uniform:
            out["stsz"] = full(b"stsz", struct.pack(">II", sizes[0] if sizes else 1, n), v)
        else:
            out["stsz"] = full(b"stsz", struct.pack(">II", 0, n) + b"".join(struct.pack(">I", x) for x in sizes), v)
        if co64:
            out["co"] = full(b"co64", struct.pack(">I", len(chunk_at)) + b"".join(struct.pack(">Q", chunk_base + x) for x in chunk_at), v)
        else:
            out["co"] = full(b"stco", struct.pack(">I", len(chunk_at)) + b"".join(struct.pack(">I", chunk_base + x) for x in chunk_at), v)
        return [out[k] for k in ("stsd", "stts", "stsc", "stsz", "co") if k not in drop] + list(stbl_extra)

    total = sum(frames)
    scale = timescale if timescale is not None else cfg["sample_rate"]
    if mdhd_version == 0:
        mdhd = full(b"mdhd", struct.pack(">IIIIHH", 0, 0, scale, total, 0x55c4, 0))
    else:
        mdhd = full(b"mdhd", struct.pack(">QQIQHH", 0, 0, scale, total, 0x55c4, 0), 1)

    def other():
        esds = Node(b"esds", bytes(20))
        stbl = [full(b"stsd", struct.pack(">I", 1) + sample_entry(b"mp4a", 2, 16, 44100, [esds]).emit(0, [])),
                full(b"stts", struct.pack(">III", 1, 1, 1024)), full(b"stsc", struct.pack(">IIII", 1, 1, 1, 1)),
                full(b"stsz", struct.pack(">III", 0, 1, 4)), full(b"stco", struct.pack(">II", 1, 0))]
        return Node(b"trak", [full(b"tkhd", bytes(80)), Node(b"mdia", [full(b"mdhd", struct.pack(">IIIIHH", 0, 0, 44100, 1024, 0, 0)),
                                                                          Node(b"minf", [Node(b"stbl", stbl)])])])

    def movie(chunk_base):
        minf = [full(b"smhd", bytes(4))]
        if free_before_stbl is not None:
            minf.append(Node(b"free", bytes(free_before_stbl)))
        minf.append(Node(b"stbl", tables(chunk_base)))
        mdia = ([] if "mdhd" in drop else [mdhd]) + [full(b"hdlr", bytes(8) + b"soun" + bytes(13)), Node(b"minf", minf)]
        trak = Node(b"trak", [full(b"tkhd", bytes(80)), Node(b"uuid", bytes(16) + b"private"), Node(b"mdia", mdia)])
        traks = {None: [trak], "before": [other(), trak], "after": [trak, other()]}[other_track]
        udta = Node(b"udta", [full(b"meta", Node(b"ilst", b"").emit(0, []))])
        return Node(b"moov", [full(b"mvhd", bytes(96))] + list(moov_extra) + traks + [udta], moov_form)

    head = [Node(b"ftyp", b"M4A \x00\x00\x02\x00isomiso2")]
    if top_free is not None:
        head.append(Node(b"free", bytes(top_free)))
    head += list(top_extra)
    marks, data, at = [], b"", 0
    for node in head:
        piece = node.emit(at, marks)
        data += piece
        at += len(piece)
    mdat = Node(b"mdat", bytes(payload), last_form if moov_last is False else 32)
    if moov_last:
        base = at + 8
        mdat_bytes = mdat.emit(at, marks)
        moov_node = movie(base)
        moov_node.form = last_form if last_form != 32 else moov_form
        data += mdat_bytes + moov_node.emit(at + len(mdat_bytes), marks)
    else:
        size = len(movie(0).emit(0, []))
        base = at + size + (16 if mdat.form == 64 else 8)
        data += movie(base).emit(at, marks)
        data += mdat.emit(at + size, marks)
    return Muxed(data=data, offsets=[base + x for x in offsets], sizes=sizes, first_frames=first_frames, frames=frames, chunk_of=chunk_of,
                 marks=marks, n=n, chunks=len(chunk_at), cfg=cfg, total_frames=total, timescale=scale)


def fixture_file(fx, **kw):
    """an Apple Lossless fixture as a file; the last packet carries what is left of the fixture's frames"""
    fl, total = fx["cfg"]["frame_length"], fx["meta"]["frames"]
    n = len(fx["packets"])
    frames = [fl] * (n - 1) + [total - fl * (n - 1)]
    return mux(fx["packets"], fx["cookie"], frames=frames, **kw)


CHUNKINGS = {"one_chunk": [1 << 20], "one_a_chunk": [1], "three_short_last": [3], "changing": [1, 2, 1]}
PATTERN_COOKIE = bytes.fromhex("00001000" "00" "10" "28" "0a" "0e" "02" "00ff" "00000000" "00000000" "0000ac44")   # frame length 4096, stereo 16


def pattern_packets(n, seed=1):
    """n packets of 1 to 90 bytes, arithmetic patterns: nothing decodes them"""
    rng = Lcg(seed)
    return [bytes((k * 7 + j * 13 + seed) & 0xff for j in range(1 + rng.next() % 90)) for k in range(n)]


def patched(m, at, value, width=4):
    data = bytearray(m.data if isinstance(m, Muxed) else m)
    data[at:at + width] = value.to_bytes(width, "big")
    return bytes(data)


def named_good():
    """-> {name: Muxed}: every way a good file is written"""
    fx = AC.load_fixture("stereo16_fl1024")
    six = AC.load_fixture("six16_fl256")
    out = {}
    for name, per_chunk in CHUNKINGS.items():
        out[name] = fixture_file(fx, per_chunk=per_chunk)
    out["co64"] = fixture_file(fx, co64=True, per_chunk=[2])
    out["moov_last"] = fixture_file(fx, moov_last=True, per_chunk=[3])
    out["moov_last_co64"] = fixture_file(six, moov_last=True, co64=True)
    out["box_size_64"] = fixture_file(fx, moov_form=64)
    out["size_0_last"] = fixture_file(fx, last_form=0)
    out["size_0_last_moov"] = fixture_file(fx, moov_last=True, last_form=0)
    out["uniform_stsz"] = mux([bytes([k] * 40) for k in range(9)], PATTERN_COOKIE, uniform=True, per_chunk=[4])
    out["two_tracks_alac_second"] = fixture_file(fx, other_track="before")
    out["two_tracks_alac_first"] = fixture_file(fx, other_track="after")
    out["mdhd_version_1"] = fixture_file(fx, mdhd_version=1)
    out["entry_per_chunk"] = mux(pattern_packets(11), PATTERN_COOKIE, per_chunk=[2, 3, 2, 3, 1], entry_per_chunk=True)
    out["free_everywhere"] = fixture_file(fx, top_free=5, free_before_stbl=2, stbl_extra=[Node(b"free", b"x")], moov_extra=[Node(b"free", b"")])
    out["no_samples"] = mux([], PATTERN_COOKIE)
    return out


def named_malformed():
    """-> {name: (bytes, status, codec or None)}: one thing wrong each"""
    fx = AC.load_fixture("stereo16_fl1024")
    good = fixture_file(fx, per_chunk=[2])
    stsc, stts, stsz, stco = (good.find(k) for k in ("stsc", "stts", "stsz", "stco"))
    mdhd, moov, trak, stsd = (good.find(k) for k in ("mdhd", "moov", "trak", "stsd"))
    X = MX
    out = {}
    out["not_mp4"] = (good.data[:4] + b"RIFF" + good.data[8:], X.NOT_MP4, None)
    out["seven_bytes"] = (good.data[:7], X.TRUNCATED, None)
    out["cut_in_moov"] = (good.data[:moov[2] - 40], X.TRUNCATED, None)
    out["no_moov"] = (good.data[:moov[0]], X.TRUNCATED, None)
    out["mp4a_only"] = (fixture_file(fx, entry_kind=b"mp4a").data, X.NOT_ALAC, b"mp4a")
    out["no_trak"] = (box(b"ftyp", b"M4A ") + box(b"moov", box(b"mvhd", bytes(100))), X.NOT_ALAC, b"\0\0\0\0")
    out["enca"] = (fixture_file(fx, entry_kind=b"enca").data, X.UNSUPPORTED, None)
    out["mvex"] = (fixture_file(fx, moov_extra=[Node(b"mvex", bytes(8))]).data, X.UNSUPPORTED, None)
    out["moof"] = (fixture_file(fx, top_extra=[Node(b"moof", bytes(8))]).data, X.UNSUPPORTED, None)
    out["stz2"] = (fixture_file(fx, stbl_extra=[full(b"stz2", bytes(8))]).data, X.UNSUPPORTED, None)
    out["compatible_version_1"] = (fixture_file(fx, inner_payload=bytes(4) + fx["cookie"][:4] + b"\x01" + fx["cookie"][5:]).data, X.UNSUPPORTED, None)
    out["config_short"] = (fixture_file(fx, inner_payload=bytes(4) + fx["cookie"][:23]).data, X.UNSUPPORTED, None)
    out["no_config"] = (fixture_file(fx, inner_kind=b"wave").data, X.UNSUPPORTED, None)
    out["nine_channels"] = (fixture_file(fx, inner_payload=bytes(4) + fx["cookie"][:9] + b"\x09" + fx["cookie"][10:]).data, X.UNSUPPORTED, None)
    out["too_many_samples"] = (patched(good, stsz[1] + 8, (1 << 24) + 1), X.INVALID, None)          # (the count no longer fits the box)
    out["too_many_uniform"] = (patched(patched(good, stsz[1] + 4, 40), stsz[1] + 8, (1 << 24) + 1), X.UNSUPPORTED, None)
    out["box_size_7"] = (patched(good, trak[0], 7), X.INVALID, None)
    out["child_past_parent"] = (patched(good, stsd[0], stsd[2] - stsd[0] + 1000), X.INVALID, None)
    out["size_0_inside"] = (patched(good, stts[0], 0), X.INVALID, None)
    out["size_64_cut_inside"] = (fixture_file(fx, stbl_extra=[RawNode(struct.pack(">I4sI", 1, b"free", 0))]).data, X.INVALID, None)
    out["timescale_0"] = (patched(good, mdhd[1] + 12, 0), X.INVALID, None)
    out["mdhd_version_2"] = (patched(good, mdhd[1], 2, 1), X.INVALID, None)
    out["stsc_first_chunk_2"] = (patched(good, stsc[1] + 8, 2), X.INVALID, None)
    out["stsc_not_ascending"] = (fixture_file(fx, stsc_override=[(1, 1), (1, 3)], per_chunk=[2]).data, X.INVALID, None)
    out["stsc_beyond_chunks"] = (fixture_file(fx, stsc_override=[(1, 1), (3, 3)], per_chunk=[2]).data, X.INVALID, None)
    out["stsc_none_a_chunk"] = (patched(good, stsc[1] + 12, 0), X.INVALID, None)
    out["stsc_covers_too_few"] = (patched(good, stsc[1] + 12, 1), X.INVALID, None)
    out["stsc_empty"] = (fixture_file(fx, stsc_override=[]).data, X.INVALID, None)
    out["stts_covers_too_few"] = (patched(good, stts[1] + 8, 2), X.INVALID, None)
    out["stts_run_of_none"] = (patched(good, stts[1] + 8, 0), X.INVALID, None)
    out["table_version_1"] = (fixture_file(fx, table_version=1).data, X.INVALID, None)
    out["count_inflated"] = (patched(good, stco[1] + 4, 1000), X.INVALID, None)
    out["no_stco"] = (fixture_file(fx, drop=("co",)).data, X.INVALID, None)
    out["no_mdhd"] = (fixture_file(fx, drop=("mdhd",)).data, X.INVALID, None)
    out["too_many_boxes"] = (fixture_file(fx, top_extra=[Node(b"free", b"")] * 4096).data, X.INVALID, None)
    return out


class RawNode(Node):
    """bytes that are written as they are, where a box should stand"""

    def __init__(self, raw):
        self.raw = raw

    def emit(self, at, marks, path=""):
        return self.raw


def damaged(count, seed=20261):
    """-> [bytes]: fixed-seed damage to the moov of good files -- bit flips, size fields set to 0, 1, 7, 2^31 and 2^32 - 1, entry counts
    inflated.  The first k of damaged(n) are damaged(k)."""
    goods = [m for name, m in named_good().items() if name != "no_samples"]
    rng = Lcg(seed)
    out = []
    for k in range(count):
        m = goods[rng.next() % len(goods)]
        moov = m.find("moov")
        inside = [x for x in m.marks if moov[0] <= x[1] and x[3] <= moov[2]]
        data = bytearray(m.data)
        kind = k % 4
        if kind == 0:                                   # bit flips anywhere in moov
            for _ in range(1 + rng.next() % 3):
                bit = moov[0] * 8 + rng.next() % ((moov[2] - moov[0]) * 8)
                data[bit >> 3] ^= 0x80 >> (bit & 7)
        elif kind == 1:                                 # a box's size field
            x = inside[rng.next() % len(inside)]
            data[x[1]:x[1] + 4] = (0, 1, 7, 1 << 31, (1 << 32) - 1)[rng.next() % 5].to_bytes(4, "big")
        elif kind == 2:                                 # a table's entry count
            name = ("stts", "stsc", "stsz", "stco", "co64", "stsd")[rng.next() % 6]
            hits = [x for x in inside if x[0].endswith("/" + name)]
            if hits:
                at = hits[0][2] + (8 if name == "stsz" else 4)
                now = int.from_bytes(data[at:at + 4], "big")
                data[at:at + 4] = ((now + 1 + rng.next() % 3) if rng.next() % 2 else (now << (1 + rng.next() % 24)) & 0xffffffff).to_bytes(4, "big")
        else:                                           # a word of a table's entries
            name = ("stts", "stsc", "stsz", "stco", "co64", "mdhd")[rng.next() % 6]
            hits = [x for x in inside if x[0].endswith("/" + name)]
            if hits and hits[0][3] - hits[0][2] >= 12:
                at = hits[0][2] + 8 + 4 * (rng.next() % ((hits[0][3] - hits[0][2] - 8) // 4))
                data[at:at + 4] = (0, 1, 2, 0x7fffffff, 0xffffffff, rng.next())[rng.next() % 6].to_bytes(4, "big")
        out.append(bytes(data))
    return out


def check_against_record(model, m, src_offset=0):
    """the model's rows against the muxer's own record (every packet inside the file, none above the limit)"""
    assert model["status"] == MX.OK and model["samples"] == m.n and model["chunks"] == m.chunks
    assert [row for row in model["rows"]] == list(zip(m.offsets, m.sizes))[:len(model["rows"])]
    assert model["samples_rows"] == list(zip(m.first_frames, m.frames, m.chunk_of))[:len(model["rows"])]
    assert model["frames"] == m.total_frames == model["duration"] and model["timescale"] == m.timescale
    assert model["config"] == {k: m.cfg.get(k, 0) for k in MX.CONFIG_FIELDS} | {"compatible_version": 0}
    assert (model["entry_channels"], model["entry_bits"], model["entry_rate"]) == (m.cfg["channels"], m.cfg["bit_depth"], m.cfg["sample_rate"] & 0xffff)


# ---- batches
def stream(data, capacity=None):
    if isinstance(data, Muxed):
        return dict(data=data.data, capacity=data.n if capacity is None else capacity)
    return dict(data=bytes(data), capacity=8 if capacity is None else capacity)


class Job:
    """streams: [stream(...)].  The source arena holds the files one after the other, stream i at an address that is `align(i)` mod 16,
    stray bytes between them and none behind the last.  Both tables have GUARD_ROWS rows in front of, between and behind the streams'
    ranges; `want_packets` / `want_samples` are the model's tables with 0xA5 in every byte no run writes, `want_results` its results."""

    def __init__(self, streams, align=lambda i: (5 * i + 1) % 16):
        from ohpipeline_amd import capi
        self.streams = streams
        src = bytearray()
        self.descs = np.zeros(len(streams), dtype=capi.MP4_STREAM_DESC)
        row = GUARD_ROWS
        for i, s in enumerate(streams):
            while len(src) % 16 != align(i) % 16:
                src.append(0xee)
            self.descs[i]["src_offset"], self.descs[i]["src_bytes"] = len(src), len(s["data"])
            self.descs[i]["packet_first"], self.descs[i]["packet_capacity"] = row, s["capacity"]
            src += s["data"]
            row += s["capacity"] + GUARD_ROWS
        self.n_packets = row if streams else 0
        self.src = np.frombuffer(bytes(src), dtype=np.uint8).copy()
        self.models = [MX.demux(s["data"], s["capacity"]) for s in streams]
        self.want_results = np.zeros(len(streams), dtype=capi.MP4_STREAM_RESULT)
        self.want_packets = np.frombuffer(bytes([FILL]) * (16 * self.n_packets), dtype=capi.ALAC_PACKET).copy()
        self.want_samples = np.frombuffer(bytes([FILL]) * (16 * self.n_packets), dtype=capi.MP4_SAMPLE).copy()
        for i, (d, m) in enumerate(zip(self.descs, self.models)):
            r = self.want_results[i]
            for k in MX.RESULT_FIELDS:
                r[k] = m[k]
            for k in MX.CONFIG_FIELDS:
                r["config"][k] = m["config"][k]
            first, base = int(d["packet_first"]), int(d["src_offset"])
            for s, (rowm, sm) in enumerate(zip(m["rows"], m["samples_rows"])):
                self.want_packets[first + s] = (base + rowm[0], rowm[1], 0) if rowm else (base, 0, 0)
                self.want_samples[first + s] = sm

    def driver_blob(self):
        """the job file of tests/cpp/mp4_core_driver.cpp"""
        return struct.pack("<QQQ", len(self.streams), self.n_packets, self.src.size) + self.descs.tobytes() + self.src.tobytes()


def assert_same(results, packets, samples, job, what=""):
    for i, (got, want) in enumerate(zip(results, job.want_results)):
        if got.tobytes() != want.tobytes():
            diff = {k: (got[k], want[k]) for k in got.dtype.names if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes()}
            raise AssertionError(f"{what} stream {i}: result (got, want) {diff}")
    assert len(results) == len(job.want_results)
    for name, got, want in (("packet", packets, job.want_packets), ("sample", samples, job.want_samples)):
        assert got.size == want.size, (what, name, got.size, want.size)
        if got.tobytes() != want.tobytes():
            k = next(k for k in range(got.size) if got[k].tobytes() != want[k].tobytes())
            raise AssertionError(f"{what} {name} row {k}: got {got[k]}, want {want[k]}")


def cuts(m):
    """every prefix of a file that ends at a box boundary or a byte to either side of one"""
    ends = sorted({b + d for b in m.boundaries() for d in (-1, 0, 1) if 0 <= b + d < len(m.data)})
    return [m.data[:e] for e in ends]
