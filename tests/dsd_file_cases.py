"""What the DSD file tests share: named good and malformed DSF and DFF files (made by tests/dsd_file_textbook.py's writer), prefixes
round every header boundary and inside the planes, and the job -- arenas, descriptors, the model's results and the destination every
route must leave -- with its comparison, and the shape sweep the device test and the CPU driver both run."""
import struct

import numpy as np

import dsd_file_textbook as FX

FILL, GUARD = 0xA5, 48
FORMATS = ((1, 0), (2, 0), (6, 2), (8, 4))
PIECE_CHUNKS = 2048          # dsdfile::kPieceChunks (csrc/dsd_file_core.h): the chunks a wave of the conversion takes
GROUP_PIECES = 2             # kDsdFileGroupPieces (csrc/ohgpu_internal.h): the pieces one workgroup of the conversion takes
UNIT_CHUNKS = 8              # the chunks a lane takes


def planes(chunks, seed):
    """Two channels' streams of `chunks` chunks: 2 x chunks bytes each, the earliest sample in a byte's top bit."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, 2 * chunks, dtype=np.uint8).tobytes(), rng.integers(0, 256, 2 * chunks, dtype=np.uint8).tobytes()


def junk(name, length, seed=7):
    return (name, bytes((seed * 31 + 17 * k + length) % 256 for k in range(length)))


def make(kind, chunks, seed, **kw):
    return (FX.dsf if kind == FX.DSF else FX.dff)(*planes(chunks, seed), **kw)


def named_good():
    p = planes
    return {
        "dsf_100": FX.dsf(*p(100, 1)),
        "dsf_one_pair": FX.dsf(*p(2048, 2), rate=5644800),
        "dsf_fmt_64": FX.dsf(*p(40, 3), fmt_size=64, version=7, channel_type=9),
        "dsf_count_not_16": FX.dsf(*p(50, 4), sample_count=16 * 49 + 9),
        "dsf_metadata_behind": FX.dsf(*p(30, 5), metadata=28 + 52 + 12 + 8192, tail=b"ID3" + bytes(40)),
        "dsf_no_samples": FX.dsf(b"", b""),
        "dsf_total_size_wrong": FX.dsf(*p(20, 6), total=5),
        "dff_100": FX.dff(*p(100, 11)),
        "dff_dsd_first": FX.dff(*p(64, 12), dsd_first=True, between=[junk(b"COMT", 9)], rate=5644800),
        "dff_junk_everywhere": FX.dff(*p(33, 13), before=[junk(b"JUNK", 3)], between=[junk(b"DIIN", 11), junk(b"COMT", 1)], behind=[junk(b"ID3 ", 5)]),
        "dff_odd_local": FX.dff(*p(21, 14), locals_before=[junk(b"ABSS", 7)], locals_after=[junk(b"LSCO", 1)]),
        "dff_no_fver": FX.dff(*p(16, 15), fver=None),
        "dff_no_cmpr": FX.dff(*p(12, 16), omit=(b"CMPR",)),
        "dff_another_prop_first": FX.dff(*p(10, 17), before=[(b"PROP", b"XXX " + bytes(6))]),
        "dff_no_audio": FX.dff(b"", b""),
        "dff_audio_longer_than_file": FX.dff(*p(25, 18), audio_size=4000),
        "dff_dst_behind_dsd": FX.dff(*p(8, 19), dsd_first=True, between=[junk(b"DST ", 6)]),
    }


def patched(w, at, raw):
    data = bytearray(w.data)
    data[at:at + len(raw)] = raw
    return bytes(data)


def many_chunks(count):
    body = b"".join(FX.dff_chunk(b"JUNK", b"") for _ in range(count))
    return b"FRM8" + struct.pack(">Q", 4 + len(body)) + b"DSD " + body


def named_malformed():
    """name -> (bytes, status, the chunk position error_offset must name)"""
    X = FX
    s, f = FX.dsf(*planes(24, 41)), FX.dff(*planes(24, 42))
    fmt, data = s.marks["fmt "], s.marks["data"]
    fver, prop, dsd = f.marks["FVER"], f.marks["PROP"], f.marks["DSD "]
    fs = prop + 16                                   # the first local chunk: FS, then CHNL (2 + 8 bytes), then CMPR
    chnl, cmpr = fs + 16, fs + 16 + 22
    assert f.data[fs:fs + 4] == b"FS  " and f.data[chnl:chnl + 4] == b"CHNL" and f.data[cmpr:cmpr + 4] == b"CMPR"
    u64 = lambda v: struct.pack(">Q", v)
    return {
        "empty": (b"", X.NOT_DSD, 0),
        "fifteen_bytes": (f.data[:15], X.NOT_DSD, 0),
        "riff": (b"RIFF" + bytes(40), X.NOT_DSD, 0),
        "frm8_of_pcm": (patched(f, 12, b"PCM "), X.NOT_DSD, 0),
        "dsd_lower_case": (patched(s, 0, b"dsd "), X.NOT_DSD, 0),
        "dsf_header_cut": (s.data[:27], X.TRUNCATED, 0),
        "dsf_header_of_29": (patched(s, 4, struct.pack("<Q", 29)), X.INVALID, 0),
        "dsf_total_size_0": (FX.dsf(*planes(4, 43), total=0).data, X.INVALID, 0),
        "dsf_fmt_header_cut": (s.data[:39], X.TRUNCATED, fmt),
        "dsf_no_fmt": (patched(s, fmt, b"junk"), X.INVALID, fmt),
        "dsf_fmt_of_51": (patched(s, fmt + 4, struct.pack("<Q", 51)), X.INVALID, fmt),
        "dsf_fmt_of_2_to_31": (patched(s, fmt + 4, struct.pack("<Q", 1 << 31)), X.INVALID, fmt),
        "dsf_fmt_fields_cut": (s.data[:79], X.TRUNCATED, fmt),
        "dsf_format_id_1": (FX.dsf(*planes(4, 44), format_id=1).data, X.UNSUPPORTED, fmt),
        "dsf_mono": (FX.dsf(*planes(4, 45), channels=1).data, X.UNSUPPORTED, fmt),
        "dsf_six_channels": (FX.dsf(*planes(4, 46), channels=6).data, X.UNSUPPORTED, fmt),
        "dsf_rate_0": (FX.dsf(*planes(4, 47), rate=0).data, X.INVALID, fmt),
        "dsf_msb_first": (FX.dsf(*planes(4, 48), bits=8).data, X.UNSUPPORTED, fmt),
        "dsf_block_of_2048": (FX.dsf(*planes(4, 49), block=2048).data, X.UNSUPPORTED, fmt),
        "dsf_data_header_cut": (s.data[:data + 11], X.TRUNCATED, data),
        "dsf_data_beyond_the_file": (patched(s, fmt + 4, struct.pack("<Q", 1 << 20)), X.TRUNCATED, fmt + (1 << 20)),
        "dsf_no_data": (patched(s, data, b"DATA"), X.INVALID, data),
        "dsf_data_of_11": (patched(s, data + 4, struct.pack("<Q", 11)), X.INVALID, data),
        "dsf_data_odd": (patched(s, data + 4, struct.pack("<Q", 12 + 8191)), X.INVALID, data),
        "dsf_more_samples_than_data": (FX.dsf(*planes(24, 50), sample_count=8 * 4096 + 8).data, X.INVALID, data),
        "dff_header_only": (f.data[:16], X.TRUNCATED, 16),
        "dff_chunk_header_cut": (f.data[:prop + 11], X.TRUNCATED, prop),
        "dff_fver_of_5": (patched(f, fver + 4, u64(5)), X.INVALID, fver),
        "dff_fver_cut": (f.data[:fver + 14], X.TRUNCATED, fver),
        "dff_version_2": (FX.dff(*planes(4, 51), fver=b"\x02\0\0\0").data, X.UNSUPPORTED, fver),
        "dff_dst": (FX.dff(*planes(4, 52), audio_id=b"DST ").data, X.UNSUPPORTED, dsd),
        "dff_prop_of_3": (patched(f, prop + 4, u64(3)), X.INVALID, prop),
        "dff_prop_cut": (f.data[:dsd - 1], X.TRUNCATED, prop),
        "dff_local_past_prop": (patched(f, cmpr + 4, u64(400)), X.INVALID, prop),
        "dff_local_header_past_prop": (patched(f, prop + 4, u64(dsd - prop - 12 + 6)), X.INVALID, prop),      # six bytes behind the last local chunk
        "dff_fs_of_8": (patched(f, fs + 4, u64(8)), X.INVALID, prop),
        "dff_rate_0": (FX.dff(*planes(4, 54), rate=0).data, X.INVALID, prop),
        "dff_chnl_of_1": (patched(f, chnl + 4, u64(1)), X.INVALID, prop),
        "dff_mono": (FX.dff(*planes(4, 55), channels=1).data, X.UNSUPPORTED, prop),
        "dff_six_channels": (FX.dff(*planes(4, 56), channels=6).data, X.UNSUPPORTED, prop),
        "dff_cmpr_dst": (FX.dff(*planes(4, 57), cmpr=b"DST ").data, X.UNSUPPORTED, prop),
        "dff_cmpr_of_2": (patched(f, cmpr + 4, u64(2)), X.INVALID, prop),
        "dff_no_fs": (FX.dff(*planes(4, 58), omit=(b"FS  ",)).data, X.INVALID, prop),
        "dff_no_chnl": (FX.dff(*planes(4, 59), omit=(b"CHNL",)).data, X.INVALID, prop),
        "dff_audio_odd": (FX.dff(*planes(4, 60), audio_size=15).data, X.INVALID, dsd),
        "dff_no_audio_chunk": (patched(f, dsd, b"dsd "), X.TRUNCATED, len(f.data)),
        "dff_size_of_2_to_63": (patched(f, fver + 4, u64(1 << 63)), X.INVALID, fver),
        "dff_too_many_chunks": (many_chunks(FX.MAX_CHUNKS + 3), X.INVALID, 16 + 12 * FX.MAX_CHUNKS),
        "dff_too_many_local_chunks": (FX.dff(*planes(4, 61), locals_before=[junk(b"JUNK", 0)] * FX.MAX_CHUNKS).data, X.INVALID, prop + 16 + 12 * (FX.MAX_CHUNKS - 2)),
    }


def cuts(w):
    """Prefixes of a file at every byte round every header boundary, and round the places inside the audio where a chunk's bytes end."""
    ends = set()
    for at in w.marks.values():
        ends.update(range(at - 1, at + 14))
    ends.update((15, 16, 17, 27, 28, 29, 79, 80, 81))
    a = w.data_offset
    inside = (0, 1, 2, 3, 4, 5, 31, 32, 33) if w.kind == FX.DFF else (0, 1, 2, 100, FX.PLANE - 1, FX.PLANE, FX.PLANE + 1, FX.PLANE + 2, FX.PLANE + 3, FX.PLANE + 4,
                                                                      FX.PLANE + 101, FX.PLANE + 2 * w.chunks_total - 1, FX.PLANE + 2 * w.chunks_total)
    ends.update(a + k for k in inside)
    ends.update((len(w.data) - 1, len(w.data)))
    return [w.data[:n] for n in sorted(ends) if 0 <= n <= len(w.data)]


def stream(data, W=2, P=0, *, chunk_first=0, room=None):
    """One stream of a job: a Written or bytes.  room: dst_bytes_capacity (default: exactly what the whole file's chunks take, four
    blocks for bare bytes)."""
    w = data if isinstance(data, FX.Written) else None
    raw = w.data if w else bytes(data)
    if room is None:
        room = -(-w.chunks_total // (W - P)) * W * 4 if w else 4 * W * 4
    return dict(data=raw, W=W, P=P, chunk_first=chunk_first, room=room, written=w)


class Job:
    """Streams laid into a source arena (stream i at an address that is `align(i)` mod 16) and a destination arena (every run at a
    multiple of 16, GUARD bytes of fill in front of, between and behind the runs), the descriptors, the model's results and the
    destination arena as every route must leave it when it starts as FILL."""

    def __init__(self, streams, align=lambda i: (5 * i + 1) % 16):
        from ohpipeline_amd import capi
        self.streams = streams
        self.descs = np.zeros(len(streams), dtype=capi.DSD_FILE_STREAM_DESC)
        src, at = bytearray(), GUARD
        self.models = []
        for i, s in enumerate(streams):
            while len(src) % 16 != align(i):
                src.append(FILL)
            d = self.descs[i]
            d["src_offset"], d["src_bytes"] = len(src), len(s["data"])
            d["dst_offset"], d["dst_bytes_capacity"], d["chunk_first"] = at, s["room"], s["chunk_first"]
            d["sample_block_words"], d["pad_bytes_per_chunk"] = s["W"], s["P"]
            src += s["data"]
            at = (at + s["room"] + GUARD + 15) // 16 * 16
            self.models.append(FX.read(s["data"], s["W"], s["P"], chunk_first=s["chunk_first"], dst_bytes_capacity=s["room"]))
        while len(src) % 4:
            src.append(FILL)
        self.src = np.frombuffer(bytes(src) or b"\0\0\0\0", dtype=np.uint8).copy()
        self.dst_bytes = at
        self.want_dst = np.full(at, FILL, dtype=np.uint8)
        for d, m in zip(self.descs, self.models):
            assert len(m["blocks"]) == m["bytes_written"] <= int(d["dst_bytes_capacity"])
            o = int(d["dst_offset"])
            self.want_dst[o:o + len(m["blocks"])] = np.frombuffer(m["blocks"], dtype=np.uint8)

    def phase(self, i):
        """(src_offset + data_offset) mod 16 of an OK stream: where its audio lies in a 16-byte line of an aligned arena."""
        return (int(self.descs[i]["src_offset"]) + self.models[i]["data_offset"]) % 16

    def driver_blob(self):
        return struct.pack("<QQQ", len(self.streams), self.src.size, self.dst_bytes) + self.descs.tobytes() + self.src.tobytes()


def assert_same(results, dst, job, what=""):
    assert len(results) == len(job.models)
    for i, (r, m) in enumerate(zip(results, job.models)):
        got = {k: int(r[k]) for k in FX.FIELDS}
        assert got == {k: m[k] for k in FX.FIELDS}, (what, i, got, {k: m[k] for k in FX.FIELDS})
    dst = np.asarray(dst)
    if not np.array_equal(dst, job.want_dst):
        at = int(np.flatnonzero(dst != job.want_dst)[0])
        owner = [i for i, d in enumerate(job.descs) if int(d["dst_offset"]) - GUARD <= at < int(d["dst_offset"]) + int(d["dst_bytes_capacity"]) + GUARD]
        raise AssertionError(f"{what}: destination byte {at} is {dst[at]:#x}, the model has {job.want_dst[at]:#x} (streams {owner}, "
                             f"run at {[int(job.descs[i]['dst_offset']) for i in owner]}, phase {[job.phase(i) for i in owner]})")


def has_wide_body(job, i):
    """Whether stream i of an aligned job has, on the fused route, at least one lane of eight chunks that goes through the 16-byte
    loads and stores (restated from the specification: P at most 4, the unit's lines inside the stream, a DSF unit inside one pair)."""
    m, d = job.models[i], job.descs[i]
    if m["status"] != FX.OK or int(d["pad_bytes_per_chunk"]) > 4:
        return False
    base, size, first = int(d["src_offset"]), int(d["src_bytes"]), int(d["chunk_first"])
    for k in range(0, m["chunks_written"] - UNIT_CHUNKS + 1, UNIT_CHUNKS):
        j = first + k
        if m["kind"] == FX.DSF:
            if j % 2048 > 2048 - UNIT_CHUNKS:
                continue
            a = base + m["data_offset"] + j // 2048 * 8192 + j % 2048 * 2
            if a // 16 * 16 + 4096 + 32 <= base + size:
                return True
        elif (base + m["data_offset"] + 4 * j) // 16 * 16 + 48 <= base + size:
            return True
    return False


TOTALS = (0, 1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4101)


def phase_sweep():
    """Every kind and format with the audio at every address mod 16: (src_offset + data_offset) mod 16 takes every value, by the
    arena offset alone for DSF, and for DFF by an odd-sized local chunk in the PROP as well."""
    streams, wanted = [], []
    for kind in (FX.DSF, FX.DFF):
        for W, P in FORMATS:
            for phase in range(16):
                kw = dict(locals_before=[junk(b"ABSS", phase | 1)]) if kind == FX.DFF and phase % 2 else {}
                w = make(kind, 37 + phase, 200 + phase, **kw)
                streams.append(stream(w, W, P))
                wanted.append((phase - w.data_offset) % 16)
    job = Job(streams, align=lambda i: wanted[i])
    assert all(job.phase(i) == i % 16 for i in range(len(streams))) and all(m["status"] == FX.OK and m["chunks_written"] == m["chunks_total"] for m in job.models)
    return job


def shape_sweep():
    """The smallest shapes at which the conversion can go wrong: every chunks_total of TOTALS (round a lane, a piece of 2048 and a
    workgroup's two pieces), a seek to every chunk_first that matters, rooms of no block, one block and exactly the stream, prefixes
    that end inside the left plane, at the plane boundary, inside the right plane and one byte short of a chunk, and every named
    file, good and malformed, beside each other."""
    streams, seed = [], 300
    for kind in (FX.DSF, FX.DFF):
        for f, (W, P) in enumerate(FORMATS):
            for total in TOTALS:
                seed += 1
                streams.append(stream(make(kind, total, seed), W, P))
            seed += 1
            w = make(kind, 2100, seed)
            for first in (0, 1, 2047, 2048, 2050, 2099, 2100, 2101, 1 << 40):
                if first in (0, 1) and f % 2:
                    continue
                streams.append(stream(w, W, P, chunk_first=first))
            seed += 1
            w = make(kind, 45, seed)
            block = W * 4
            whole = -(-45 // (W - P)) * block
            for room in (0, block - 1, block, block + 1, whole - 1, whole, whole + 5 * block):
                streams.append(stream(w, W, P, room=room))
            streams.append(stream(w, W, P, chunk_first=7, room=3 * block))
            a = w.data_offset
            ends = (a + 1, a + 30, a + 4 * 8, a + 4 * 8 + 3, a + 179, a + 180) if kind == FX.DFF else \
                (a + 50, a + FX.PLANE, a + FX.PLANE + 1, a + FX.PLANE + 2, a + FX.PLANE + 33, a + FX.PLANE + 34, a + FX.PLANE + 89, a + FX.PLANE + 90)
            streams += [stream(w.data[:n], W, P, room=whole) for n in ends]
    seed += 1
    two_pairs = FX.dsf(*planes(2100, seed))
    for n in (two_pairs.data_offset + 8192 + 60, two_pairs.data_offset + 8192 + FX.PLANE + 20 * 2 + 1, two_pairs.data_offset + 8192 + FX.PLANE + 51 * 2):
        streams.append(stream(two_pairs.data[:n], 6, 2, room=2100 * 6))
    good, bad = named_good(), named_malformed()
    for k, (data, _, _) in enumerate(bad.values()):
        streams += [stream(list(good.values())[k % len(good)], *FORMATS[k % 4]), stream(data, *FORMATS[(k + 1) % 4])]
    return streams
