"""An independent model of the fragmented MPEG-4 layer (ohgpu_mp4f_*, include/ohgpu.h's section) with the simplest means there are:
the boxes by recursion into Python lists, every fragment's samples one after the other with a running file offset and a running frame
count, the gather as a join of slices.  No prefix sums, no searches, no records of runs to be summed later: it shares no algorithm
with csrc/mp4_frag_core.h, and none of its text.  It shares nothing with the muxer of tests/mp4f_cases.py either.

demux(data, codecs=3, packet_capacity, run_capacity, gather, gather_first_row, dst_capacity, head_only) -> dict: the fields of
ohgpu_mp4f_stream_result by name (config and flac as dicts), and
    rows          [(file offset, bytes) or None for a refused sample], the first min(samples of the written runs, packet_capacity)
    samples_rows  [(first_frame, frames, run)] of the same
    run_rows      [(place from the file's first byte -- may be negative --, first_frame, first_sample, samples, bytes)]
    gathered      the bytes the gather writes (b"" where it writes none)

Where this reading differs from the reference's (OpenHome/Media/Codec/Mpeg4.cpp; include/ohgpu.h carries the same list):
  - the reference plays a fragment only when its data begins right behind its moof; here a run lies wherever its offsets say;
  - the reference ignores trex, tfdt and the entries' durations; here they give every sample its frames;
  - the reference refuses a run of no samples; here it is passed over;
  - the reference cannot seek in a fragmented stream; here the sample rows serve ohgpu_mp4_seek;
  - the reference takes sidx for its seek table; here sidx is skipped."""
import mp4_textbook as MX

OK, NOT_MP4, TRUNCATED, INVALID, NOT_CODEC, UNSUPPORTED, NOT_FRAGMENTED = range(7)
MAX_SAMPLES, MAX_RUN_SAMPLES, MAX_BOXES, ENTRY_BOXES, NO_SAMPLE = 1 << 24, 1 << 16, 65536, 4096, 0xffffffff
CODEC_ALAC, CODEC_FLAC = 1, 2
FAR, M64 = 1 << 62, (1 << 64) - 1
CONFIG_FIELDS = MX.CONFIG_FIELDS
FLAC_FIELDS = ("min_blocksize", "max_blocksize", "sample_rate", "channels", "bits", "total_samples", "md5", "min_framesize", "max_framesize")
RESULT_FIELDS = ("status", "codec", "track_id", "timescale", "duration", "frames", "samples", "runs", "samples_available", "samples_refused",
                 "first_bad_sample", "entry_rate", "entry_channels", "entry_bits", "bytes_gathered", "moov_offset", "first_moof_offset", "error_offset")
Refuse, u, code = MX.Refuse, MX.u, MX.code


class Counter:
    def __init__(self, most):
        self.seen, self.most = 0, most


def boxes(data, at, end, counter):
    """the child boxes of [at, end): (kind, box start, payload start, box end), each counted as it is read"""
    while end - at >= 8:
        size, kind, head = u(data, at, 4), data[at + 4:at + 8], 8
        counter.seen += 1
        if counter.seen > counter.most:
            raise Refuse(INVALID, at)
        if size == 1:
            if end - at < 16:
                raise Refuse(INVALID, at)
            size, head = u(data, at + 8, 8), 16
        if size < head or at + size > end:
            raise Refuse(INVALID, at)
        yield kind, at, at + head, at + size
        at += size


def versioned(data, box, pay, end, short, long):
    """a full box of version 0 (at least `short` bytes) or 1 (`long`) -> the version"""
    if end - pay < 4 or data[pay] > 1 or end - pay < (short, long)[data[pay]]:
        raise Refuse(INVALID, box)
    return data[pay]


class Reader:
    def __init__(self, data, codecs, head_only):
        self.data, self.codecs, self.head_only = data, codecs, head_only
        self.counter = Counter(MAX_BOXES)
        self.track = self.first_codec = self.moov = self.first_moof = None
        self.mvex = False
        self.moofs = 0
        self.runs = []                  # dicts: place (None: behind its predecessor), time (None: where the last run ended), entries [(size, frames)]
        self.samples = 0

    def file(self):
        data, n = self.data, len(self.data)
        if n < 8:
            raise Refuse(TRUNCATED, 0)
        if data[4:8] != b"ftyp":
            raise Refuse(NOT_MP4, 0)
        at = 0
        while n - at >= 8:
            size, kind, head = u(data, at, 4), data[at + 4:at + 8], 8
            if size == 1 and n - at < 16:
                break
            self.counter.seen += 1
            if self.counter.seen > MAX_BOXES:
                raise Refuse(INVALID, at)
            if size == 1:
                size, head = u(data, at + 8, 8), 16
            elif size == 0:
                size = n - at
            if size < head:
                raise Refuse(INVALID, at)
            end = at + size
            if kind == b"moov" and self.moov is None:
                if end > n:
                    raise Refuse(TRUNCATED, at)
                self.moov = at
                self.movie(at, at + head, end)
                if self.head_only:
                    break
            elif kind == b"moof":
                if self.moov is None:
                    raise Refuse(INVALID, at)
                if end > n:
                    break
                if self.first_moof is None:
                    self.first_moof = at
                self.moofs += 1
                self.fragment(at, at + head, end)
            elif end > n:
                break
            at = end
        if self.moov is None:
            raise Refuse(TRUNCATED, at)
        if not self.mvex and not self.moofs and self.track["stsz"]:
            raise Refuse(NOT_FRAGMENTED, self.moov)

    # ---- moov
    def movie(self, box, at, end):
        mvex = None
        for kind, child, pay, child_end in boxes(self.data, at, end, self.counter):
            if kind == b"trak" and self.track is None:
                t = self.trak(child, pay, child_end)
                if self.first_codec is None:
                    self.first_codec = t["codec"]
                bit = {code(b"alac"): CODEC_ALAC, code(b"fLaC"): CODEC_FLAC}.get(t["codec"], 0)
                self.last = t
                if bit & self.codecs:
                    if "track_id" not in t or "mdhd" not in t or not t.get("parsed"):
                        raise Refuse(INVALID, child)
                    self.track = t
            elif kind == b"mvex" and mvex is None:
                mvex = (pay, child_end)
        if self.track is None:
            raise Refuse(NOT_CODEC, box)
        self.trex = self.mehd = None
        if mvex:                                      # (read here, at moov's end: the track is known by now)
            self.mvex = True
            data = self.data
            for kind, child, pay, child_end in boxes(data, mvex[0], mvex[1], self.counter):
                if kind == b"trex" and self.trex is None:
                    if child_end - pay < 24:
                        raise Refuse(INVALID, child)
                    if u(data, pay + 4, 4) == self.track["track_id"]:
                        self.trex = (u(data, pay + 12, 4), u(data, pay + 16, 4))          # (duration, size)
                elif kind == b"mehd" and self.mehd is None:
                    v = versioned(data, child, pay, child_end, 8, 12)
                    self.mehd = u(data, pay + 4, 8 if v else 4)

    def trak(self, box, at, end):
        data, t = self.data, {"codec": 0, "stsz": 0}
        for kind, child, pay, child_end in boxes(data, at, end, self.counter):
            if kind == b"tkhd" and "track_id" not in t:
                t["track_id"] = None
                v = versioned(data, child, pay, child_end, 16, 24)
                t["track_id"] = u(data, pay + (20 if v else 12), 4)
            if kind != b"mdia":
                continue
            for kind2, child2, pay2, end2 in boxes(data, pay, child_end, self.counter):
                if kind2 == b"mdhd" and "mdhd" not in t:
                    t["mdhd"] = None
                    v = versioned(data, child2, pay2, end2, 20, 32)
                    t["mdhd"] = (u(data, pay2 + 20, 4), u(data, pay2 + 24, 8)) if v else (u(data, pay2 + 12, 4), u(data, pay2 + 16, 4))
                    if t["mdhd"][0] == 0:
                        raise Refuse(INVALID, child2)
                if kind2 != b"minf":
                    continue
                for kind3, _, pay3, end3 in boxes(data, pay2, end2, self.counter):
                    if kind3 != b"stbl":
                        continue
                    for kind4, child4, pay4, end4 in boxes(data, pay3, end3, self.counter):
                        if kind4 == b"stsd" and "stsd" not in t:
                            t["stsd"] = child4
                            self.description(t, child4, pay4, end4)
                        elif kind4 == b"stsz" and "stsz_seen" not in t:
                            t["stsz_seen"] = True
                            if end4 - pay4 >= 12:
                                t["stsz"] = u(data, pay4 + 8, 4)
        return t

    def description(self, t, box, pay, end):
        data = self.data
        if end - pay < 8 or data[pay] != 0 or u(data, pay + 4, 4) > end - pay - 8:
            raise Refuse(INVALID, box)
        if u(data, pay + 4, 4) == 0:
            return
        inner = Counter(ENTRY_BOXES)                   # the boxes of a sample description have a counter of their own
        entry = pay + 8
        got = next(boxes(data, entry, end, inner), None)
        if got is None:
            raise Refuse(INVALID, entry)
        kind, _, body, entry_end = got
        t["codec"] = code(kind)
        if kind == b"enca":
            raise Refuse(UNSUPPORTED, entry)
        if kind == b"alac":                            # the plain layout's reading of it, whatever the mask
            r = MX.Reader(data, 0)
            r.headers = 0
            track = {}
            r.description(track, box, pay, end)
            t.update(entry=track["entry"], config=track["config"], parsed=True)
            t["limit"] = track["config"]["frame_length"] * track["config"]["channels"] * 5 + 64
            return
        if kind != b"fLaC" or not self.codecs & CODEC_FLAC:
            return
        if entry_end - body < 28:
            raise Refuse(INVALID, entry)
        t["entry"] = (u(data, body + 16, 2), u(data, body + 18, 2), u(data, body + 24, 2))
        for kind, child, cpay, cend in boxes(data, body + 28, entry_end, inner):
            if kind != b"dfLa":
                continue
            t["parsed"] = True
            if cend - cpay < 4:
                raise Refuse(INVALID, child)
            if u(data, cpay, 4) != 0:
                raise Refuse(UNSUPPORTED, child)
            at, first = cpay + 4, True
            while True:
                if cend - at < 4 or u(data, at + 1, 3) > cend - at - 4:
                    raise Refuse(INVALID, child)
                last, kind_, length = data[at] >> 7, data[at] & 0x7f, u(data, at + 1, 3)
                if first:
                    if kind_ != 0 or length != 34:
                        raise Refuse(INVALID, child)
                    bits = u(data, at + 4, 34)                     # the 272 bits of STREAMINFO as one number
                    f = {"md5": bits & ((1 << 128) - 1)}
                    bits >>= 128
                    for name, width in (("total_samples", 36), ("bits", 5), ("channels", 3), ("sample_rate", 20), ("max_framesize", 24),
                                        ("min_framesize", 24), ("max_blocksize", 16), ("min_blocksize", 16)):
                        f[name] = bits & ((1 << width) - 1)
                        bits >>= width
                    f["bits"] += 1
                    f["channels"] += 1
                    f["md5"] = f["md5"].to_bytes(16, "big")
                    if f["bits"] not in (8, 16, 24):
                        raise Refuse(UNSUPPORTED, child)
                    t["flac"] = f
                    t["limit"] = f["max_blocksize"] * f["channels"] * (f["bits"] // 8 + 1) + 64
                    first = False
                at += 4 + length
                if last or at == cend:
                    return
        raise Refuse(UNSUPPORTED, entry)

    # ---- moof
    def fragment(self, moof, at, end):
        data, trafs = self.data, 0
        for kind, traf, pay, traf_end in boxes(data, at, end, self.counter):
            if kind != b"traf":
                continue
            trafs += 1
            head = None                 # None: no tfhd yet; False: another track's; else a dict
            first_run, time = True, None
            for kind2, child, pay2, end2 in boxes(data, pay, traf_end, self.counter):
                if kind2 == b"tfhd" and head is None:
                    head = self.fragment_header(child, pay2, end2, moof, trafs == 1)
                    continue
                if kind2 not in (b"tfdt", b"trun"):
                    continue
                if head is None:
                    raise Refuse(INVALID, child)
                if head is False:
                    continue
                if kind2 == b"tfdt":
                    if first_run and time is None:
                        v = versioned(data, child, pay2, end2, 8, 12)
                        time = u(data, pay2 + 4, 8 if v else 4)
                    continue
                run = self.run(child, pay2, end2, head)
                if run is None:
                    continue
                if run["offset"] is not None:
                    run["place"] = head["base"] + run["offset"]
                elif first_run:
                    run["place"] = head["base"]
                else:
                    run["place"] = None
                run["time"] = time if first_run else None
                first_run = False
                self.runs.append(run)
            if head is None:
                raise Refuse(INVALID, traf)

    def fragment_header(self, box, pay, end, moof, first_traf):
        data = self.data
        if end - pay < 8:
            raise Refuse(INVALID, box)
        flags, at = u(data, pay + 1, 3), pay + 8
        fields = {}
        for bit, width in ((0x1, 8), (0x2, 4), (0x8, 4), (0x10, 4), (0x20, 4)):
            if flags & bit:
                if end - at < width:
                    raise Refuse(INVALID, box)
                fields[bit] = u(data, at, width)
                at += width
        if u(data, pay + 4, 4) != self.track["track_id"]:
            return False
        if 0x1 not in fields and not flags & 0x20000 and not first_traf:
            raise Refuse(UNSUPPORTED, box)
        head = {"base": min(fields[0x1], FAR) if 0x1 in fields else moof}
        head["duration"] = fields.get(0x8, self.trex[0] if self.trex else None)
        head["size"] = fields.get(0x10, self.trex[1] if self.trex else None)
        return head

    def run(self, box, pay, end, head):
        data = self.data
        if end - pay < 8:
            raise Refuse(INVALID, box)
        flags, count, at = u(data, pay + 1, 3), u(data, pay + 4, 4), pay + 8
        offset = None
        if flags & 0x1:
            if end - at < 4:
                raise Refuse(INVALID, box)
            offset = int.from_bytes(data[at:at + 4], "big", signed=True)
            at += 4
        if flags & 0x4:
            if end - at < 4:
                raise Refuse(INVALID, box)
            at += 4
        wide = sum(4 for bit in (0x100, 0x200, 0x400, 0x800) if flags & bit)
        if count * wide > end - at:
            raise Refuse(INVALID, box)
        if count == 0:
            return None
        if (not flags & 0x200 and head["size"] is None) or (not flags & 0x100 and head["duration"] is None):
            raise Refuse(INVALID, box)
        if count > MAX_RUN_SAMPLES or self.samples + count > MAX_SAMPLES:
            raise Refuse(UNSUPPORTED, box)
        self.samples += count
        if wide == 0:
            return dict(offset=offset, count=count, same=(head["size"], head["duration"]))
        entries = []
        for k in range(count):
            e = at + k * wide
            duration = head["duration"]
            if flags & 0x100:
                duration = u(data, e, 4)
                e += 4
            entries.append((u(data, e, 4) if flags & 0x200 else head["size"], duration))
        return dict(offset=offset, count=count, entries=entries)


def run_entries(run):
    return run["entries"] if "entries" in run else [run["same"]] * run["count"]


def demux(data, codecs=3, packet_capacity=1 << 20, run_capacity=1 << 20, gather=False, gather_first_row=0, dst_capacity=0, head_only=False):
    data = bytes(data)
    r = Reader(data, codecs, head_only)
    out = dict.fromkeys(RESULT_FIELDS, 0)
    out.update(config=dict.fromkeys(CONFIG_FIELDS, 0), flac=dict.fromkeys(FLAC_FIELDS, 0) | {"md5": bytes(16)}, first_bad_sample=NO_SAMPLE,
               rows=[], samples_rows=[], run_rows=[], gathered=b"")
    try:
        r.file()
    except Refuse as e:
        codec = (r.first_codec or 0) if e.status == NOT_CODEC else r.track["codec"] if e.status == NOT_FRAGMENTED else 0
        out.update(status=e.status, error_offset=e.at, codec=codec)
        return out
    t = r.track
    n, limit = len(data), t["limit"]
    frame = frames = place = first_sample = 0
    for k, run in enumerate(r.runs):
        if run["place"] is not None:
            place = run["place"]
        if run["time"] is not None:
            frame = run["time"]
        written = k < run_capacity
        if "entries" not in run:                       # (a run of a million samples of one size is not walked sample by sample)
            size, duration = run["same"]
            run_bytes, run_frames = size * run["count"], duration * run["count"]
        else:
            run_bytes, run_frames = sum(e[0] for e in run["entries"]), sum(e[1] for e in run["entries"])
        if written:
            out["run_rows"].append((place, frame, first_sample, run["count"], run_bytes))
            at, begins = place, frame
            for j in range(min(run["count"], max(0, packet_capacity - first_sample))):
                size, duration = run["entries"][j] if "entries" in run else run["same"]
                out["rows"].append((at, size) if 0 <= at and at + size <= n and size <= limit else None)
                out["samples_rows"].append((begins & M64, duration, k))
                at += size
                begins += duration
            first_sample += run["count"]
        place += run_bytes
        frame = (frame + run_frames) & M64
        frames += run_frames
    rows = out["rows"]
    bad = [s for s, row in enumerate(rows) if row is None]
    available = bad[0] if bad else len(rows)
    gathered = b""
    if gather:
        gathered = b"".join(data[at:at + size] for at, size in rows[gather_first_row:available])
        if len(gathered) > dst_capacity:
            gathered = b""
    duration = t["mdhd"][1] or (r.mehd or 0)
    alac = t["codec"] == code(b"alac")
    out.update(status=OK, codec=t["codec"], track_id=t["track_id"], timescale=t["mdhd"][0], duration=duration, frames=frames & M64, samples=r.samples,
               runs=len(r.runs), samples_available=available, samples_refused=len(bad), first_bad_sample=bad[0] if bad else NO_SAMPLE,
               entry_channels=t["entry"][0], entry_bits=t["entry"][1], entry_rate=t["entry"][2], bytes_gathered=len(gathered),
               moov_offset=r.moov, first_moof_offset=r.first_moof or 0, gathered=gathered)
    if alac:
        out["config"] = t["config"]
    else:
        out["flac"] = t["flac"]
    return out
