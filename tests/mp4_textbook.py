"""An independent model of the MPEG-4 container layer (ohgpu_mp4_*, include/ohgpu.h's MPEG-4 section) with the simplest loops there
are: the boxes by recursion, the samples chunk by chunk and sample by sample with a running file offset, the frames run by run with a
running count.  No prefix sums, no searches: it shares no algorithm with csrc/mp4_box_core.h's fused route, and none of its text.

demux(data, packet_capacity) -> dict: the fields of ohgpu_mp4_stream_result by name (config as a dict), and
    rows     [(file offset, bytes) or None for a refused sample], the first min(N, packet_capacity) samples
    samples  [(first_frame, frames, chunk)] of the same

Where this reading differs from the reference's (OpenHome/Media/Codec/Mpeg4.cpp; include/ohgpu.h carries the same list):
  - the reference streams, and fetches a moov behind mdat out of band; here the bytes are there and the walk goes on past mdat;
  - the reference refuses a file at its second stsz; here the first alac trak is taken and the rest skipped;
  - the reference's box header has no 64-bit size; here it has;
  - the reference wants chunk offsets that do not go backwards, because it streams; rows are independent here;
  - every sum is unbounded here (64-bit in the product), where the reference's are 32-bit with wrap checks;
  - a seek lands on the packet that holds the frame, not on that packet's chunk, and neither of the reference's two mixed-up
    comparisons (audio samples against codec samples; an offset within one stts entry taken for the track's) is reproduced;
  - an stts run of no samples among those that cover the track is INVALID."""
OK, NOT_MP4, TRUNCATED, INVALID, NOT_ALAC, UNSUPPORTED = range(6)
MAX_SAMPLES, MAX_BOXES, NO_SAMPLE = 1 << 24, 4096, 0xffffffff
CONFIG_FIELDS = ("frame_length", "compatible_version", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "max_frame_bytes", "avg_bit_rate", "sample_rate")
RESULT_FIELDS = ("status", "codec", "timescale", "entry_rate", "duration", "frames", "samples", "chunks", "samples_available", "samples_refused",
                 "first_bad_sample", "entry_channels", "entry_bits", "moov_offset", "mdat_offset", "mdat_bytes", "error_offset")


class Refuse(Exception):
    def __init__(self, status, at):
        self.status, self.at = status, at


def u(data, at, width):
    return int.from_bytes(data[at:at + width], "big")


def code(kind):
    return int.from_bytes(kind, "big")


class Reader:
    def __init__(self, data, capacity):
        self.data, self.capacity = data, capacity
        self.headers = 0
        self.taken = None
        self.first_codec = None
        self.moov = self.mdat = None

    def header(self, at, end, top=False):
        """the box at `at` of a parent that ends at `end` -> (kind, payload start, box end), or None where the parent has fewer than 8
        bytes left (at top level also: where a 64-bit size is cut off)"""
        data = self.data
        if end - at < 8:
            return None
        size, kind, head = u(data, at, 4), data[at + 4:at + 8], 8
        if size == 1 and end - at < 16 and top:
            return None
        self.headers += 1
        if self.headers > MAX_BOXES:
            raise Refuse(INVALID, at)
        if size == 1:
            if end - at < 16:
                raise Refuse(INVALID, at)
            size, head = u(data, at + 8, 8), 16
        elif size == 0:
            if not top:
                raise Refuse(INVALID, at)
            size = end - at
        if size < head:
            raise Refuse(INVALID, at)
        return kind, at + head, at + size

    def children(self, at, end):
        """every child box of [at, end) in order: (kind, box start, payload start, box end)"""
        while True:
            h = self.header(at, end)
            if h is None:
                return
            kind, pay, box_end = h
            if box_end > end:
                raise Refuse(INVALID, at)
            yield kind, at, pay, box_end
            at = box_end

    def file(self):
        data, n = self.data, len(self.data)
        if n < 8:
            raise Refuse(TRUNCATED, 0)
        if data[4:8] != b"ftyp":
            raise Refuse(NOT_MP4, 0)
        at = 0
        while True:
            h = self.header(at, n, top=True)
            if h is None:
                break
            kind, pay, end = h
            if kind == b"moof":
                raise Refuse(UNSUPPORTED, at)
            if kind == b"mdat" and self.mdat is None:
                self.mdat = (at, end - pay)
            if kind == b"moov" and self.moov is None:
                if end > n:
                    raise Refuse(TRUNCATED, at)
                self.moov = at
                self.movie(at, pay, end)
            if end > n:
                break
            at = end
        if self.moov is None:
            raise Refuse(TRUNCATED, at)

    def movie(self, box, at, end):
        for kind, child, pay, child_end in self.children(at, end):
            if kind == b"mvex":
                raise Refuse(UNSUPPORTED, child)
            if kind == b"trak" and self.taken is None:
                track = {}
                self.track(track, pay, child_end)
                if self.first_codec is None:
                    self.first_codec = track.get("codec", 0)
                if track.get("codec") == code(b"alac"):
                    self.finish(track, child)
                    self.taken = track
        if self.taken is None:
            raise Refuse(NOT_ALAC, box)

    def track(self, track, at, end):
        for kind, _, pay, child_end in self.children(at, end):
            if kind != b"mdia":
                continue
            for kind2, box2, pay2, end2 in self.children(pay, child_end):
                if kind2 == b"mdhd" and "mdhd" not in track:
                    track["mdhd"] = self.media_header(box2, pay2, end2)
                if kind2 != b"minf":
                    continue
                for kind3, _, pay3, end3 in self.children(pay2, end2):
                    if kind3 != b"stbl":
                        continue
                    for kind4, box4, pay4, end4 in self.children(pay3, end3):
                        self.table(track, kind4, box4, pay4, end4)

    def media_header(self, box, pay, end):
        data = self.data
        if end - pay < 4 or data[pay] > 1 or end - pay < (20, 32)[data[pay]]:
            raise Refuse(INVALID, box)
        timescale, duration = (u(data, pay + 12, 4), u(data, pay + 16, 4)) if data[pay] == 0 else (u(data, pay + 20, 4), u(data, pay + 24, 8))
        if timescale == 0:
            raise Refuse(INVALID, box)
        return timescale, duration

    def counted(self, box, pay, end, fixed, entry):
        """a version-0 table whose count (the last word of its `fixed` leading bytes) fits the box -> the count"""
        data = self.data
        if end - pay < fixed or data[pay] != 0:
            raise Refuse(INVALID, box)
        count = u(data, pay + fixed - 4, 4)
        if count * entry > end - pay - fixed:
            raise Refuse(INVALID, box)
        return count

    def table(self, track, kind, box, pay, end):
        data = self.data
        if kind == b"stz2":
            raise Refuse(UNSUPPORTED, box)
        if kind == b"stsd" and "stsd" not in track:
            track["stsd"] = box
            self.description(track, box, pay, end)
        elif kind == b"stts" and "stts" not in track:
            track["stts"] = box
            count = self.counted(box, pay, end, 8, 8)
            track["stts_runs"] = [(u(data, pay + 8 + 8 * m, 4), u(data, pay + 12 + 8 * m, 4)) for m in range(count)]
        elif kind == b"stsc" and "stsc" not in track:
            track["stsc"] = box
            count = self.counted(box, pay, end, 8, 12)
            track["stsc_runs"] = [(u(data, pay + 8 + 12 * k, 4), u(data, pay + 12 + 12 * k, 4)) for k in range(count)]
        elif kind in (b"stco", b"co64") and "co" not in track:
            track["co"] = box
            width = 4 if kind == b"stco" else 8
            count = self.counted(box, pay, end, 8, width)
            track["chunk_at"] = lambda c, base=pay + 8, width=width: u(data, base + width * c, width)
            track["chunks"] = count
        elif kind == b"stsz" and "stsz" not in track:
            track["stsz"] = box
            if end - pay < 12 or data[pay] != 0:
                raise Refuse(INVALID, box)
            uniform, count = u(data, pay + 4, 4), u(data, pay + 8, 4)
            if uniform == 0 and count * 4 > end - pay - 12:
                raise Refuse(INVALID, box)
            if count > MAX_SAMPLES:
                raise Refuse(UNSUPPORTED, box)
            track["samples"] = count
            track["size_of"] = (lambda s: uniform) if uniform else (lambda s, base=pay + 12: u(data, base + 4 * s, 4))

    def description(self, track, box, pay, end):
        data = self.data
        if self.counted(box, pay, end, 8, 1) == 0:
            return
        entry = pay + 8
        h = self.header(entry, end)
        if h is None or h[2] > end:
            raise Refuse(INVALID, entry)
        kind, body, entry_end = h
        track["codec"] = code(kind)
        if kind == b"enca":
            raise Refuse(UNSUPPORTED, entry)
        if kind != b"alac":
            return
        if entry_end - body < 28:
            raise Refuse(INVALID, entry)
        track["entry"] = (u(data, body + 16, 2), u(data, body + 18, 2), u(data, body + 24, 2))
        for kind, child, inner, child_end in self.children(body + 28, entry_end):
            if kind != b"alac":
                continue
            if child_end - inner < 28 or data[inner + 8] != 0:
                raise Refuse(UNSUPPORTED, child)
            widths = (4, 1, 1, 1, 1, 1, 1, 2, 4, 4, 4)
            cfg, at = {}, inner + 4
            for name, width in zip(CONFIG_FIELDS, widths):
                cfg[name] = u(data, at, width)
                at += width
            if not (1 <= cfg["channels"] <= 8 and 1 <= cfg["frame_length"] <= 16384 and cfg["bit_depth"] in (16, 20, 24, 32)):
                raise Refuse(UNSUPPORTED, child)
            track["config"] = cfg
            return
        raise Refuse(UNSUPPORTED, entry)

    def finish(self, track, box):
        """the taken trak's tables against each other"""
        for need in ("mdhd", "stsd", "stts", "stsc", "stsz", "co"):
            if need not in track:
                raise Refuse(INVALID, box)
        runs, chunks, samples = track["stsc_runs"], track["chunks"], track["samples"]
        covered = 0
        for k, (first, per_chunk) in enumerate(runs):
            if (first != 1 if k == 0 else first <= runs[k - 1][0]) or first > chunks or per_chunk < 1:
                raise Refuse(INVALID, track["stsc"])
            behind = runs[k + 1][0] if k + 1 < len(runs) else chunks + 1
            if behind > first:                        # (the next entry is judged in its own turn)
                covered += (behind - first) * per_chunk
        if covered < samples:
            raise Refuse(INVALID, track["stsc"])
        left, frames = samples, 0
        for count, delta in track["stts_runs"]:
            if left == 0:
                break
            if count == 0:
                raise Refuse(INVALID, track["stts"])
            frames += min(count, left) * delta
            left -= min(count, left)
        if left:
            raise Refuse(INVALID, track["stts"])
        track["frames"] = frames

    def expand(self, track):
        n, rows_wanted = len(self.data), min(track["samples"], self.capacity)
        rows, samples = [], []
        runs, chunks = track["stsc_runs"], track["chunks"]
        limit = track["config"]["frame_length"] * track["config"]["channels"] * 5 + 64
        s = 0
        for k, (first, per_chunk) in enumerate(runs):
            behind = runs[k + 1][0] if k + 1 < len(runs) else chunks + 1
            for chunk in range(first - 1, behind - 1):
                if s == rows_wanted:
                    break
                at = track["chunk_at"](chunk)
                for _ in range(per_chunk):
                    if s == rows_wanted:
                        break
                    size = track["size_of"](s)
                    rows.append((at, size) if at + size <= n and size <= limit else None)
                    samples.append([0, 0, chunk])
                    at += size
                    s += 1
        s = frame = 0
        for count, delta in track["stts_runs"]:
            for _ in range(count):
                if s == rows_wanted:
                    break
                samples[s][0], samples[s][1] = frame, delta
                frame += delta
                s += 1
        return rows, [tuple(x) for x in samples]


def demux(data, packet_capacity):
    data = bytes(data)
    r = Reader(data, packet_capacity)
    out = dict.fromkeys(RESULT_FIELDS, 0)
    out.update(config=dict.fromkeys(CONFIG_FIELDS, 0), first_bad_sample=NO_SAMPLE, rows=[], samples_rows=[])
    try:
        r.file()
    except Refuse as e:
        out.update(status=e.status, error_offset=e.at, codec=(r.first_codec or 0) if e.status == NOT_ALAC else 0)
        return out
    t = r.taken
    rows, sample_rows = r.expand(t)
    bad = [s for s, row in enumerate(rows) if row is None]
    out.update(status=OK, codec=t["codec"], config=t["config"], timescale=t["mdhd"][0], duration=t["mdhd"][1], frames=t["frames"],
               entry_channels=t["entry"][0], entry_bits=t["entry"][1], entry_rate=t["entry"][2], samples=t["samples"], chunks=t["chunks"],
               samples_refused=len(bad), first_bad_sample=bad[0] if bad else NO_SAMPLE, samples_available=bad[0] if bad else len(rows),
               moov_offset=r.moov, mdat_offset=r.mdat[0] if r.mdat else 0, mdat_bytes=r.mdat[1] if r.mdat else 0, rows=rows, samples_rows=sample_rows)
    return out


def seek(sample_rows, frame):
    """the row that holds the frame -> (index, its first frame), or None behind the last row; the plainest search"""
    for index, (first, frames, _) in enumerate(sample_rows):
        if first <= frame < first + frames:
            return index, first
    return None
