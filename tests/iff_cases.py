"""The tests' own writer of WAV, AIFF and AIFC files, and what the PCM file tests share: named good and malformed files, prefixes
round every chunk boundary, seeded damage to the headers, and the job (arenas, descriptors, the model's results and the destination
every route must leave) with its comparison.  The writer keeps a record of what it wrote -- the format, where the audio lies, the
samples most significant byte first -- which tests/test_iff_textbook.py holds the model (tests/iff_textbook.py) to."""
import random
import struct

import numpy as np

import iff_textbook as IX

FILL, GUARD = 0xA5, 48


class Written:
    """data: the file.  kind, channels, rate, depth (as reported), sample_bytes, little, frames; data_offset: the first audio byte;
    top_first: the samples as rows of bytes, most significant first; marks: (chunk position, payload position, stated size) per chunk."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def pcm(self, out_bytes=None, first=0, frames=None):
        rows = self.top_first[first * self.channels:(self.frames if frames is None else first + frames) * self.channels]
        return rows[:, :out_bytes or self.sample_bytes].tobytes()


def samples(frames, channels, sample_bytes, seed=1):
    """Rows of sample bytes, most significant first."""
    return np.random.default_rng(seed).integers(0, 256, size=(frames * channels, sample_bytes), dtype=np.uint8)


def assemble(form, kind_id, chunks, little_sizes, form_size=None):
    """chunks: (id, payload, stated size or None).  Returns the bytes and the marks."""
    body, marks = bytearray(), []
    for name, payload, stated in chunks:
        size = len(payload) if stated is None else stated
        marks.append((12 + len(body), 20 + len(body), size))
        body += name + size.to_bytes(4, "little" if little_sizes else "big") + payload
        if len(payload) % 2:
            body += b"\0"
    total = 4 + len(body) if form_size is None else form_size
    return bytes(form + total.to_bytes(4, "little" if little_sizes else "big") + kind_id + body), marks


def junk(name, length, seed=7):
    return (name, bytes(random.Random(seed * 1000 + length).randrange(256) for _ in range(length)), None)


def wav(top_first, channels, *, rate=44100, fmt_size=16, tag=None, sub_format=1, data_first=False, before_fmt=(), between=(), behind=(), continuous=False,
        data_size=None, byte_rate=None, depth=None):
    sample_bytes = top_first.shape[1]
    depth = 8 * sample_bytes if depth is None else depth
    frames = top_first.shape[0] // channels
    tag = (0xfffe if fmt_size == 40 else 1) if tag is None else tag
    byte_rate = rate * channels * sample_bytes if byte_rate is None else byte_rate
    fmt = struct.pack("<HHIIHH", tag, channels, rate, byte_rate, channels * sample_bytes, depth)
    if fmt_size >= 18:
        fmt += struct.pack("<H", fmt_size - 18)
    if fmt_size == 40:
        fmt += struct.pack("<HIH", depth, 3, sub_format) + bytes.fromhex("0000" "0000" "1000" "8000" "00aa00389b71")
    audio = top_first[:, ::-1].tobytes()
    f, d = (b"fmt ", fmt, None), (b"data", audio, data_size)
    chunks = list(before_fmt) + ([d] + list(between) + [f] if data_first else [f] + list(between) + [d]) + list(behind)
    data, marks = assemble(b"RIFF", b"WAVE", chunks, True, 0 if continuous else None)
    at = marks[chunks.index(d)][1]
    return Written(data=data, kind=IX.WAV, channels=channels, rate=rate, depth=depth, sample_bytes=sample_bytes, little=True, frames=frames, data_offset=at,
                   top_first=top_first, marks=marks, bit_rate=(byte_rate * 8) % 2 ** 32, audio_bytes=len(audio),
                   frames_stated=0 if continuous else (len(audio) if data_size is None else data_size) // (channels * sample_bytes))


def ext80(rate):
    """An integer rate as the 80-bit extended number of a COMM chunk."""
    top = rate.bit_length() - 1
    return struct.pack(">HQ", 0x3fff + top, rate << (63 - top))


def aiff(top_first, channels, *, rate=44100, rate_field=None, depth=None, compression=None, ssnd_offset=0, ssnd_first=False, before=(), between=(), behind=(),
         frames_field=None, name=b"not compressed"):
    sample_bytes = top_first.shape[1]
    depth = 8 * sample_bytes if depth is None else depth
    frames = top_first.shape[0] // channels
    little = compression in (b"sowt", b"SOWT")
    comm = struct.pack(">HIH", channels, frames if frames_field is None else frames_field, depth) + (ext80(rate) if rate_field is None else rate_field)
    if compression is not None:
        pstring = bytes([len(name)]) + name
        comm += compression + pstring + (b"\0" if len(pstring) % 2 else b"")
    audio = (top_first[:, ::-1] if little else top_first).tobytes()
    ssnd = struct.pack(">II", ssnd_offset, 0) + bytes((37 * k + 11) % 256 for k in range(ssnd_offset)) + audio
    c, s = (b"COMM", comm, None), (b"SSND", ssnd, None)
    chunks = list(before) + ([s] + list(between) + [c] if ssnd_first else [c] + list(between) + [s]) + list(behind)
    data, marks = assemble(b"FORM", b"AIFF" if compression is None else b"AIFC", chunks, False)
    at = marks[chunks.index(s)][1] + 8 + ssnd_offset
    return Written(data=data, kind=IX.AIFF if compression is None else IX.AIFC, channels=channels, rate={22255: 22050, 11127: 11025}.get(rate, rate),
                   depth=24 if depth == 20 else depth, sample_bytes=sample_bytes, little=little, frames=frames, data_offset=at, top_first=top_first, marks=marks,
                   bit_rate=({22255: 22050, 11127: 11025}.get(rate, rate) * channels * sample_bytes * 8) % 2 ** 32, audio_bytes=len(audio),
                   frames_stated=frames if frames_field is None else frames_field)


def named_good():
    s = samples
    return {
        "wav16": wav(s(40, 2, 2, 1), 2),
        "wav8_mono": wav(s(33, 1, 1, 2), 1, rate=8000),
        "wav24_odd_data": wav(s(7, 1, 3, 3), 1, rate=48000),                       # 21 audio bytes and a pad byte
        "wav32": wav(s(19, 2, 4, 4), 2, rate=96000),
        "wav_fmt18": wav(s(12, 2, 2, 5), 2, fmt_size=18),
        "wav_extensible_6ch": wav(s(9, 6, 3, 6), 6, fmt_size=40, rate=48000),
        "wav_extensible_tag_short": wav(s(5, 2, 2, 7), 2, tag=0xfffe),             # 16 bytes of an extensible format: no sub-format to look at
        "wav_data_first": wav(s(21, 2, 2, 8), 2, data_first=True, between=[junk(b"LIST", 9)]),
        "wav_junk_everywhere": wav(s(15, 3, 2, 9), 3, before_fmt=[junk(b"JUNK", 3), junk(b"bext", 10)], between=[junk(b"LIST", 1)], behind=[junk(b"id3 ", 5)]),
        "wav_continuous": wav(s(25, 2, 2, 10), 2, continuous=True, data_size=0),
        "wav_data_longer_than_file": wav(s(10, 2, 2, 11), 2, data_size=1000),
        "wav_second_fmt_ignored": wav(s(6, 2, 2, 12), 2, between=[(b"fmt ", b"\0" * 16, None)]),
        "wav_10ch": wav(s(4, 10, 4, 13), 10),
        "aiff16": aiff(s(30, 2, 2, 21), 2),
        "aiff8": aiff(s(17, 1, 1, 22), 1, rate=22255),
        "aiff20": aiff(s(11, 2, 3, 23), 2, depth=20, rate=48000),
        "aiff24_offset": aiff(s(13, 2, 3, 24), 2, ssnd_offset=5),
        "aiff32": aiff(s(9, 2, 4, 25), 2, rate=192000),
        "aiff_ssnd_first": aiff(s(14, 1, 2, 26), 1, ssnd_first=True, between=[junk(b"ANNO", 7)], rate=11127),
        "aiff_junk": aiff(s(8, 2, 2, 27), 2, before=[junk(b"NAME", 5)], between=[junk(b"AUTH", 2)], behind=[junk(b"ID3 ", 3)], rate=1),
        "aifc_none": aiff(s(16, 2, 3, 28), 2, compression=b"NONE"),
        "aifc_sowt": aiff(s(18, 2, 2, 29), 2, compression=b"sowt", name=b""),
        "aifc_SOWT24": aiff(s(10, 3, 3, 30), 3, compression=b"SOWT", ssnd_offset=3, rate=88200),
        "aifc_sowt32": aiff(s(6, 2, 4, 31), 2, compression=b"sowt", rate=0xfffffffe),
    }


def patched(w, at, raw):
    data = bytearray(w.data)
    data[at:at + len(raw)] = raw
    return bytes(data)


def many_chunks(count):
    return assemble(b"RIFF", b"WAVE", [(b"JUNK", b"", None)] * count + [(b"fmt ", struct.pack("<HHIIHH", 1, 1, 8000, 16000, 2, 16), None), (b"data", b"\1\2", None)], True)[0]


def named_malformed():
    """name -> (bytes, status, the chunk position error_offset must name)"""
    s = samples
    w, a, c = wav(s(8, 2, 2, 41), 2), aiff(s(8, 2, 2, 42), 2), aiff(s(8, 2, 2, 43), 2, compression=b"NONE")
    fmt, comm, ssnd = w.marks[0], a.marks[0], a.marks[1]
    X = IX
    return {
        "empty": (b"", X.NOT_IFF, 0),
        "eleven_bytes": (w.data[:11], X.NOT_IFF, 0),
        "riff_not_wave": (patched(w, 8, b"AVI "), X.NOT_IFF, 0),
        "form_not_aiff": (patched(a, 8, b"8SVX"), X.NOT_IFF, 0),
        "rifx": (patched(w, 0, b"RIFX"), X.NOT_IFF, 0),
        "header_only": (w.data[:12], X.TRUNCATED, 12),
        "fmt_cut": (w.data[:30], X.TRUNCATED, 12),
        "no_data_chunk": (w.data[:fmt[1] + 16 + 5], X.TRUNCATED, fmt[1] + 16),
        "fmt_size_20": (patched(w, fmt[0] + 4, struct.pack("<I", 20)), X.INVALID, 12),
        "adpcm": (patched(w, fmt[1], struct.pack("<H", 2)), X.UNSUPPORTED, 12),
        "float": (patched(w, fmt[1], struct.pack("<H", 3)), X.UNSUPPORTED, 12),
        "extensible_float": (wav(s(4, 2, 4, 44), 2, fmt_size=40, sub_format=3).data, X.UNSUPPORTED, 12),
        "no_channels": (patched(w, fmt[1] + 2, struct.pack("<H", 0)), X.INVALID, 12),
        "eleven_channels": (patched(w, fmt[1] + 2, struct.pack("<H", 11)), X.UNSUPPORTED, 12),
        "rate_0": (patched(w, fmt[1] + 4, struct.pack("<I", 0)), X.INVALID, 12),
        "byte_rate_0": (patched(w, fmt[1] + 8, struct.pack("<I", 0)), X.INVALID, 12),
        "depth_0": (patched(w, fmt[1] + 14, struct.pack("<H", 0)), X.INVALID, 12),
        "depth_12": (patched(w, fmt[1] + 14, struct.pack("<H", 12)), X.INVALID, 12),
        "depth_40": (patched(w, fmt[1] + 14, struct.pack("<H", 40)), X.UNSUPPORTED, 12),
        "continuous_data_first": (wav(s(4, 2, 2, 45), 2, continuous=True, data_first=True).data, X.INVALID, 12),
        "too_many_chunks": (many_chunks(IX.MAX_CHUNKS), X.INVALID, 12 + 8 * IX.MAX_CHUNKS),
        "comm_17": (patched(a, comm[0] + 4, struct.pack(">I", 17)), X.INVALID, 12),
        "aifc_comm_18": (patched(c, comm[0] + 4, struct.pack(">I", 18)), X.INVALID, 12),
        "comm_cut": (a.data[:25], X.TRUNCATED, 12),
        "aiff_no_channels": (patched(a, comm[1], struct.pack(">H", 0)), X.INVALID, 12),
        "aiff_depth_12": (patched(a, comm[1] + 6, struct.pack(">H", 12)), X.UNSUPPORTED, 12),
        "rate_negative": (patched(a, comm[1] + 8, struct.pack(">H", 0xc00e)), X.INVALID, 12),
        "rate_below_one": (patched(a, comm[1] + 8, struct.pack(">H", 0x3ffe)), X.INVALID, 12),
        "rate_2_to_32": (patched(a, comm[1] + 8, struct.pack(">H", 0x401f)), X.INVALID, 12),
        "rate_denormal_0": (patched(a, comm[1] + 8, struct.pack(">HQ", 0x3fff, 0)), X.INVALID, 12),
        "aifc_ulaw": (patched(c, comm[1] + 18, b"ulaw"), X.UNSUPPORTED, 12),
        "aifc_fl32": (patched(c, comm[1] + 18, b"fl32"), X.UNSUPPORTED, 12),
        "ssnd_of_4": (patched(a, ssnd[0] + 4, struct.pack(">I", 4)), X.INVALID, ssnd[0]),
        "ssnd_header_cut": (a.data[:ssnd[1] + 7], X.TRUNCATED, ssnd[0]),
        "ssnd_offset_beyond": (patched(a, ssnd[1], struct.pack(">I", ssnd[2] - 7)), X.INVALID, ssnd[0]),
        "more_frames_than_ssnd_holds": (patched(a, comm[1] + 2, struct.pack(">I", 9)), X.INVALID, ssnd[0]),
        "offset_eats_the_audio": (patched(a, ssnd[1], struct.pack(">I", 1)), X.INVALID, ssnd[0]),
    }


def cuts(w):
    """Prefixes of a file round every chunk boundary and inside the audio."""
    ends = set()
    for chunk, pay, size in w.marks:
        for at in (chunk, chunk + 4, pay, pay + 1, pay + size, pay + size + size % 2):
            ends.update((at - 1, at, at + 1))
    frame = w.channels * w.sample_bytes
    for k in (0, 1, 2, w.frames // 2, w.frames - 1, w.frames):
        ends.update((w.data_offset + k * frame - 1, w.data_offset + k * frame, w.data_offset + k * frame + 1))
    return [w.data[:n] for n in sorted(ends) if 0 <= n <= len(w.data)]


def damaged(count, seed=20262):
    """Files with one to three bytes of their headers (everything but the audio) replaced, seeded."""
    rnd = random.Random(seed)
    good = [w for name, w in named_good().items() if name != "wav_continuous"]
    out = []
    for _ in range(count):
        w = rnd.choice(good)
        header = [k for k in range(len(w.data)) if not w.data_offset <= k < w.data_offset + w.audio_bytes]
        data = bytearray(w.data)
        for _ in range(rnd.choice((1, 1, 2, 3))):
            data[rnd.choice(header)] = rnd.choice((0, 0, 1, 2, 3, 8, 16, 18, 20, 24, 32, 40, 0x40, 0x7f, 0x80, 0xfe, 0xff, rnd.randrange(256), rnd.randrange(256)))
        out.append(bytes(data))
    return out


def check_against_record(model, w, out_bytes=None):
    assert model["status"] == IX.OK, model
    got = {k: model[k] for k in ("kind", "channels", "sample_rate", "src_bit_depth", "src_endian", "bit_rate", "data_offset")}
    assert got == dict(kind=w.kind, channels=w.channels, sample_rate=w.rate, src_bit_depth=w.depth, src_endian=IX.LITTLE if w.little else IX.BIG, bit_rate=w.bit_rate,
                       data_offset=w.data_offset), (got, w.__dict__)
    assert model["frames_available"] == w.frames == model["frames_written"] and model["frames_total"] == w.frames_stated
    assert model["pcm"] == w.pcm(out_bytes or min(w.sample_bytes, model["out_bit_depth"] // 8))


def stream(data, *, flags=0, frame_first=0, frames=None, room=None, max_bit_depth=24):
    """One stream of a job: a Written or bytes.  frames: dst_frame_capacity (default: the file's frames, 16 for bare bytes);
    room: dst_bytes_capacity (default: those frames at the file's output width, 40 bytes a frame for bare bytes)."""
    w = data if isinstance(data, Written) else None
    raw = w.data if w else bytes(data)
    if frames is None:
        frames = w.frames if w else 16
    if room is None:
        room = frames * w.channels * min(w.sample_bytes, max_bit_depth // 8) if w else frames * 40
    return dict(data=raw, flags=flags, frame_first=frame_first, frames=frames, room=room, max_bit_depth=max_bit_depth)


class Job:
    """Streams laid into a source arena (stream i at an address that is `align(i)` mod 16) and a destination arena (its run at
    `dst_align(i)` mod 16, GUARD bytes of fill in front of, between and behind the runs), the descriptors, the model's results and
    the destination arena as every route must leave it when it starts as FILL."""

    def __init__(self, streams, align=lambda i: (5 * i + 1) % 16, dst_align=lambda i: (7 * i + 3) % 16):
        from ohpipeline_amd import capi
        self.streams = streams
        self.descs = np.zeros(len(streams), dtype=capi.IFF_STREAM_DESC)
        src, at = bytearray(), GUARD
        self.models = []
        for i, s in enumerate(streams):
            while len(src) % 16 != align(i):
                src.append(FILL)
            while at % 16 != dst_align(i):
                at += 1
            d = self.descs[i]
            d["src_offset"], d["src_bytes"], d["flags"] = len(src), len(s["data"]), s["flags"]
            d["dst_offset"], d["dst_bytes_capacity"], d["frame_first"] = at, s["room"], s["frame_first"]
            d["dst_frame_capacity"], d["max_bit_depth"] = s["frames"], s["max_bit_depth"]
            src += s["data"]
            at += s["room"] + GUARD
            self.models.append(IX.read(s["data"], flags=s["flags"], frame_first=s["frame_first"], dst_frame_capacity=s["frames"], dst_bytes_capacity=s["room"],
                                       max_bit_depth=s["max_bit_depth"]))
        while len(src) % 4:
            src.append(FILL)
        self.src = np.frombuffer(bytes(src) or b"\0\0\0\0", dtype=np.uint8).copy()
        self.dst_bytes = at
        self.want_dst = np.full(at, FILL, dtype=np.uint8)
        for d, m in zip(self.descs, self.models):
            assert len(m["pcm"]) <= int(d["dst_bytes_capacity"])
            o = int(d["dst_offset"])
            self.want_dst[o:o + len(m["pcm"])] = np.frombuffer(m["pcm"], dtype=np.uint8)

    def driver_blob(self):
        return struct.pack("<QQQ", len(self.streams), self.src.size, self.dst_bytes) + self.descs.tobytes() + self.src.tobytes()


FIELDS = ("status", "kind", "channels", "sample_rate", "src_bit_depth", "out_bit_depth", "src_endian", "bit_rate", "frames_total", "frames_available",
          "frames_written", "data_offset", "data_bytes", "error_offset")


def assert_same(results, dst, job, what=""):
    assert len(results) == len(job.models)
    for i, (r, m) in enumerate(zip(results, job.models)):
        got = {k: int(r[k]) for k in FIELDS}
        assert got == {k: m[k] for k in FIELDS}, (what, i, got, {k: m[k] for k in FIELDS})
    dst = np.asarray(dst)
    if not np.array_equal(dst, job.want_dst):
        at = int(np.flatnonzero(dst != job.want_dst)[0])
        owner = [i for i, d in enumerate(job.descs) if int(d["dst_offset"]) - GUARD <= at < int(d["dst_offset"]) + int(d["dst_bytes_capacity"]) + GUARD]
        raise AssertionError(f"{what}: destination byte {at} is {dst[at]:#x}, the model has {job.want_dst[at]:#x} (streams {owner}, "
                             f"run at {[int(job.descs[i]['dst_offset']) for i in owner]})")


GROUP_PIECES = 1024          # kIffGroupPieces (csrc/ohgpu_internal.h): the pieces one workgroup of the conversion takes


def combos():
    """(name, make(frames, channels, seed, **kw) -> Written, stream keywords, a piece's output bytes) for every source width x output
    width x byte order the conversion tells apart."""
    def w(sample_bytes):
        return lambda frames, channels, seed, **kw: wav(samples(frames, channels, sample_bytes, seed), channels, **kw)

    def a(sample_bytes, compression=None):
        return lambda frames, channels, seed, **kw: aiff(samples(frames, channels, sample_bytes, seed), channels, compression=compression, **kw)
    return [("wav8", w(1), {}, 16), ("wav8_unsigned", w(1), dict(flags=IX.FLAG_WAV8_UNSIGNED), 16), ("wav16", w(2), {}, 16), ("wav24", w(3), {}, 48),
            ("wav32", w(4), dict(max_bit_depth=32), 16), ("wav32_to_24", w(4), {}, 48),
            ("aiff8", a(1), {}, 16), ("aiff16", a(2), {}, 16), ("aiff24", a(3), {}, 16), ("aiff32", a(4), dict(max_bit_depth=32), 16), ("aiff32_to_24", a(4), {}, 48),
            ("sowt16", a(2, b"sowt"), {}, 16), ("sowt24", a(3, b"sowt"), {}, 48), ("sowt32", a(4, b"sowt"), dict(max_bit_depth=32), 16),
            ("sowt32_to_24", a(4, b"sowt"), {}, 48)]


def shape_sweep():
    """The streams of the shape sweep: the smallest shapes at which the conversion can go wrong."""
    streams, seed = [], 100
    for name, make, kw, unit in combos():
        for channels in (1, 2, 3, 6):
            for frames in (0, 1, 2, 3, 5, 15, 16, 17, 63, 64, 65):
                seed += 1
                streams.append(stream(make(frames, channels, seed), **kw))
        # one workgroup's pieces, a frame fewer and a frame more (the head takes up to 15 bytes: two frames more as well), and a third workgroup
        first = make(1, 1, 0)
        out_bytes = min(first.sample_bytes, kw.get("max_bit_depth", 24) // 8)
        whole = GROUP_PIECES * unit // out_bytes
        for frames in (whole - 1, whole, whole + 1, whole + 16, 2 * whole + 7):
            seed += 1
            streams.append(stream(make(frames, 1, seed), **kw))
        # a seek, a seek behind the end, a room shorter than the audio in frames and in bytes, a file cut in mid-frame
        seed += 1
        f = make(37, 2, seed)
        frame_out = 2 * out_bytes
        streams += [stream(f, frame_first=1, **kw), stream(f, frame_first=36, **kw), stream(f, frame_first=37, **kw), stream(f, frame_first=1 << 33, **kw),
                    stream(f, frames=20, **kw), stream(f, frames=37, room=20 * frame_out + frame_out - 1, **kw), stream(f, frames=0, room=0, **kw),
                    stream(f.data[:f.data_offset + 11 * 2 * f.sample_bytes + 1], frames=37, room=37 * frame_out, **kw)]
    streams.append(stream(wav(samples(90, 2, 2, 5), 2, continuous=True, data_size=0, before_fmt=[junk(b"JUNK", 5)])))
    streams.append(stream(wav(samples(90, 2, 3, 6), 2, continuous=True, data_size=0xffffffff), frame_first=3))
    # every kind between refused neighbours
    good, bad = named_good(), named_malformed()
    for k, (data, _, _) in enumerate(bad.values()):
        streams += [stream(list(good.values())[k % len(good)]), stream(data)]
    return streams


def alignment_sweep(frames=17):
    """Jobs of 256 streams each: the audio at every address mod 16 (a junk chunk of that length in front of it, and the file placed to
    suit) crossed with the run at every address mod 16."""
    jobs = []
    for name, make, kw, unit in combos():
        if name not in ("wav16", "wav24", "wav32_to_24", "aiff32_to_24", "sowt24", "wav32"):
            continue
        files = [make(frames, 2, 300 + k, **({"before" if name.startswith(("aiff", "sowt")) else "before_fmt": [junk(b"JUNK", k)]})) for k in range(16)]
        job = Job([stream(files[i % 16], **kw) for i in range(256)], align=lambda i, files=files: (i % 16 - files[i % 16].data_offset) % 16, dst_align=lambda i: i // 16)
        assert {((int(d["src_offset"]) + files[i % 16].data_offset) % 16, int(d["dst_offset"]) % 16) for i, d in enumerate(job.descs)} == \
            {(a, b) for a in range(16) for b in range(16)}
        assert all(m["status"] == IX.OK and m["frames_written"] == frames for m in job.models)
        jobs.append(job)
    return jobs
