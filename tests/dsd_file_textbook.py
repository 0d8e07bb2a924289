"""A textbook model of DSF and DFF files in front of the pipeline's DSD format (ohgpu_dsd_file_*), written from the
specification in include/ohgpu.h's DSD file section, one field at a time, sharing nothing with csrc/dsd_file_core.h.  For the audio
bytes it calls the packers of tests/dsd_textbook.py on the run it found, so the file layer and the packer layer cannot drift.  It also
carries the tests' own writer of DSF and DFF files from two channels' bit streams.

The kind.  Bytes 0..4 "DSD " is DSF; bytes 0..4 "FRM8" with bytes 12..16 "DSD " is DFF; anything else, or fewer than 16 bytes, is
NOT_DSD.  The first thing wrong gives the status and error_offset names the chunk that gave it; every other field of a refused stream
reads 0.  A header the walk needs that does not lie inside the bytes at hand is TRUNCATED.

DSF, little-endian, chunk sizes u64 that include the 12 bytes of id and size:
    `DSD `  28 bytes: size (28, else INVALID), the file's total size (0: INVALID), the metadata pointer (reported, not followed).
    `fmt `  at 28, else INVALID; size at least 52 and below 2^31, else INVALID.  Format version (reported), format id (0, else
            UNSUPPORTED), channel type (reported), channel count (2, else UNSUPPORTED), rate (0: INVALID), bits per sample (1, else
            UNSUPPORTED), sample count u64, block size per channel (4096, else UNSUPPORTED), 4 reserved bytes.
    `data`  at 28 + the fmt size, else INVALID; size at least 12, else INVALID.  Audio bytes = size - 12: odd: INVALID;
            2 * floor(sample_count / 8) above them: INVALID.
    chunks_total = floor(sample_count / 16).
DFF, big-endian, id + u64 size + payload + one pad byte behind an odd size:
    chunks from byte 16; more than MAX_CHUNKS headers (a PROP's local ones counted): INVALID; a size of 2^63 or more: INVALID.  The
    first `PROP` of type `SND ` and the first `DSD `, in either order; the walk stops when it has both.
    `FVER`  size 4, else INVALID; payload inside the bytes, else TRUNCATED; first byte 1, else UNSUPPORTED.
    `DST `  before `DSD `: UNSUPPORTED.
    `PROP`  size at least 4, else INVALID; payload inside the bytes, else TRUNCATED.  Local chunks: `FS  ` size 4 (else INVALID), rate
            0: INVALID; `CHNL` at least 2 bytes (else INVALID), u16 count 2, else UNSUPPORTED; `CMPR` at least 4 bytes (else INVALID),
            fourcc `DSD `, else UNSUPPORTED; a local chunk that runs past the PROP: INVALID; no `FS  ` or no `CHNL`: INVALID.
    `DSD `  audio = the stated size; odd: INVALID.  chunks_total = floor(size / 4), sample_count = 16 * chunks_total.
Audio past the bytes at hand is no error: chunks_available counts the chunks below chunks_total whose four source bytes are all there.

The conversion.  cpb = W * 4 / (4 + P); room = floor(capacity / (W * 4)) * cpb; n = min(chunks_available - chunk_first, room), 0 when
chunk_first lies behind the available chunks.  If the n chunks reach chunks_total the last partial block is filled with 0x69; if not,
n is rounded down to whole blocks.

Where this differs from the reference (include/ohgpu.h carries the same list):
  - the reference streams and wants DFF's chunks in its own order; here `PROP` and `DSD ` are read in either order and everything
    else is skipped by its size;
  - the reference does not skip the pad byte behind an odd DFF chunk; here it is honoured;
  - the reference does not look at `CMPR`, at a `DST ` chunk, at DSF's format id or at its bits per sample; here they are looked at
    and refused, instead of played as noise;
  - a channel count other than 2 is UNSUPPORTED in both kinds;
  - the reference does not hold DSF's sample count against the `data` size; here a count the chunk cannot hold is INVALID.
"""
import struct

import dsd_textbook as DT

OK, NOT_DSD, TRUNCATED, INVALID, UNSUPPORTED = range(5)
DSF, DFF = DT.DSF, DT.DFF
MAX_CHUNKS = 4096
PLANE = DT.DSF_BLOCK
FIELDS = ("status", "kind", "channels", "sample_rate", "format_version", "channel_type", "sample_count", "chunks_total", "chunks_available", "chunks_written",
          "bytes_written", "data_offset", "data_bytes", "metadata_offset", "error_offset")


class Refusal(Exception):
    def __init__(self, status, at):
        self.status, self.at = status, at


def _need(data, pos, count, chunk):
    if pos + count > len(data):
        raise Refusal(TRUNCATED, chunk)


def _walk_dsf(data):
    _need(data, 0, 28, 0)
    size, total, metadata = struct.unpack_from("<QQQ", data, 4)
    if size != 28 or total == 0:
        raise Refusal(INVALID, 0)
    _need(data, 28, 12, 28)
    if data[28:32] != b"fmt ":
        raise Refusal(INVALID, 28)
    fmt_size, = struct.unpack_from("<Q", data, 32)
    if fmt_size < 52 or fmt_size >= 2 ** 31:
        raise Refusal(INVALID, 28)
    _need(data, 28, 52, 28)
    version, format_id, channel_type, channels, rate, bits, samples, block = struct.unpack_from("<IIIIIIQI", data, 40)
    if format_id != 0:
        raise Refusal(UNSUPPORTED, 28)
    if channels != 2:
        raise Refusal(UNSUPPORTED, 28)
    if rate == 0:
        raise Refusal(INVALID, 28)
    if bits != 1:
        raise Refusal(UNSUPPORTED, 28)
    if block != PLANE:
        raise Refusal(UNSUPPORTED, 28)
    at = 28 + fmt_size
    _need(data, at, 12, at)
    if data[at:at + 4] != b"data":
        raise Refusal(INVALID, at)
    data_size, = struct.unpack_from("<Q", data, at + 4)
    if data_size < 12 or (data_size - 12) % 2:
        raise Refusal(INVALID, at)
    if 2 * (samples // 8) > data_size - 12:
        raise Refusal(INVALID, at)
    return dict(kind=DSF, sample_rate=rate, format_version=version, channel_type=channel_type, sample_count=samples, chunks_total=samples // 16, data_offset=at + 12,
                data_bytes=data_size - 12, metadata_offset=metadata)


def _walk_prop(data, chunk, pay, size, count):
    rate = channels = None
    pos, end = pay + 4, pay + size
    while pos < end:
        count[0] += 1
        if count[0] > MAX_CHUNKS:
            raise Refusal(INVALID, pos)
        if end - pos < 12:
            raise Refusal(INVALID, chunk)
        name, local = data[pos:pos + 4], struct.unpack_from(">Q", data, pos + 4)[0]
        at = pos + 12
        if local > end - at:
            raise Refusal(INVALID, chunk)
        if name == b"FS  ":
            if local != 4:
                raise Refusal(INVALID, chunk)
            rate, = struct.unpack_from(">I", data, at)
            if rate == 0:
                raise Refusal(INVALID, chunk)
        elif name == b"CHNL":
            if local < 2:
                raise Refusal(INVALID, chunk)
            channels, = struct.unpack_from(">H", data, at)
            if channels != 2:
                raise Refusal(UNSUPPORTED, chunk)
        elif name == b"CMPR":
            if local < 4:
                raise Refusal(INVALID, chunk)
            if data[at:at + 4] != b"DSD ":
                raise Refusal(UNSUPPORTED, chunk)
        pos = at + local + local % 2
    if rate is None or channels is None:
        raise Refusal(INVALID, chunk)
    return rate


def _walk_dff(data):
    found, rate, audio, count, pos = dict(format_version=0), None, None, [0], 16
    while rate is None or audio is None:
        count[0] += 1
        if count[0] > MAX_CHUNKS:
            raise Refusal(INVALID, pos)
        _need(data, pos, 12, pos)
        name, size = data[pos:pos + 4], struct.unpack_from(">Q", data, pos + 4)[0]
        pay = pos + 12
        if size >= 2 ** 63:
            raise Refusal(INVALID, pos)
        if name == b"FVER":
            if size != 4:
                raise Refusal(INVALID, pos)
            _need(data, pay, 4, pos)
            if data[pay] != 1:
                raise Refusal(UNSUPPORTED, pos)
            found["format_version"], = struct.unpack_from(">I", data, pay)
        elif name == b"DST " and audio is None:
            raise Refusal(UNSUPPORTED, pos)
        elif name == b"PROP" and rate is None:
            if size < 4:
                raise Refusal(INVALID, pos)
            _need(data, pay, size, pos)
            if data[pay:pay + 4] == b"SND ":
                rate = _walk_prop(data, pos, pay, size, count)
        elif name == b"DSD " and audio is None:
            if size % 2:
                raise Refusal(INVALID, pos)
            audio = (pay, size)
        pos = pay + size + size % 2
    found.update(kind=DFF, sample_rate=rate, channel_type=0, chunks_total=audio[1] // 4, sample_count=16 * (audio[1] // 4), data_offset=audio[0], data_bytes=audio[1],
                 metadata_offset=0)
    return found


def chunk_is_present(kind, data, data_offset, j):
    """Whether the four source bytes of chunk j all lie inside the bytes at hand."""
    if kind == DFF:
        return data_offset + 4 * j + 4 <= len(data)
    q, r = divmod(j, PLANE // 2)
    left = data_offset + 2 * PLANE * q + 2 * r
    return left + PLANE + 2 <= len(data)


def read(data, W, P, chunk_first=0, dst_bytes_capacity=None):
    """The result record of one stream (FIELDS) and "blocks": the bytes it writes at its dst_offset."""
    data = bytes(data)
    none = dict({k: 0 for k in FIELDS}, blocks=b"")
    try:
        if len(data) < 16:
            raise Refusal(NOT_DSD, 0)
        if data[0:4] == b"DSD ":
            found = _walk_dsf(data)
        elif data[0:4] == b"FRM8" and data[12:16] == b"DSD ":
            found = _walk_dff(data)
        else:
            raise Refusal(NOT_DSD, 0)
    except Refusal as r:
        return dict(none, status=r.status, error_offset=r.at)
    kind, total, at = found["kind"], found["chunks_total"], found["data_offset"]
    # the count is monotone: chunk j + 1 ends behind chunk j
    lo, hi = 0, min(total, len(data))
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if chunk_is_present(kind, data, at, mid - 1):
            lo = mid
        else:
            hi = mid - 1
    available = lo
    assert available == total or not chunk_is_present(kind, data, at, available)
    assert available == 0 or chunk_is_present(kind, data, at, available - 1)
    cpb = DT.chunks_per_block(W, P)
    room = (1 << 62 if dst_bytes_capacity is None else dst_bytes_capacity) // (W * 4) * cpb
    n = min(available - chunk_first, room) if chunk_first < available else 0
    ends = n > 0 and chunk_first + n == total
    if not ends:
        n -= n % cpb
    audio = data[at:]
    out = []
    for j in range(chunk_first, chunk_first + n):
        out += DT.chunk_bytes(kind, P, audio, j)
    while len(out) % (W * 4):
        out.append(DT.SILENCE)
    blocks = bytes(out)
    if chunk_first == 0 and 0 < n <= 600:                # the same bytes as the packer layer's descriptor of n chunks
        need, _ = DT.layout(kind, W, P, n)
        assert blocks == DT.convert(kind, W, P, audio[:need] + bytes(max(0, need - len(audio))), n)
    return dict(found, status=OK, channels=2, chunks_available=available, chunks_written=n, bytes_written=len(blocks), error_offset=0, blocks=blocks)


def seek(kind, sample):
    """(chunk_first, sample_rounded): the reference's rounding, to a pair of DSF planes or to DFF's 2048-sample grid."""
    rounded = sample & ~((32768 if kind == DSF else 2048) - 1)
    return rounded // 16, rounded


# ---- the writer
class Written:
    """data: the file.  kind, rate, sample_count, chunks_total, data_offset, data_bytes, format_version, channel_type, metadata; left,
    right: the channels' streams, a byte per eight samples, the earliest sample in the top bit; marks: name -> chunk position."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def blocks(self, W, P, first=0, count=None):
        """Chunks [first, first + count) in the pipeline's format straight from the streams, 0x69 up to the end of the last block."""
        count = self.chunks_total - first if count is None else count
        out, pad = bytearray(), bytes(P // 2)
        for j in range(first, first + count):
            out += pad + self.left[2 * j:2 * j + 2] + pad + self.right[2 * j:2 * j + 2]
        while len(out) % (W * 4):
            out.append(DT.SILENCE)
        return bytes(out)


def dsf(left, right, *, rate=2822400, sample_count=None, fmt_size=52, version=1, format_id=0, channel_type=2, channels=2, bits=1, block=PLANE, metadata=0,
        total=None, data_size=None, dsd_size=28, fmt_id=b"fmt ", data_id=b"data", tail=b""):
    assert len(left) == len(right)
    samples = 8 * len(left) if sample_count is None else sample_count
    audio = DT.dsf_image(bytes(DT.reverse_bits(b) for b in left), bytes(DT.reverse_bits(b) for b in right))
    fmt = fmt_id + struct.pack("<QIIIIIIQII", fmt_size, version, format_id, channel_type, channels, rate, bits, samples, block, 0) + bytes(max(0, fmt_size - 52))
    body = fmt + data_id + struct.pack("<Q", 12 + len(audio) if data_size is None else data_size) + audio + tail
    whole = 28 + len(body)
    data = b"DSD " + struct.pack("<QQQ", dsd_size, whole if total is None else total, metadata) + body
    return Written(data=data, kind=DSF, rate=rate, sample_count=samples, chunks_total=samples // 16, data_offset=28 + len(fmt) + 12, data_bytes=len(audio),
                   format_version=version, channel_type=channel_type, metadata=metadata, left=bytes(left), right=bytes(right),
                   marks={"DSD ": 0, "fmt ": 28, "data": 28 + len(fmt)})


def dff_chunk(name, payload, stated=None):
    return name + struct.pack(">Q", len(payload) if stated is None else stated) + payload + (b"\0" if len(payload) % 2 else b"")


def dff(left, right, *, rate=2822400, channels=2, cmpr=b"DSD ", fver=b"\x01\x05\x00\x00", locals_before=(), locals_after=(), before=(), between=(), behind=(),
        dsd_first=False, prop_type=b"SND ", omit=(), audio_size=None, audio_id=b"DSD "):
    """locals_*, before, between, behind: (id, payload) chunks laid in as they are; omit: local chunk ids to leave out."""
    assert len(left) == len(right) and len(left) % 2 == 0
    audio = bytes(b for pair in zip(left, right) for b in pair)
    name = b"not compressed"
    local = [(b"FS  ", struct.pack(">I", rate)), (b"CHNL", struct.pack(">H", channels) + b"SLFTSRGT"[:4 * channels] + b"C000" * max(0, channels - 2)),
             (b"CMPR", cmpr + bytes([len(name)]) + name)]
    local = list(locals_before) + [c for c in local if c[0] not in omit] + list(locals_after)
    prop = (b"PROP", prop_type + b"".join(dff_chunk(*c) for c in local))
    sound = (audio_id, audio)
    chunks = ([(b"FVER", fver)] if fver is not None else []) + list(before) + ([sound] + list(between) + [prop] if dsd_first else [prop] + list(between) + [sound]) + list(behind)
    body, marks = bytearray(), {}
    for c in chunks:
        marks.setdefault(c[0].decode(), 16 + len(body))
        body += dff_chunk(c[0], c[1], audio_size if c is sound else None)
    data = b"FRM8" + struct.pack(">Q", 4 + len(body)) + b"DSD " + bytes(body)
    stated = len(audio) if audio_size is None else audio_size
    return Written(data=data, kind=DFF, rate=rate, sample_count=16 * (stated // 4), chunks_total=stated // 4, data_offset=marks[audio_id.decode()] + 12, data_bytes=stated,
                   format_version=struct.unpack(">I", fver)[0] if fver is not None else 0, channel_type=0, metadata=0, left=bytes(left), right=bytes(right), marks=marks)
