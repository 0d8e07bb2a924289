"""An independent model of the PCM file layer (ohgpu_iff_*, include/ohgpu.h's IFF section): file bytes and descriptor fields in, the
result record and the PCM bytes out.  Written from the rules of that section with slices and int.from_bytes; it shares no table and no
helper with csrc/iff_chunk_core.h.

Where the rules differ from the reference (CodecWav, CodecAiffBase, CodecAiff, CodecAifc), on purpose:
  - either order of `fmt ` / `data` and of `COMM` / `SSND` is read (the reference streams and wants the format first);
  - an odd `data` size does not count its pad byte as audio (the reference's chunk search returns the padded size);
  - an extensible format whose sub-format is not PCM is UNSUPPORTED (the reference does not look);
  - a 20-bit AIFF sample has three bytes (the reference computes two and reports 24 bits);
  - 32-bit AIFF is read (the reference refuses it);
  - SSND's offset field is honoured, and the audio's size is held against the chunk's size without its 8 header bytes;
  - one formula turns the 80-bit rate into a number for every exponent (the reference's branch from 0x4013 up shifts by e - 0x4007);
  - the flag WAV8_UNSIGNED has no counterpart; without it 8-bit WAV is copied as the reference copies it."""

import numpy as np

OK, NOT_IFF, TRUNCATED, INVALID, UNSUPPORTED = range(5)
WAV, AIFF, AIFC = 1, 2, 3
LITTLE, BIG = 1, 2
MAX_CHUNKS, MAX_CHANNELS = 4096, 10
FLAG_WAV8_UNSIGNED = 1


class Refused(Exception):
    def __init__(self, status, at):
        self.status, self.at = status, at


def _u(data, at, width, order):
    return int.from_bytes(data[at:at + width], order)


def _wav_format(data, chunk, pay, size):
    tag, channels = _u(data, pay, 2, "little"), _u(data, pay + 2, 2, "little")
    rate, byte_rate = _u(data, pay + 4, 4, "little"), _u(data, pay + 8, 4, "little")
    depth = _u(data, pay + 14, 2, "little")
    if tag not in (1, 0xfffe):
        raise Refused(UNSUPPORTED, chunk)
    if tag == 0xfffe and size == 40 and _u(data, pay + 24, 2, "little") != 1:
        raise Refused(UNSUPPORTED, chunk)
    if channels == 0:
        raise Refused(INVALID, chunk)
    if channels > MAX_CHANNELS:
        raise Refused(UNSUPPORTED, chunk)
    if rate == 0 or byte_rate == 0:
        raise Refused(INVALID, chunk)
    if depth == 0 or depth % 8:
        raise Refused(INVALID, chunk)
    if depth > 32:
        raise Refused(UNSUPPORTED, chunk)
    return dict(channels=channels, rate=rate, depth=depth, sample_bytes=depth // 8, little=True, bit_rate=(byte_rate * 8) % 2 ** 32)


def extended_rate(ten):
    """The 80-bit number of a COMM chunk as a sample rate; None: not one."""
    head, mantissa = int.from_bytes(ten[:2], "big"), int.from_bytes(ten[2:10], "big")
    if head & 0x8000 or not 0x3fff <= head <= 0x401e:
        return None
    rate = (mantissa >> 32) >> (0x401e - head)
    return {22255: 22050, 11127: 11025}.get(rate, rate) or None


def _comm(data, chunk, pay, aifc):
    channels, frames, depth = _u(data, pay, 2, "big"), _u(data, pay + 2, 4, "big"), _u(data, pay + 6, 2, "big")
    if channels == 0:
        raise Refused(INVALID, chunk)
    if channels > MAX_CHANNELS:
        raise Refused(UNSUPPORTED, chunk)
    if depth not in (8, 16, 20, 24, 32):
        raise Refused(UNSUPPORTED, chunk)
    rate = extended_rate(data[pay + 8:pay + 18])
    if rate is None:
        raise Refused(INVALID, chunk)
    little = False
    if aifc:
        how = bytes(data[pay + 18:pay + 22])
        if how in (b"sowt", b"SOWT"):
            little = True
        elif how != b"NONE":
            raise Refused(UNSUPPORTED, chunk)
    sample_bytes = -(-depth // 8)
    return dict(channels=channels, rate=rate, depth=24 if depth == 20 else depth, sample_bytes=sample_bytes, little=little,
                bit_rate=(rate * channels * sample_bytes * 8) % 2 ** 32), frames


def _walk(data):
    n = len(data)
    if n < 12:
        raise Refused(NOT_IFF, 0)
    form, kind_id = bytes(data[0:4]), bytes(data[8:12])
    kind = {(b"RIFF", b"WAVE"): WAV, (b"FORM", b"AIFF"): AIFF, (b"FORM", b"AIFC"): AIFC}.get((form, kind_id))
    if kind is None:
        raise Refused(NOT_IFF, 0)
    wav = kind == WAV
    order = "little" if wav else "big"
    continuous = wav and _u(data, 4, 4, "little") == 0
    fmt, audio, frames = None, None, 0
    pos, seen = 12, 0
    while fmt is None or audio is None:
        seen += 1
        if seen > MAX_CHUNKS:
            raise Refused(INVALID, pos)
        if pos + 8 > n:
            raise Refused(TRUNCATED, pos)
        name, size, pay = bytes(data[pos:pos + 4]), _u(data, pos + 4, 4, order), pos + 8
        if name == (b"fmt " if wav else b"COMM") and fmt is None:
            good = size in (16, 18, 40) if wav else size == 18 if kind == AIFF else size >= 22
            if not good:
                raise Refused(INVALID, pos)
            if pay + size > n:
                raise Refused(TRUNCATED, pos)
            if wav:
                fmt = _wav_format(data, pos, pay, size)
            else:
                fmt, frames = _comm(data, pos, pay, kind == AIFC)
        elif name == (b"data" if wav else b"SSND") and audio is None:
            if wav:
                if continuous and fmt is None:
                    raise Refused(INVALID, pos)
                audio = (pos, pay, n - pay if continuous else size)
            else:
                if size < 8:
                    raise Refused(INVALID, pos)
                if pay + 8 > n:
                    raise Refused(TRUNCATED, pos)
                offset = _u(data, pay, 4, "big")
                if offset > size - 8:
                    raise Refused(INVALID, pos)
                audio = (pos, pay + 8 + offset, size - 8 - offset)
        pos = pay + size + size % 2
    chunk, start, held = audio
    frame_bytes = fmt["channels"] * fmt["sample_bytes"]
    if wav:
        stated, total = held, held // frame_bytes
    else:
        stated, total = frames * frame_bytes, frames
        if stated > held:
            raise Refused(INVALID, chunk)
    present = max(n - start, 0)
    return kind, fmt, start, stated, 0 if continuous else total, min(stated, present) // frame_bytes


def read(data, *, flags=0, frame_first=0, dst_frame_capacity=1 << 31, dst_bytes_capacity=None, max_bit_depth=24):
    """The result record as a dict (the fields of ohgpu_iff_stream_result) with "pcm": the bytes the stream writes at dst_offset."""
    blank = dict(status=OK, kind=0, channels=0, sample_rate=0, src_bit_depth=0, out_bit_depth=0, src_endian=0, bit_rate=0, frames_total=0, frames_available=0,
                 frames_written=0, data_offset=0, data_bytes=0, error_offset=0, pcm=b"")
    try:
        kind, fmt, start, stated, total, available = _walk(data)
    except Refused as r:
        return dict(blank, status=r.status, error_offset=r.at)
    out_depth = min(fmt["depth"], max_bit_depth)
    out_bytes, in_bytes, channels = out_depth // 8, fmt["sample_bytes"], fmt["channels"]
    room = dst_frame_capacity * 40 if dst_bytes_capacity is None else dst_bytes_capacity
    n = min(max(available - frame_first, 0), dst_frame_capacity, room // (channels * out_bytes))
    at = start + frame_first * channels * in_bytes
    flip = 0x80 if kind == WAV and fmt["depth"] == 8 and flags & FLAG_WAV8_UNSIGNED else 0
    samples = np.frombuffer(bytes(data[at:at + n * channels * in_bytes]), dtype=np.uint8).reshape(n * channels, in_bytes)
    top_first = samples[:, ::-1] if fmt["little"] else samples
    pcm = (top_first[:, :out_bytes] ^ flip).astype(np.uint8).tobytes()
    return dict(blank, kind=kind, channels=channels, sample_rate=fmt["rate"], src_bit_depth=fmt["depth"], out_bit_depth=out_depth,
                src_endian=LITTLE if fmt["little"] else BIG, bit_rate=fmt["bit_rate"], frames_total=total, frames_available=available, frames_written=n,
                data_offset=start, data_bytes=stated, pcm=pcm)
