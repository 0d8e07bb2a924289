"""The three layout-changing processors behind ohgpu_fmt_batch_create / ohgpu_fmt_batch_run, from their definitions: plain Python
integers over `bytes`, one loop over frames and channels per kind, written from the reference's three functions

    a11  OHGPU_FMT_UNPACK_PLANAR  FlywheelInput::DoProcessFragment + AppendSubsample8/16/24/32   Pipeline/StarvationRamper.cpp:117-186
    a13  OHGPU_FMT_SENDER_PACK    Sender::DoProcessFragment, Sender::FirstChannelToSend          Av/Songcast/Sender.cpp:350-377
    a14  OHGPU_FMT_FLAC_PACK      CodecFlac::CallbackWrite                                       Codec/Flac.cpp:379-417

and from include/ohgpu.h's description of ohgpu_fmt_desc -- not from the oracle's restatement, not from the generic device kernel,
and not as an index map: each function keeps the reference's moving read and write positions and nothing else.  It knows nothing
of chunks, routes, alignment or wide loads.  tests/test_fmt_textbook.py ties it to the oracle byte for byte and to answers written
out by hand; tests/test_gpu_fmt_textbook.py holds every device route against it.

A descriptor is anything indexable by the field names of capi.FMT_DESC (a numpy record or a dict).  Each kind's function returns
the pieces it writes as [(destination offset, bytes)]; batch_bytes() lays a batch's pieces into a filled arena.

Where the reference leaves a reading open, and which one this model takes:

  * a13, two copies per frame whatever the channel count.  Sender::DoProcessFragment always does two memcpys per frame (the
    subsample at `src` and the one at `src + aBytesPerSubsample`) and then advances dst by outputChannels * dstBytesPerSubsample.
    For a MONO stream the second copy therefore takes the first bytes of the NEXT frame and puts them where the next iteration's
    first copy writes the very same bytes again; only the last frame's second copy survives, and it reads past the fragment and
    lands past totalBytesToCopy, the only bytes iAudioBuf->SetBytes counts.  The ABI's contract (like the oracle's) is the counted
    bytes only: the model performs both copies into a buffer with room for the stray one (reading zeros past the fragment) and
    returns the counted bytes.  A device kernel must not write the stray bytes: whole-arena comparisons see them if it does.
  * a13, which channels.  FirstChannelToSend is `(aNumChannels < 10) ? 0 : 8` under its own "FIXME: review how this mapping is
    generated".  The model takes the code as it stands: channels 0 and 1 below ten channels, 8 and 9 at ten.  (Sender::
    ProcessFragment is only told about up to ten channels; ohgpu_fmt_desc admits 1..10.)
  * a13, depth.  dstBytesPerSubsample = min(aBytesPerSubsample, 3): a 32-bit subsample loses its FOURTH (least significant, the
    data is big endian) byte; nothing is rounded.
  * a14, truncation.  `TUint subsample = aBuffer[j][i]` followed by `(TByte)(subsample >> 8)` ... keeps the LOW bitDepth bits of
    the TInt32 and drops whatever lies above them, silently: a plane value outside the stream's depth is not clipped, not
    refused.  The model does the same arithmetic on the value taken modulo 2^32.
  * a14, 32 bits.  The switch has cases 8, 16 and 24 only; anything else throws CodecStreamFeatureUnsupported.  The model raises
    Unsupported (the ABI: OHGPU_ERR_UNSUPPORTED).  The planes are host-endian TInt32; every host this project builds for is little
    endian, and so is the model's reading of the source arena.
  * a14, iBuf.  CallbackWrite fills iBuf, hands it to OutputAudioPcm and starts again when a block exceeds it; the concatenation of
    those buffers is what one descriptor writes.
  * a11, write positions.  FlywheelInput keeps one write pointer per channel (iChannelPtr[j], set by Prepare() to consecutive
    planes of channelBytes each) and every fragment appends to them.  One descriptor stands for one fragment: dst_offset is
    iChannelPtr[0] at the fragment's start and dst_plane_stride is channelBytes, so channel j's pointer is dst_offset + j *
    dst_plane_stride; the bytes of a plane beyond the fragment's frames are not touched.  ProcessSilence is the same function.
  * a11 and a13 count frames by integer division of the fragment's bytes; a descriptor gives n_frames and the fragment is exactly
    n_frames * channels * bytes long, so no remainder arises.
"""

UNPACK_PLANAR, SENDER_PACK, FLAC_PACK = 1, 2, 3


class Unsupported(Exception):
    """CodecFlac::CallbackWrite's THROW(CodecStreamFeatureUnsupported)."""


def _fields(d):
    return {k: int(d[k]) for k in ("src_offset", "dst_offset", "src_plane_stride", "dst_plane_stride", "n_frames", "kind", "channels",
                                   "src_bits", "dst_bits")}


def unpack_planar(d, src):
    """FlywheelInput::DoProcessFragment: for every sample, for every channel, AppendSubsampleN(iChannelPtr[j], src)."""
    f = _fields(d)
    channels, subsample_bytes, frames = f["channels"], f["src_bits"] // 8, f["n_frames"]
    assert subsample_bytes in (1, 2, 3, 4)                              # default: ASSERTS()
    data = bytes(src[f["src_offset"]:f["src_offset"] + frames * channels * subsample_bytes])
    assert len(data) == frames * channels * subsample_bytes
    planes = [bytearray() for _ in range(channels)]                     # what each iChannelPtr[j] has been advanced over
    p = 0                                                               # `src`
    for _ in range(frames):
        for j in range(channels):
            for k in range(4):                                          # AppendSubsample8/16/24/32: N source bytes, then zeros
                if k < subsample_bytes:
                    planes[j].append(data[p])
                    p += 1
                else:
                    planes[j].append(0)
    return [(f["dst_offset"] + j * f["dst_plane_stride"], bytes(planes[j])) for j in range(channels)]


def first_channel_to_send(channels):
    return 0 if channels < 10 else 8


def sender_pack(d, src):
    """Sender::DoProcessFragment; the counted bytes (totalBytesToCopy) only."""
    f = _fields(d)
    channels, bytes_per_subsample, frames = f["channels"], f["src_bits"] // 8, f["n_frames"]
    stride = bytes_per_subsample * channels
    data = bytes(src[f["src_offset"]:f["src_offset"] + frames * stride])
    assert len(data) == frames * stride
    data += bytes(2 * bytes_per_subsample)                              # (what a mono stream's last second copy reads: not ours)
    dst_bytes_per_subsample = min(bytes_per_subsample, 3)
    output_channels = min(channels, 2)
    total_bytes_to_copy = frames * output_channels * dst_bytes_per_subsample
    buf = bytearray(total_bytes_to_copy + 2 * dst_bytes_per_subsample)
    s = bytes_per_subsample * first_channel_to_send(channels)
    o = 0
    for _ in range(frames):
        for k in range(dst_bytes_per_subsample):                        # memcpy(dst, src, dstBytesPerSubsample)
            buf[o + k] = data[s + k]
        for k in range(dst_bytes_per_subsample):                        # memcpy(dst + dstBytesPerSubsample, src + aBytesPerSubsample, ...)
            buf[o + dst_bytes_per_subsample + k] = data[s + bytes_per_subsample + k]
        s += stride
        o += output_channels * dst_bytes_per_subsample
    return [(f["dst_offset"], bytes(buf[:total_bytes_to_copy]))]


def flac_pack(d, src):
    """CodecFlac::CallbackWrite over planes of little-endian TInt32."""
    f = _fields(d)
    channels, bit_depth, frames = f["channels"], f["dst_bits"], f["n_frames"]
    if bit_depth not in (8, 16, 24):
        raise Unsupported(bit_depth)
    out = bytearray()
    for i in range(frames):
        for j in range(channels):
            at = f["src_offset"] + j * f["src_plane_stride"] + 4 * i
            word = bytes(src[at:at + 4])
            assert len(word) == 4
            subsample = int.from_bytes(word, "little")                  # TUint subsample = aBuffer[j][i]
            if bit_depth == 8:
                out.append(subsample & 0xFF)
            elif bit_depth == 16:
                out.append((subsample >> 8) & 0xFF)
                out.append(subsample & 0xFF)
            else:
                out.append((subsample >> 16) & 0xFF)
                out.append((subsample >> 8) & 0xFF)
                out.append(subsample & 0xFF)
    return [(f["dst_offset"], bytes(out))]


KINDS = {UNPACK_PLANAR: unpack_planar, SENDER_PACK: sender_pack, FLAC_PACK: flac_pack}


def pieces(d, src):
    return KINDS[int(d["kind"])](d, src)


def batch_bytes(descs, src, dst_bytes, fill=0xA5):
    """The whole destination arena after the batch: `fill` wherever no descriptor writes."""
    src = bytes(src)
    dst = bytearray([fill]) * dst_bytes
    for d in descs:
        for off, b in pieces(d, src):
            assert off + len(b) <= dst_bytes or not b, (off, len(b), dst_bytes)
            dst[off:off + len(b)] = b
    return bytes(dst)


def source_span(d):
    """(first byte, one past the last byte) of the source arena that a descriptor's fragment occupies; (0, 0) for no frames."""
    f = _fields(d)
    if f["n_frames"] == 0:
        return 0, 0
    if f["kind"] == FLAC_PACK:
        return f["src_offset"], f["src_offset"] + (f["channels"] - 1) * f["src_plane_stride"] + 4 * f["n_frames"]
    return f["src_offset"], f["src_offset"] + f["n_frames"] * f["channels"] * (f["src_bits"] // 8)


def totals(descs, src):
    """What ohgpu_batch_info reports for the batch: frames, and the byte spans each descriptor reads and writes (first byte to
    last, gaps between an a11 descriptor's planes included)."""
    src = bytes(src)
    frames = s_bytes = d_bytes = 0
    for d in descs:
        frames += int(d["n_frames"])
        lo, hi = source_span(d)
        s_bytes += hi - lo
        ps = [(off, off + len(b)) for off, b in pieces(d, src) if b]
        if ps:
            d_bytes += max(e for _, e in ps) - min(o for o, _ in ps)
    return {"n_msgs": len(descs), "in_frames": frames, "out_frames": frames, "src_bytes_touched": s_bytes, "dst_bytes_written": d_bytes}
