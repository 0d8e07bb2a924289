"""One Songcast (OHM) audio datagram and the sender's audio in front of it, from the wire's definition: struct.pack of the header
fields in the order oracle/ohp_songcast.h documents for the wire, re-read from the reference's field table (OhmMsg.cpp: Serialise
writes the per-frame fields, GetStreamHeader the per-stream ones; Ohm.cpp: OhmHeader::Externalise).  It calls neither the oracle
nor the library.  The frame layout is PARITY UNPINNED in the reference (no golden datagram exists): this is a second reading of the
same table, not a copy of the first.

  "Ohm " | major 1 | type 3 (audio) | u16 total bytes (8 + 28 + stream header + audio)
  u8 50 (OhmMsgAudio::kHeaderBytes) | u8 flags | u16 samples | u32 frame | u32 network timestamp | u32 media latency |
  u32 media timestamp | u64 sample start
  u64 samples total | u32 sample rate | u32 bit rate | i16 volume offset | u8 bit depth | u8 channels | u8 0 | u8 codec bytes | codec
  audio: big-endian, at most two channels (the first two; channels 8 and 9 of a stream of ten or more), at most 24 bits
All integers big-endian.  A sender that timestamps sets BOTH timestamp flags (ReinitialiseFields: iTimestamped2 = iTimestamped) and
always writes media timestamp 0.
"""
import struct

FLAG_HALT, FLAG_LOSSLESS, FLAG_TIMESTAMPED, FLAG_RESENT, FLAG_TIMESTAMPED2 = 1, 2, 4, 8, 16
AUDIO_HEADER_BYTES = 50
MAX_CODEC_BYTES = 29
MAX_SAMPLE_BYTES = 5760
JIFFIES_PER_MS = 56448
PACKET_JIFFIES = 5 * JIFFIES_PER_MS


def stream_header(samples_total, sample_rate, bit_rate, volume_offset, bit_depth, channels, codec=b""):
    assert len(codec) <= MAX_CODEC_BYTES
    return struct.pack(">QIIhBBBB", samples_total, sample_rate, bit_rate, volume_offset, bit_depth, channels, 0, len(codec)) + bytes(codec)


def audio_frame(flags, samples, frame, network_timestamp, media_latency, sample_start, stream_hdr, audio, media_timestamp=0):
    """flags: FLAG_HALT | FLAG_LOSSLESS | FLAG_TIMESTAMPED | FLAG_RESENT as the sender is told; the wire adds FLAG_TIMESTAMPED2."""
    wire_flags = flags & (FLAG_HALT | FLAG_LOSSLESS | FLAG_TIMESTAMPED | FLAG_RESENT)
    if flags & FLAG_TIMESTAMPED:
        wire_flags |= FLAG_TIMESTAMPED2
    per_frame = struct.pack(">BBHIIIIQ", AUDIO_HEADER_BYTES, wire_flags, samples, frame, network_timestamp, media_latency,
                            media_timestamp, sample_start)
    assert len(per_frame) == 28
    total = 8 + len(per_frame) + len(stream_hdr) + len(audio)
    return b"Ohm " + struct.pack(">BBH", 1, 3, total) + per_frame + bytes(stream_hdr) + bytes(audio)


def wire_format(channels, bits):
    """(channels, bits) of the audio on the wire for a source of `channels` x `bits`."""
    return min(channels, 2), min(bits, 24)


def sender_audio(pcm_be, channels, bits):
    """What the sender's processor appends for big-endian interleaved PCM: per frame the first two channels (from channel 8 when the
    stream has ten or more; one channel for mono), the most significant min(bytes, 3) bytes of each."""
    nbytes = bits // 8
    frame_bytes = channels * nbytes
    assert len(pcm_be) % frame_bytes == 0
    first = 8 if channels >= 10 else 0
    keep = min(nbytes, 3)
    out = bytearray()
    for f in range(len(pcm_be) // frame_bytes):
        for c in range(first, first + min(channels, 2)):
            at = f * frame_bytes + c * nbytes
            out += bytes(pcm_be[at:at + keep])
    return bytes(out)


def packet_cuts(msg_jiffies, flush=True):
    """The 5 ms packetiser's cut points (Sender::ProcessAudio): messages wait until five milliseconds' worth of jiffies is pending;
    the message that reaches it is split exactly there, the packet goes out, and the rest is cut into further whole packets while
    it is long enough; what is left waits.  Returns the packets, each a list of (message index, jiffies taken from it); with
    `flush` the audio still pending at the end goes out as a last (short) packet."""
    packets, pending, pending_jiffies = [], [], 0
    for i, size in enumerate(msg_jiffies):
        if pending_jiffies + size < PACKET_JIFFIES:
            pending.append((i, size))
            pending_jiffies += size
            continue
        left = size
        while pending_jiffies + left >= PACKET_JIFFIES:
            take = PACKET_JIFFIES - pending_jiffies
            packets.append(pending + [(i, take)])
            pending, pending_jiffies = [], 0
            left -= take
        if left > 0:
            pending, pending_jiffies = [(i, left)], left
    if flush:
        packets.append(pending)
    return packets
