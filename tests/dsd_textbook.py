"""A textbook model of DSD in the pipeline: the three codec-side packers (DSF, DFF, raw), the playable pass-through, DSD silence
and the tail fill -- written from the description of the format, one byte at a time, sharing nothing with the kernels
(ohpipeline_amd/csrc/dsd_line_kernel.hip) or the library's validation.  numpy holds the bytes; every index is spelt out.

The format.  DSD audio in the pipeline is a run of SAMPLE BLOCKS of W 32-bit words.  A block holds W * 4 / (4 + P) CHUNKS, where
P is the number of pad bytes per chunk, and a chunk is

    [P/2 x 00]  L  L  [P/2 x 00]  R  R

that is, sixteen one-bit samples of the left channel (two bytes, the earliest sample in the top bit of the first), then sixteen of
the right, each pair of bytes preceded by half of the padding.  W * 4 must be a whole number of chunks AND W - P must be that
number: so either P == 0 (W chunks of 4 bytes) or W == P + 4 with P even (4 chunks of 4 + P bytes).

The packers make chunks from what a file holds:

    DSF   the file is pairs of 4096-byte blocks, one of the left channel, then one of the right, bits LSB first.  Chunk j takes
          bytes 2j and 2j + 1 of the left STREAM and the same two of the right, each with its bits reversed.
    DFF   the file is bytes L R L R ..., MSB first.  Chunk j takes file bytes 4j .. 4j + 3 = (l0, r0, l1, r1) -> l0 l1 | r0 r1.
    raw   the source is already L L R R.  Chunk j takes source bytes 4j .. 4j + 3 = (l0, l1, r0, r1) -> l0 l1 | r0 r1.

The output of n chunks is ceil(n / chunks per block) whole blocks: the chunks, then 0x69 in EVERY remaining byte of the last
block.  Raw, pass-through and silence exist only in whole blocks.  Pass-through copies n * (4 + P) bytes unchanged; silence is
0x69 in every byte.

Worked bytes (W = 6, P = 2), kept as literals in WORKED and checked by tests/test_dsd_textbook.py:

    DSF   left 00 01 02 03, right 80 81 82 83  ->  00 00 80 00 01 81 | 00 40 C0 00 41 C1
    DFF   11 22 33 44                          ->  00 11 33 00 22 44
    raw   11 22 33 44                          ->  00 11 22 00 33 44
    DFF with P = 0 (W = 1)                     ->  11 33 22 44
    five DSF or DFF chunks                     ->  30 bytes of chunks, 18 bytes of 69: two blocks, 48 bytes
"""
import numpy as np

PASS, DSF, DFF, RAW = 1, 2, 3, 4
FLAG_SILENCE = 1
SILENCE = 0x69
DSF_BLOCK = 4096

WORKED = [
    # (kind, W, P, source bytes (DSF: left, right), chunks, output)
    (DSF, 6, 2, (bytes.fromhex("00010203"), bytes.fromhex("80818283")), 2, bytes.fromhex("000080000181" "0040C00041C1")),
    (DFF, 6, 2, bytes.fromhex("11223344"), 1, bytes.fromhex("001133002244")),
    (RAW, 6, 2, bytes.fromhex("11223344"), 1, bytes.fromhex("001122003344")),
    (DFF, 1, 0, bytes.fromhex("11223344"), 1, bytes.fromhex("11332244")),
]


class Refused(ValueError):
    """What the library answers with OHGPU_ERR_INVALID."""


def chunks_per_block(W, P):
    """The chunks in a sample block, or Refused for a pair the format does not have."""
    if not 1 <= W <= 255 or P < 0 or P % 2 != 0:
        raise Refused(f"W = {W}, P = {P}")
    if (W * 4) % (4 + P) != 0 or (W * 4) // (4 + P) != W - P:
        raise Refused(f"W = {W}, P = {P}: {W * 4} bytes are not W - P chunks of {4 + P}")
    return W - P


def reverse_bits(byte):
    """Bit 0 becomes bit 7, bit 1 becomes bit 6, ..."""
    out = 0
    for k in range(8):
        if byte & (1 << k):
            out |= 1 << (7 - k)
    return out


def dsf_stream_byte(src, channel, i):
    """Byte i of a channel's stream in a DSF file image: block i // 4096 of that channel, which is block 2 * (i // 4096) +
    channel of the file."""
    block, within = i // DSF_BLOCK, i % DSF_BLOCK
    return src[(2 * block + channel) * DSF_BLOCK + within]


def chunk_bytes(kind, P, src, j):
    """Chunk j as a list of 4 + P byte values."""
    if kind == PASS:
        return [src[j * (4 + P) + k] for k in range(4 + P)]
    if kind == DSF:
        l0, l1 = reverse_bits(dsf_stream_byte(src, 0, 2 * j)), reverse_bits(dsf_stream_byte(src, 0, 2 * j + 1))
        r0, r1 = reverse_bits(dsf_stream_byte(src, 1, 2 * j)), reverse_bits(dsf_stream_byte(src, 1, 2 * j + 1))
    elif kind == DFF:
        l0, r0, l1, r1 = src[4 * j], src[4 * j + 1], src[4 * j + 2], src[4 * j + 3]
    elif kind == RAW:
        l0, l1, r0, r1 = src[4 * j], src[4 * j + 1], src[4 * j + 2], src[4 * j + 3]
    else:
        raise Refused(f"kind {kind}")
    pad = [0] * (P // 2)
    return pad + [l0, l1] + pad + [r0, r1]


def layout(kind, W, P, n_chunks, silence=False):
    """(source bytes read from the descriptor's source offset on, destination bytes written), or Refused."""
    if kind not in (PASS, DSF, DFF, RAW):
        raise Refused(f"kind {kind}")
    per_block = chunks_per_block(W, P)
    if (silence or kind in (RAW, PASS)) and n_chunks % per_block != 0:
        raise Refused(f"{n_chunks} chunks are not whole blocks of {per_block}")
    blocks = (n_chunks + per_block - 1) // per_block
    if silence:
        src_bytes = 0
    elif kind == DSF:
        pairs = (n_chunks + DSF_BLOCK // 2 - 1) // (DSF_BLOCK // 2)      # a pair of blocks holds 2048 chunks' worth
        src_bytes = pairs * 2 * DSF_BLOCK
    elif kind == PASS:
        src_bytes = n_chunks * (4 + P)
    else:
        src_bytes = n_chunks * 4
    return src_bytes, blocks * W * 4


def convert(kind, W, P, src, n_chunks, silence=False):
    """The output bytes of one descriptor whose source starts at src[0]."""
    _, dst_bytes = layout(kind, W, P, n_chunks, silence)
    out = []
    if not silence:
        for j in range(n_chunks):
            out += chunk_bytes(kind, P, src, j)
    while len(out) < dst_bytes:
        out.append(SILENCE)
    assert len(out) == dst_bytes
    return bytes(out)


def dsf_image(left, right):
    """A DSF file's sample data from the two channels' streams (each padded with zeros to whole 4096-byte blocks, as a file's
    last block is)."""
    assert len(left) == len(right)
    blocks = (len(left) + DSF_BLOCK - 1) // DSF_BLOCK
    out = bytearray()
    for b in range(blocks):
        for stream in (left, right):
            part = stream[b * DSF_BLOCK:(b + 1) * DSF_BLOCK]
            out += part + bytes(DSF_BLOCK - len(part))
    return bytes(out)


def _field(d, name):
    v = d[name]
    return int(v)


def batch_bytes(descs, src, dst_bytes, fill):
    """The whole destination arena after a batch: `fill` wherever no descriptor writes.  descs: a numpy array of capi.DSD_DESC or
    a list of dicts with its fields.  Refused / IndexError for what the library refuses."""
    out = np.full(dst_bytes, fill, dtype=np.uint8)
    src = bytes(src)
    for d in descs:
        n, kind, W, P = _field(d, "n_chunks"), _field(d, "kind"), _field(d, "sample_block_words"), _field(d, "pad_bytes_per_chunk")
        silence = bool(_field(d, "flags") & FLAG_SILENCE)
        src_need, dst_need = layout(kind, W, P, n, silence)
        if n == 0:
            continue
        so, do = _field(d, "src_offset"), _field(d, "dst_offset")
        if (src_need and so + src_need > len(src)) or do + dst_need > dst_bytes:     # (a silent descriptor's source offset means nothing)
            raise IndexError("descriptor outside the arenas")
        got = convert(kind, W, P, src[so:so + src_need], n, silence)
        out[do:do + dst_need] = np.frombuffer(got, dtype=np.uint8)
    return out.tobytes()


def totals(descs):
    """What ohgpu_batch_info reports for the batch."""
    t = {"n_msgs": len(descs), "in_frames": 0, "out_frames": 0, "src_bytes_touched": 0, "dst_bytes_written": 0}
    for d in descs:
        n = _field(d, "n_chunks")
        s, o = layout(_field(d, "kind"), _field(d, "sample_block_words"), _field(d, "pad_bytes_per_chunk"), n,
                      bool(_field(d, "flags") & FLAG_SILENCE))
        t["in_frames"] += n
        t["out_frames"] += n
        t["src_bytes_touched"] += s
        t["dst_bytes_written"] += o
    return t
