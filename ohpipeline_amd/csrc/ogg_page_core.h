// ogg_page_core.h -- the Ogg page layer in front of the FLAC decoder: what stands between the bytes of an Ogg stream
// and the contiguous run of packet bytes a codec reads.  Every function is __host__ __device__: csrc/ogg_page_kernel.hip runs this text
// on the device, tests/cpp/ogg_core_driver.cpp runs the same text on the CPU under the sanitizers.
//
//   the page   0 "OggS" | 4 version | 5 flags (1 continued, 2 first page, 4 last page) | 6 i64 granule position | 14 u32 serial |
//              18 u32 page number | 22 u32 checksum | 26 n | 27 n lacing values | the body, as long as their sum.  Little-endian.
//   checksum   polynomial 0x04c11db7, register 0 at the start, most significant bit first, nothing reflected, nothing complemented,
//              over the whole page with bytes 22..25 read as zero.  With a zero start the register is a linear function of the bytes:
//              crc(A | B) = crc(A) * x^(8 |B|) + crc(B) in GF(2)[x] / P.  A page is therefore cut into contiguous slices, a lane each;
//              a lane runs its slice through the byte table and multiplies what it gets by x^(8 m), m the bytes behind its slice, and
//              the page's checksum is the sum (xor) over the lanes.  x^(8 m) = shift[m & 255] * shift256[m >> 8]: two table entries
//              and two 32-step multiplications a lane, for every m a page can have (m < 65307).
//   find       a byte position is a candidate when a whole page image starts there: "OggS", 27 + n bytes of header, the body the
//              lacing values add up to, all inside the stream's range.  Nothing else is asked of it (a page of version 1 is a page).
//   verify     the checksum of a candidate, lane by lane (crc_lane); a good one sets the position's bit in the batch's bitmap.
//   walk       one stream, from its first byte: the page at p is parsed again (27 + n bytes), its verdict is the bit of p, and the
//              next page is the one that starts where this one ends.  A candidate that the walk never stands on -- "OggS" inside a
//              body, even a whole valid page image there -- is never asked about.  The walk applies the rules of include/ohgpu.h's
//              Ogg section: pages of another serial or version are counted and passed over, the page numbers must follow one
//              another, lacing values join into packets across pages, the mapping's first header loses its nine bytes.  It writes
//              the packet records, the result, and the gather plan: pieces, each a run of body bytes that goes to the delivered run
//              as it lies.  A page gives one piece, and one more for every mapping header in it.  Only completed packets are
//              delivered: when the walk ends inside a packet, the pieces are cut back to where that packet began (truncate()).
//              With kFollowLinks it also follows a chained stream from one logical stream into the next (rules L1 ... L5 there): a
//              first page of another serial whose body begins with the descriptor's magic makes that serial the followed one, the
//              packet still open is cut away as at the end of a range, and the link's first packet is flagged.
//   gather     a piece is copied by csrc/ohm_rx_core.h's gather_lane: both ends at any byte address.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define OGGP_HD __host__ __device__ __forceinline__
#else
#define OGGP_HD inline
#endif

namespace oggpage {

enum { kHeaderBytes = 27, kMaxPageBytes = 27 + 255 + 255 * 255, kMappingHeaderBytes = 9 };
enum Status : uint32_t { kOk = 0, kLostSync = 1, kHole = 2, kNotFlac = 3, kUnsupportedMapping = 4, kBadResume = 5 };
enum { kAnySeq = 1, kFlacMapping = 2, kAnySerial = 4, kFollowLinks = 16, kKnownFlags = 23 };
enum { kPageContinued = 1, kPageBos = 2, kPageEos = 4 };
enum { kPacketBos = 1, kPacketEos = 2, kPacketMappingHeader = 4, kPacketLink = 8 };
enum { kMaxMagicBytes = 8 };
constexpr uint32_t kPoly = 0x04c11db7u;
constexpr uint32_t kLanes = 64, kSliceMin = 16;       // a page's slices: one a lane, none shorter than kSliceMin but the last

struct Stream {               // 64 bytes = ohgpu_ogg_stream_desc
    uint64_t src_offset, dst_offset, dst_capacity;
    uint32_t src_bytes, serial, expect_seq, packet_first, packet_capacity, first_page_segment, flags;
    uint32_t reserved[3];     // with kFollowLinks the link magic: [0] its length (0 ... 8), the eight bytes of [1] and [2] as they lie the magic
};
struct Result {               // 64 bytes = ohgpu_ogg_stream_result
    uint32_t status, pages, pages_ignored, packets;
    uint64_t bytes_delivered, bytes_consumed;
    uint32_t resume_segment, next_seq;
    int64_t  last_granule;
    uint32_t serial;
    uint8_t  bos_seen, eos_seen, reserved[2];
    uint32_t links, reserved2;
};
struct Packet {               // 40 bytes = ohgpu_ogg_packet
    uint64_t run_pos;         // of its first delivered byte, from the stream's dst_offset
    uint32_t bytes, flags;
    int64_t  granule;
    uint64_t page_offset;     // where it began: the page (from src_offset), that page's number, the segment
    uint32_t page_seq, segment;
};
struct Candidate { uint32_t stream, pos, bytes, reserved; };
struct Piece { uint32_t stream, src_pos, run_pos, bytes; };           // bytes [src_pos, + bytes) of the stream's range -> [run_pos, + bytes) of its run
struct Tables { uint32_t byte[256], shift[256], shift256[256]; };    // i * x^32, x^(8 j), x^(2048 j), all mod P
static_assert(sizeof(Stream) == 64 && sizeof(Result) == 64 && sizeof(Packet) == 40 && sizeof(Candidate) == 16 && sizeof(Piece) == 16, "Ogg layouts");

// ---- the checksum.  A register holds a polynomial of degree < 32, bit k the coefficient of x^k.
OGGP_HD uint32_t times_x(uint32_t v) { return (v << 1) ^ ((v >> 31) ? kPoly : 0u); }
OGGP_HD uint32_t times_x8(const uint32_t* byte_table, uint32_t v) { return (v << 8) ^ byte_table[v >> 24]; }
OGGP_HD uint32_t mul(uint32_t a, uint32_t b)                         // a * b mod P, Horner over b's bits from the top
{
    uint32_t r = 0;
    for (int k = 0; k < 32; k++) {
        r = times_x(r) ^ ((b >> 31) ? a : 0u);
        b <<= 1;
    }
    return r;
}
inline void make_tables(Tables* t)
{
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t r = i << 24;
        for (int k = 0; k < 8; k++) r = times_x(r);
        t->byte[i] = r;
    }
    t->shift[0] = 1;
    for (uint32_t j = 1; j < 256; j++) t->shift[j] = times_x8(t->byte, t->shift[j - 1]);
    const uint32_t x2048 = times_x8(t->byte, t->shift[255]);
    t->shift256[0] = 1;
    for (uint32_t j = 1; j < 256; j++) t->shift256[j] = mul(t->shift256[j - 1], x2048);
}
OGGP_HD uint32_t ld32u(const uint8_t* p)                              // four bytes at any address, as they lie
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
OGGP_HD uint32_t crc_byte(const uint32_t* byte_table, uint32_t crc, uint32_t b) { return (crc << 8) ^ byte_table[(crc >> 24) ^ b]; }
// Bytes [from, to) of a page through the byte table, the checksum field read as zero.  No byte outside [from, to) is read.
OGGP_HD uint32_t crc_run(const uint32_t* byte_table, const uint8_t* page, uint32_t from, uint32_t to)
{
    uint32_t crc = 0, j = from;
    for (; j + 4u <= to; j += 4u) {
        if (j + 4u > 22u && j < 26u) {                                // the dword touches the field: its bytes one by one
            for (uint32_t k = j; k < j + 4u; k++) crc = crc_byte(byte_table, crc, k - 22u < 4u ? 0u : page[k]);
            continue;
        }
        const uint32_t w = ld32u(page + j);
        crc = crc_byte(byte_table, crc, w & 0xffu);
        crc = crc_byte(byte_table, crc, (w >> 8) & 0xffu);
        crc = crc_byte(byte_table, crc, (w >> 16) & 0xffu);
        crc = crc_byte(byte_table, crc, w >> 24);
    }
    for (; j < to; j++) crc = crc_byte(byte_table, crc, j - 22u < 4u ? 0u : page[j]);
    return crc;
}
OGGP_HD uint32_t slice_bytes(uint32_t page_bytes)
{
    const uint32_t even = (page_bytes + kLanes - 1u) / kLanes;
    return even < kSliceMin ? kSliceMin : even;
}
// Lane `lane`'s term of the page's checksum: its slice's register times x^(8 * the bytes behind the slice).  The xor over the kLanes
// lanes is the page's checksum.
OGGP_HD uint32_t crc_lane(const uint32_t* byte_table, const uint32_t* shift, const uint32_t* shift256, const uint8_t* page, uint32_t page_bytes, uint32_t lane)
{
    const uint32_t slice = slice_bytes(page_bytes), from = lane * slice;
    if (from >= page_bytes) return 0;
    const uint32_t to = from + slice < page_bytes ? from + slice : page_bytes, behind = page_bytes - to;
    uint32_t c = crc_run(byte_table, page, from, to);
    if (behind & 255u) c = mul(c, shift[behind & 255u]);
    if (behind >> 8) c = mul(c, shift256[behind >> 8]);
    return c;
}
OGGP_HD uint32_t stored_crc(const uint8_t* page) { return page[22] | ((uint32_t)page[23] << 8) | ((uint32_t)page[24] << 16) | ((uint32_t)page[25] << 24); }
inline uint32_t crc_bytes(const Tables& t, const uint8_t* bytes, uint64_t n)      // of any bytes, nothing read as zero (ohgpu_ogg_crc)
{
    uint32_t crc = 0;
    for (uint64_t j = 0; j < n; j++) crc = crc_byte(t.byte, crc, bytes[j]);
    return crc;
}

// ---- the page.  `avail` bytes are readable from p.  1: a whole page image, *out filled; 0: the range ends inside it (fewer than 27
// bytes, than the header, than the page); -1: 27 bytes or more and no capture pattern.
struct Page {
    uint32_t bytes, header_bytes, segments, flags, version, serial, seq;
    int64_t  granule;
};
OGGP_HD uint32_t le32(const uint8_t* p) { return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
OGGP_HD int parse_page(const uint8_t* p, uint32_t avail, Page* out)
{
    if (avail < (uint32_t)kHeaderBytes) return 0;
    if (p[0] != 'O' || p[1] != 'g' || p[2] != 'g' || p[3] != 'S') return -1;
    const uint32_t n = p[26];
    if (avail < kHeaderBytes + n) return 0;
    uint32_t body = 0;
    for (uint32_t k = 0; k < n; k++) body += p[kHeaderBytes + k];
    if (avail < kHeaderBytes + n + body) return 0;
    out->bytes = kHeaderBytes + n + body;
    out->header_bytes = kHeaderBytes + n;
    out->segments = n;
    out->version = p[4];
    out->flags = p[5];
    out->granule = (int64_t)((uint64_t)le32(p + 6) | ((uint64_t)le32(p + 10) << 32));
    out->serial = le32(p + 14);
    out->seq = le32(p + 18);
    return 1;
}

// The verdict on the whole page image at `pos` of a stream: the bit the verify phase set.  When the find phase met more candidates
// than its list holds (`overflowed`: "OggS" strings a few bytes apart, which no stream of pages has), a clear bit may be a page nobody
// verified, and the walk runs the checksum itself.
OGGP_HD bool page_good(const uint32_t* bits, uint64_t bit_base, uint32_t pos, bool overflowed, const Tables* t, const uint8_t* page, uint32_t bytes)
{
    const uint64_t b = bit_base + pos;
    if ((bits[b >> 5] >> (b & 31u)) & 1u) return true;
    return overflowed && crc_run(t->byte, page, 0, bytes) == stored_crc(page);
}

// The link magic: `len` bytes, byte k the k-th byte in memory of the two words (lo first)
OGGP_HD bool begins_with(const uint8_t* body, uint32_t body_bytes, uint32_t len, uint32_t lo, uint32_t hi)
{
    if (body_bytes < len) return false;
    for (uint32_t k = 0; k < len; k++)
        if (body[k] != (((k < 4u ? lo >> (8u * k) : hi >> (8u * (k - 4u)))) & 0xffu)) return false;
    return true;
}

// ---- the walk over one stream.
struct Walker {
    const uint8_t* base;      // the stream's first byte
    Packet*  packets;         // the stream's part of the packet table
    Piece*   pieces;          // ... and of the gather plan, piece_cap records
    uint32_t stream_index, packet_cap, piece_cap, flags;
    uint32_t n_packets, n_pieces, delivered;
    uint32_t cur_src, cur_run, cur_len;                               // the piece being made
    bool     open;                                                    // a packet has begun and not ended
    bool     link_pending;                                            // a link began and none of its packets has
    uint32_t pk_page, pk_seq, pk_seg, pk_run, pk_bytes, pk_flags, pk_verdict, pk_piece, pk_cut;

    OGGP_HD void flush()
    {
        if (cur_len && n_pieces < piece_cap) {
            Piece& g = pieces[n_pieces++];
            g.stream = stream_index; g.src_pos = cur_src; g.run_pos = cur_run; g.bytes = cur_len;
        }
        cur_len = 0;
    }
    // the packet that is open is not delivered: the plan and the run end where it began
    OGGP_HD void truncate()
    {
        delivered = pk_run;
        if (n_pieces > pk_piece) {                                    // the piece it began in is written already
            if (pk_cut) { pieces[pk_piece].bytes = pk_cut; n_pieces = pk_piece + 1u; }
            else n_pieces = pk_piece;
            cur_len = 0;
        } else cur_len = pk_cut;
        flush();
        open = false;
    }
    // segment `seg` of the page at `page_pos`, `v` bytes at `at` (both from the stream's start); true: the packet it ends has a
    // mapping header that the stream must stop for (pk_verdict)
    OGGP_HD bool segment(uint32_t page_pos, uint32_t page_seq, uint32_t seg, uint32_t v, uint32_t at, bool first_of_bos_page, bool last_of_eos_page, uint32_t* completed)
    {
        uint32_t skip = 0;
        if (!open) {
            open = true;
            pk_page = page_pos; pk_seq = page_seq; pk_seg = seg; pk_run = delivered; pk_bytes = 0;
            pk_flags = (first_of_bos_page ? (uint32_t)kPacketBos : 0u) | (link_pending ? (uint32_t)kPacketLink : 0u);
            link_pending = false;
            pk_verdict = kOk;
            if ((flags & kFlacMapping) && v > 0 && base[at] == 0x7f) {
                const uint8_t* h = base + at;
                if (v < (uint32_t)kMappingHeaderBytes || h[1] != 'F' || h[2] != 'L' || h[3] != 'A' || h[4] != 'C') pk_verdict = kNotFlac;
                else if (h[5] != 1) pk_verdict = kUnsupportedMapping;
                else { skip = kMappingHeaderBytes; pk_flags |= kPacketMappingHeader; flush(); }
            }
            pk_piece = n_pieces; pk_cut = cur_len;
        }
        const uint32_t take = v - skip;
        if (take) {
            if (!cur_len) { cur_src = at + skip; cur_run = delivered; }
            cur_len += take; delivered += take; pk_bytes += take;
        }
        if (last_of_eos_page) pk_flags |= kPacketEos;
        if (v == 255u) return false;
        if (pk_verdict != kOk) return true;
        if (n_packets < packet_cap) {
            Packet& k = packets[n_packets];
            k.run_pos = pk_run; k.bytes = pk_bytes; k.flags = pk_flags; k.granule = -1;
            k.page_offset = pk_page; k.page_seq = pk_seq; k.segment = pk_seg;
        }
        *completed = n_packets++;
        open = false;
        return false;
    }
};

// One stream.  `good(pos, page, bytes)`: the checksum of the whole page image at `pos` holds.  `pieces` has room for piece_capacity(s)
// records; *n_pieces of them are the plan.
OGGP_HD uint32_t piece_capacity(const Stream& s)
{
    // 27 bytes a page and 10 a mapping header (its nine bytes and a lacing value): a page gives a piece and every header one more
    return s.src_bytes / 27u + 1u + ((s.flags & kFlacMapping) ? s.src_bytes / 10u + 1u : 0u);
}
// Links = false is the walk without rules L1 ... L5 in its text: what a batch none of whose streams has kFollowLinks runs.
template <bool Links = true, typename Good>
OGGP_HD void walk(const Stream& s, uint32_t stream_index, const uint8_t* src, Packet* packet_table, Piece* pieces, Good& good, Result* out, uint32_t* n_pieces)
{
    Walker w;
    w.base = src + s.src_offset;
    w.packets = packet_table + s.packet_first;
    w.pieces = pieces;
    w.stream_index = stream_index; w.packet_cap = s.packet_capacity; w.piece_cap = piece_capacity(s); w.flags = s.flags;
    w.n_packets = w.n_pieces = w.delivered = 0;
    w.cur_src = w.cur_run = w.cur_len = 0;
    w.open = w.link_pending = false;
    w.pk_page = w.pk_seq = w.pk_seg = w.pk_run = w.pk_bytes = w.pk_flags = w.pk_verdict = w.pk_piece = w.pk_cut = 0;

    uint32_t p = 0, status = kOk, serial = s.serial, expect = s.expect_seq, pages = 0, ignored = 0;
    bool serial_known = !(s.flags & kAnySerial), seq_known = !(s.flags & kAnySeq), first = true;
    uint8_t bos_seen = 0, eos_seen = 0;
    int64_t last_granule = -1;
    // the links (rules L1 ... L5): how many, and whether the followed serial's last accepted page had the "first page" flag.  What
    // the result was in front of the last link is kept in *out, where nothing else is written before the end: a link is rare, and
    // the walk without one should not carry that in registers.
    const bool follow = Links && (s.flags & kFollowLinks) != 0;
    uint32_t links = 0;
    bool last_bos = false;
    for (;;) {
        Page pg;
        const uint8_t* page = w.base + p;
        const int whole = parse_page(page, s.src_bytes - p, &pg);
        if (whole == 0) break;
        if (whole < 0 || !good(p, page, pg.bytes)) { status = kLostSync; break; }
        if (!serial_known) { serial = pg.serial; serial_known = true; }
        if (pg.serial != serial || pg.version != 0) {
            const bool link = follow && pg.version == 0 && pg.serial != serial && (pg.flags & kPageBos) && !last_bos &&
                              begins_with(page + pg.header_bytes, pg.bytes - pg.header_bytes, s.reserved[0], s.reserved[1], s.reserved[2]);
            if (!link) { ignored++; p += pg.bytes; continue; }
            if (w.open) w.truncate();                                 // L2: the packet still open is dropped
            out->bytes_consumed = p; out->serial = serial; out->next_seq = expect; out->pages = pages; out->pages_ignored = ignored;
            out->packets = w.n_packets; out->bos_seen = bos_seen; out->eos_seen = eos_seen;
            serial = pg.serial; seq_known = false; first = false;
            links++;
            w.link_pending = true;
        }
        if (seq_known && pg.seq != expect) { status = kHole; break; }
        const uint8_t* lace = page + kHeaderBytes;
        uint32_t seg = 0, at = p + pg.header_bytes;
        bool bos = (pg.flags & kPageBos) != 0;
        if (first && s.first_page_segment) {
            if (s.first_page_segment > pg.segments) { status = kBadResume; break; }
            for (; seg < s.first_page_segment; seg++) at += lace[seg];
            bos = false;
        } else if ((pg.flags & kPageContinued) && !w.open) {          // the end of a packet whose beginning was never seen
            bos = false;
            while (seg < pg.segments) {
                const uint32_t v = lace[seg++];
                at += v;
                if (v < 255u) break;
            }
        }
        first = false; seq_known = true; expect = pg.seq + 1u; pages++;
        last_bos = (pg.flags & kPageBos) != 0;
        if (pg.flags & kPageBos) bos_seen = 1;
        if (pg.flags & kPageEos) eos_seen = 1;
        const bool eos = (pg.flags & kPageEos) != 0;
        if (eos && pg.segments == 0 && w.open) w.pk_flags |= kPacketEos;
        uint32_t last_completed = ~0u;
        bool stop = false;
        for (; seg < pg.segments && !stop; seg++) {
            const uint32_t v = lace[seg];
            stop = w.segment(p, pg.seq, seg, v, at, bos && seg == 0, eos && seg + 1u == pg.segments, &last_completed);
            at += v;
        }
        if (stop) { status = w.pk_verdict; break; }
        if (last_completed != ~0u) {                                  // the page's granule position is its last completed packet's
            if (last_completed < w.packet_cap) w.packets[last_completed].granule = pg.granule;
            if (pg.granule != -1) last_granule = pg.granule;
        }
        w.flush();
        p += pg.bytes;
    }
    uint32_t consumed = p, resume = 0, next_seq = expect;
    if (w.open) {
        if (status == kOk) { consumed = w.pk_page; resume = w.pk_seg; next_seq = w.pk_seq; }
        w.truncate();
    }
    if (links && status == kOk && w.n_packets == out->packets) {      // L4: the last link is the next call's to find
        consumed = (uint32_t)out->bytes_consumed; resume = 0; next_seq = out->next_seq;
        serial = out->serial; pages = out->pages; ignored = out->pages_ignored;
        bos_seen = out->bos_seen; eos_seen = out->eos_seen;
        links--;
    }
    w.flush();
    out->status = status; out->pages = pages; out->pages_ignored = ignored; out->packets = w.n_packets;
    out->bytes_delivered = w.delivered; out->bytes_consumed = consumed;
    out->resume_segment = resume; out->next_seq = next_seq;
    out->last_granule = last_granule;
    out->serial = serial;
    out->bos_seen = bos_seen; out->eos_seen = eos_seen; out->reserved[0] = out->reserved[1] = 0;
    out->links = links; out->reserved2 = 0;
    *n_pieces = w.n_pieces;
}

}  // namespace oggpage
