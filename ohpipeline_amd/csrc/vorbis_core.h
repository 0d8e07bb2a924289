// vorbis_core.h -- Vorbis I, written from the specification's behaviour (the rules V1-V6 are include/ohgpu_vorbis.h's).
// The setup parse is host text; everything a packet needs is __host__ __device__: csrc/vorbis_kernel.hip runs it on the device,
// tests/cpp/vorbis_core_driver.cpp runs the same text on the CPU under the sanitizers.
//
// Reading of the format:
//   bits       least significant bit of each byte first; a read past the packet's end sets `eop`, which sticks, and gives 0
//   codebook   codewords are assigned from the lengths in entry order, each entry taking the lowest-valued free codeword of its
//              length (first bit most significant); the setup image holds the binary tree (a node is two int32: >= 0 a node, -1
//              nothing there, <= -2 the leaf of entry -(v + 2)) and, for lookup types 1 and 2, every entry's value vector in float32
//   floor 1    a nonzero bit, two amplitudes of ilog(range - 1) bits, per partition a master codeword and the class's subclass books;
//              the amplitudes are unwrapped against the line between their neighbours (all integer); the curve is drawn by the
//              integer line rule and indexes the dB table
//   residue    classification codewords in pass 0, then per pass and partition the class's book of that pass adds value vectors:
//              type 0 strided, type 1 in order, type 2 in order over the interleaved channels of the submap
//   coupling   magnitude / angle pairs, undone from the last step to the first
// Where the specification leaves a choice (DESIGN.md 5.23 lists them): the end of the packet anywhere in a floor leaves that floor
// unused (Tremor's reading); a codeword the tree does not hold counts as the end of the packet; a type 1 / 2 partition whose size is no
// multiple of the book's dimension drops the last vector's overhang; the curve's end points are clamped to the dB table.
//
// Every loop is bounded by the setup's counts or the block size, every load by the packet's bytes, every row store by the block size.
#pragma once

#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define VB_HD __host__ __device__ inline
#else
#define VB_HD inline
#endif

namespace vorbiscore {

enum { kOk = 0, kHeader = 1, kCorrupt = 2 };                              // OHGPU_VORBIS_*
enum { kOutPlanar32 = 1 };
enum { kMaxChannels = 8, kMaxFloorValues = 65, kMaxCoupling = 32 };
enum { kParseOk = 0, kParseInvalid = -1, kParseUnsupported = -6 };        // OHGPU_ERR_*
constexpr uint32_t kMagic = 0x31425256u;                                   // "VRB1"
constexpr uint32_t kMaxImageBytes = 16u << 20, kMaxClassBytes = 1u << 20;

struct Image {                   // the image's first 32 words; every off_* counts 32-bit words from the image's start
    uint32_t magic, words, channels, rate, bs0, bs1;
    uint32_t n_books, n_floors, n_residues, n_mappings, n_modes, mode_bits;
    uint32_t off_books, off_floors, off_residues, off_mappings, off_modes;
    uint32_t class_bytes;        // what a packet's residue classifications take at most
    uint32_t reserved[14];
};
struct Book { uint32_t entries, dim, lookup, off_tree, n_nodes, off_values, used, reserved; };
struct Floor {
    uint32_t partitions, multiplier, rangebits, values;
    uint8_t  part_class[32];
    uint8_t  class_dim[16], class_sub[16];
    int16_t  class_master[16];
    int16_t  sub_book[16][8];    // -1: none
    uint16_t x[66];
    uint8_t  sorted[66], low[66], high[66];   // the values' order by x; each value's neighbours among those in front of it
    uint8_t  pad[2];
};
struct Residue {
    uint32_t type, begin, end, psize, classifications, classbook;
    uint8_t  cascade[64];
    int16_t  books[64][8];       // -1: none
};
struct Mapping {
    uint32_t submaps, steps;
    uint8_t  mag[kMaxCoupling], ang[kMaxCoupling];
    uint8_t  mux[kMaxChannels];
    uint8_t  sub_floor[16], sub_residue[16];
};
struct Mode { uint32_t blockflag, mapping; };
static_assert(sizeof(Image) == 128 && sizeof(Book) == 32 && sizeof(Floor) % 4 == 0 && sizeof(Residue) % 4 == 0 && sizeof(Mapping) % 4 == 0, "image records are whole words");

struct Stream {                  // a descriptor as the device sees it: 88 bytes
    uint64_t dst_offset, dst_plane_stride, max_samples;
    uint64_t image_word;         // where its image begins in the batch's blob, in words
    uint64_t row_base, block_base, class_base;   // its first spectrum row (floats), block (floats), classification byte
    uint32_t first_packet, n_packets;
    uint32_t flags, channels, bs0, bs1, class_bytes, reserved;
};
struct Packet { uint64_t src_offset; uint32_t bytes, stream, index, reserved; };   // 24 bytes
struct Rec {                     // 24 bytes: ohgpu_vorbis_packet_result, whose reserved word holds what the later phases need
    uint8_t  status, mode;
    uint16_t blocksize;
    uint32_t samples;
    uint64_t position;
    uint16_t prev_block;         // the block of the OK packet in front of it, 0 for the one that primes
    uint8_t  prev_flag, next_flag;
    uint32_t prev_packet;        // that packet's place in the stream
};
struct FloorOut {                // one channel's floor of one packet: 148 bytes
    uint32_t used;
    uint32_t flags[3];           // bit i: value i takes part in the curve
    int16_t  y[66];
};
static_assert(sizeof(Stream) == 88 && sizeof(Packet) == 24 && sizeof(Rec) == 24 && sizeof(FloorOut) == 148, "Vorbis device layouts");

VB_HD uint32_t ilog(uint32_t v) { uint32_t n = 0; while (v) { n++; v >>= 1; } return n; }

struct Bits { const uint8_t* p; uint64_t bits; uint64_t pos; bool eop; };
VB_HD Bits bits_open(const uint8_t* p, uint32_t bytes) { return Bits{p, (uint64_t)bytes * 8u, 0, false}; }
VB_HD uint32_t get(Bits& b, uint32_t n)              // n <= 32
{
    if (n == 0) return 0;
    if (b.eop || b.pos + n > b.bits) { b.eop = true; return 0; }
    uint64_t v = 0, pos = b.pos;
    uint32_t got = 0;
    while (got < n) {
        const uint32_t off = (uint32_t)(pos & 7u), room = 8u - off;
        const uint32_t take = room < n - got ? room : n - got;
        v |= (uint64_t)((b.p[pos >> 3] >> off) & ((1u << take) - 1u)) << got;
        got += take; pos += take;
    }
    b.pos = pos;
    return (uint32_t)v;
}

VB_HD const Image& image_head(const uint32_t* img) { return *(const Image*)img; }
VB_HD const Book& image_book(const uint32_t* img, uint32_t i) { return *(const Book*)(img + image_head(img).off_books + i * (sizeof(Book) / 4)); }
VB_HD const Floor& image_floor(const uint32_t* img, uint32_t i) { return *(const Floor*)(img + image_head(img).off_floors + i * (sizeof(Floor) / 4)); }
VB_HD const Residue& image_residue(const uint32_t* img, uint32_t i) { return *(const Residue*)(img + image_head(img).off_residues + i * (sizeof(Residue) / 4)); }
VB_HD const Mapping& image_mapping(const uint32_t* img, uint32_t i) { return *(const Mapping*)(img + image_head(img).off_mappings + i * (sizeof(Mapping) / 4)); }
VB_HD const Mode& image_mode(const uint32_t* img, uint32_t i) { return *(const Mode*)(img + image_head(img).off_modes + i * (sizeof(Mode) / 4)); }

// One codeword: the entry, or -1 at the end of the packet or where the tree holds nothing (which then counts as the end).
VB_HD int32_t book_decode(const uint32_t* img, const Book& bk, Bits& b)
{
    const int32_t* tree = (const int32_t*)(img + bk.off_tree);
    int32_t node = 0;
    for (uint32_t depth = 0; depth < 33; depth++) {
        const uint32_t bit = get(b, 1);
        if (b.eop) return -1;
        const int32_t c = tree[node * 2 + (int32_t)bit];
        if (c <= -2) return -(c + 2);
        if (c == -1) break;
        node = c;
    }
    b.eop = true;
    return -1;
}

// ---- phase 1: what a packet's first bits say
VB_HD void head_packet(const uint32_t* img, const uint8_t* p, uint32_t bytes, Rec* r)
{
    const Image& im = image_head(img);
    Rec o;
    o.status = kCorrupt; o.mode = 0; o.blocksize = 0; o.samples = 0; o.position = 0; o.prev_block = 0; o.prev_flag = 0; o.next_flag = 0; o.prev_packet = 0;
    Bits b = bits_open(p, bytes);
    const uint32_t type = get(b, 1);
    if (!b.eop && type == 1) o.status = kHeader;
    else if (!b.eop) {
        const uint32_t mode = get(b, im.mode_bits);
        if (!b.eop && mode < im.n_modes) {
            const Mode& m = image_mode(img, mode);
            uint32_t pf = 0, nf = 0;
            if (m.blockflag) { pf = get(b, 1); nf = get(b, 1); }
            if (!b.eop) {
                o.status = kOk; o.mode = (uint8_t)mode; o.blocksize = (uint16_t)(m.blockflag ? im.bs1 : im.bs0);
                o.prev_flag = (uint8_t)pf; o.next_flag = (uint8_t)nf;
            }
        }
    }
    *r = o;
}

// ... and a stream's positions from its packets' blocks (V3, V4)
VB_HD void scan_stream(const Stream& s, Rec* recs)
{
    uint64_t pos = 0;
    uint32_t prev = 0, prev_k = 0;
    for (uint32_t k = 0; k < s.n_packets; k++) {
        Rec& r = recs[k];
        r.position = pos;
        if (r.status != kOk) continue;
        if (prev) {
            const uint32_t d = prev / 4u + r.blocksize / 4u;
            const uint64_t room = pos < s.max_samples ? s.max_samples - pos : 0u;
            r.samples = (uint32_t)(room < d ? room : d);
            pos += d;
        }
        r.prev_block = (uint16_t)prev; r.prev_packet = prev_k;
        prev = r.blocksize; prev_k = k;
    }
}

// ---- phase 2: floor values, residue, inverse coupling
VB_HD int32_t render_point(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t x)
{
    const int32_t dy = y1 - y0, adx = x1 - x0, ady = dy < 0 ? -dy : dy;
    const int32_t off = ady * (x - x0) / adx;
    return dy < 0 ? y0 - off : y0 + off;
}

VB_HD void floor1_decode(const uint32_t* img, const Floor& f, Bits& b, FloorOut* out)
{
    out->used = 0; out->flags[0] = out->flags[1] = out->flags[2] = 0;
    if (!get(b, 1)) return;
    int32_t Y[66], fin[66];
    const int32_t range = f.multiplier == 1 ? 256 : f.multiplier == 2 ? 128 : f.multiplier == 3 ? 86 : 64;
    const uint32_t abits = ilog((uint32_t)range - 1u);
    Y[0] = (int32_t)get(b, abits); Y[1] = (int32_t)get(b, abits);
    uint32_t off = 2;
    for (uint32_t i = 0; i < f.partitions; i++) {
        const uint32_t c = f.part_class[i], cdim = f.class_dim[c], cbits = f.class_sub[c], csub = (1u << cbits) - 1u;
        uint32_t cval = 0;
        if (cbits) { const int32_t e = book_decode(img, image_book(img, (uint32_t)f.class_master[c]), b); cval = e < 0 ? 0u : (uint32_t)e; }
        for (uint32_t j = 0; j < cdim; j++) {
            const int32_t book = f.sub_book[c][cval & csub];
            cval >>= cbits;
            int32_t v = 0;
            if (book >= 0) { v = book_decode(img, image_book(img, (uint32_t)book), b); if (v < 0) v = 0; }
            Y[off + j] = v;
        }
        off += cdim;
    }
    if (b.eop) return;
    uint32_t flags[3] = {3u, 0u, 0u};
    fin[0] = Y[0]; fin[1] = Y[1];
    for (uint32_t i = 2; i < f.values; i++) {
        const uint32_t lo = f.low[i], hi = f.high[i];
        const int32_t predicted = render_point(f.x[lo], fin[lo], f.x[hi], fin[hi], f.x[i]);
        const int32_t val = Y[i], highroom = range - predicted, lowroom = predicted;
        const int32_t room = (highroom < lowroom ? highroom : lowroom) * 2;
        if (val) {
            flags[lo >> 5] |= 1u << (lo & 31u); flags[hi >> 5] |= 1u << (hi & 31u); flags[i >> 5] |= 1u << (i & 31u);
            if (val >= room) fin[i] = highroom > lowroom ? val - lowroom + predicted : predicted - val + highroom - 1;
            else fin[i] = (val & 1) ? predicted - (val + 1) / 2 : predicted + val / 2;
        } else fin[i] = predicted;
    }
    for (uint32_t i = 0; i < f.values; i++) out->y[i] = (int16_t)fin[i];
    out->flags[0] = flags[0]; out->flags[1] = flags[1]; out->flags[2] = flags[2];
    out->used = 1;
}

// The rows of one packet: channel c's value i is rows[c * stride + i].
struct Rows { float* rows; uint32_t stride; };

VB_HD void residue_decode(const uint32_t* img, const Residue& r, Bits& b, uint32_t half, uint32_t nvec, const uint8_t* chan, const bool* dnd, const Rows& rows, uint8_t* cls)
{
    const bool two = r.type == 2;
    if (two) {
        bool all = true;
        for (uint32_t j = 0; j < nvec; j++) all = all && dnd[j];
        if (all) return;
    }
    const uint32_t vecs = two ? 1u : nvec, actual = two ? half * nvec : half;
    const uint32_t lb = r.begin < actual ? r.begin : actual, le = r.end < actual ? r.end : actual;
    if (le <= lb) return;
    const Book& cb = image_book(img, r.classbook);
    const uint32_t cw = cb.dim, parts = (le - lb) / r.psize, stride = parts + cw;
    if (!parts) return;
    const auto add = [&](uint32_t j, uint32_t idx, float v) {
        float* q = two ? rows.rows + (uint64_t)chan[idx % nvec] * rows.stride + idx / nvec : rows.rows + (uint64_t)chan[j] * rows.stride + idx;
        *q = *q + v;
    };
    for (uint32_t pass = 0; pass < 8; pass++) {
        uint32_t pc = 0;
        while (pc < parts) {
            if (pass == 0)
                for (uint32_t j = 0; j < vecs; j++) {
                    if (!two && dnd[j]) continue;
                    const int32_t e = book_decode(img, cb, b);
                    if (e < 0) return;
                    uint32_t temp = (uint32_t)e;
                    for (uint32_t i = cw; i-- > 0;) { cls[j * stride + pc + i] = (uint8_t)(temp % r.classifications); temp /= r.classifications; }
                }
            for (uint32_t i = 0; i < cw && pc < parts; i++, pc++)
                for (uint32_t j = 0; j < vecs; j++) {
                    if (!two && dnd[j]) continue;
                    const uint32_t vqclass = cls[j * stride + pc];
                    const int32_t vqbook = r.books[vqclass][pass];
                    if (!((r.cascade[vqclass] >> pass) & 1u) || vqbook < 0) continue;
                    const Book& vb = image_book(img, (uint32_t)vqbook);
                    const float* values = (const float*)(img + vb.off_values);
                    const uint32_t offset = lb + pc * r.psize;
                    if (r.type == 0) {
                        const uint32_t step = r.psize / vb.dim;
                        for (uint32_t k = 0; k < step; k++) {
                            const int32_t e = book_decode(img, vb, b);
                            if (e < 0) return;
                            for (uint32_t d = 0; d < vb.dim; d++) add(j, offset + k + d * step, values[(uint64_t)e * vb.dim + d]);
                        }
                    } else {
                        for (uint32_t k = 0; k < r.psize;) {
                            const int32_t e = book_decode(img, vb, b);
                            if (e < 0) return;
                            for (uint32_t d = 0; d < vb.dim && k < r.psize; d++, k++) add(j, offset + k, values[(uint64_t)e * vb.dim + d]);
                        }
                    }
                }
        }
    }
}

// One OK packet: its channels' floors to `floors`, its residue, uncoupled, to the rows (which come zeroed).  `cls`: class_bytes of work space.
VB_HD void decode_packet(const uint32_t* img, const uint8_t* p, uint32_t bytes, const Rec& rec, const Rows& rows, FloorOut* floors, uint8_t* cls)
{
    const Image& im = image_head(img);
    const Mode& mode = image_mode(img, rec.mode);
    const Mapping& map = image_mapping(img, mode.mapping);
    const uint32_t half = rec.blocksize / 2u, ch = im.channels;
    Bits b = bits_open(p, bytes);
    (void)get(b, 1); (void)get(b, im.mode_bits);
    if (mode.blockflag) (void)get(b, 2);
    bool nonzero[kMaxChannels];
    for (uint32_t c = 0; c < ch; c++) {
        floor1_decode(img, image_floor(img, map.sub_floor[map.mux[c]]), b, &floors[c]);
        nonzero[c] = floors[c].used != 0;
    }
    for (uint32_t s = 0; s < map.steps; s++)
        if (nonzero[map.mag[s]] || nonzero[map.ang[s]]) nonzero[map.mag[s]] = nonzero[map.ang[s]] = true;
    for (uint32_t sm = 0; sm < map.submaps; sm++) {
        uint8_t chan[kMaxChannels];
        bool dnd[kMaxChannels];
        uint32_t nvec = 0;
        for (uint32_t c = 0; c < ch; c++)
            if (map.mux[c] == sm) { chan[nvec] = (uint8_t)c; dnd[nvec] = !nonzero[c]; nvec++; }
        if (nvec) residue_decode(img, image_residue(img, map.sub_residue[sm]), b, half, nvec, chan, dnd, rows, cls);
    }
    for (uint32_t s = map.steps; s-- > 0;) {
        float* M = rows.rows + (uint64_t)map.mag[s] * rows.stride;
        float* A = rows.rows + (uint64_t)map.ang[s] * rows.stride;
        for (uint32_t i = 0; i < half; i++) {
            const float m = M[i], a = A[i];
            float nm, na;
            if (m > 0) { if (a > 0) { nm = m; na = m - a; } else { na = m; nm = m + a; } }
            else       { if (a > 0) { nm = m; na = m + a; } else { na = m; nm = m - a; } }
            M[i] = nm; A[i] = na;
        }
    }
}

// ---- phase 3's integer half: the curve's segments, and one segment drawn
struct Segment { int32_t x0, y0, x1, y1; };
// Up to 64 segments, then the level that holds from the last point on: returns their number; *tail_x, *tail_y the last point.
VB_HD uint32_t floor_segments(const Floor& f, const FloorOut& fo, Segment* segs, int32_t* tail_x, int32_t* tail_y)
{
    const auto level = [&](uint32_t j) { const int32_t v = fo.y[j] * (int32_t)f.multiplier; return v < 0 ? 0 : v > 255 ? 255 : v; };
    uint32_t n = 0;
    int32_t lx = 0, ly = level(f.sorted[0]);
    for (uint32_t i = 1; i < f.values; i++) {
        const uint32_t j = f.sorted[i];
        if (!((fo.flags[j >> 5] >> (j & 31u)) & 1u)) continue;
        const int32_t hx = f.x[j], hy = level(j);
        segs[n++] = Segment{lx, ly, hx, hy};
        lx = hx; ly = hy;
    }
    *tail_x = lx; *tail_y = ly;
    return n;
}
// put(x, y) for x0 <= x < min(x1, limit): the specification's render_line
template <typename Put>
VB_HD void draw_segment(const Segment& s, int32_t limit, Put&& put)
{
    const int32_t dy = s.y1 - s.y0, adx = s.x1 - s.x0;
    const int32_t base = dy / adx, sy = dy < 0 ? base - 1 : base + 1;
    const int32_t ady = (dy < 0 ? -dy : dy) - (base < 0 ? -base : base) * adx;
    int32_t y = s.y0, err = 0;
    const int32_t end = s.x1 < limit ? s.x1 : limit;
    if (s.x0 < end) put(s.x0, y);
    for (int32_t x = s.x0 + 1; x < end; x++) {
        err += ady;
        if (err >= adx) { err -= adx; y += sy; } else y += base;
        put(x, y);
    }
}

// The window's value at i of a block of n (V3's overlap relies on it being 0 and 1 outside the slopes): slope_n and slope_0 are the
// rising halves for this block's size and for the short size.
VB_HD float window_at(uint32_t i, uint32_t n, uint32_t bs0, bool is_long, bool prev_flag, bool next_flag, const float* slope_n, const float* slope_0)
{
    const bool right = i >= n / 2u;
    const uint32_t k = right ? n - 1u - i : i;
    const bool full = !is_long || (right ? next_flag : prev_flag);
    if (full) return slope_n[k];
    const uint32_t start = n / 4u - bs0 / 4u;
    if (k < start) return 0.0f;
    if (k < start + bs0 / 2u) return slope_0[k - start];
    return 1.0f;
}

// ---- phases 3 and 4 as serial text (the device's plain route is this sum; csrc/vorbis_kernel.hip has the FFT): the DCT-IV by its
// definition over a cosine table of 8N points (cos8[j] = cos(2 pi j / 8N)), accumulated in double; the unfolding of its N values into
// the block's n = 2N by the cosine's symmetries; and one output sample from the previous block's second half and this block's first.
VB_HD float dct4_direct(const float* spec, uint32_t N, const float* cos8, uint32_t i)
{
    double acc = 0.0;
    const uint32_t oi = 2u * i + 1u, mask = 8u * N - 1u;
    for (uint32_t k = 0; k < N; k++) acc += (double)spec[k] * (double)cos8[(oi * (2u * k + 1u)) & mask];
    return (float)acc;
}
VB_HD float unfold_at(const float* u, uint32_t N, uint32_t i)
{
    return i < N / 2u ? u[i + N / 2u] : i < 3u * N / 2u ? -u[3u * N / 2u - 1u - i] : -u[i - 3u * N / 2u];
}
// sample j of what a packet delivers: prev is the previous OK packet's windowed block of pn, cur this packet's of n (one channel each)
VB_HD float overlap_at(const float* prev, uint32_t pn, const float* cur, uint32_t n, uint32_t j)
{
    const int32_t ci = (int32_t)j + (int32_t)(n / 4u) - (int32_t)(pn / 4u);
    const float a = j < pn / 2u ? prev[pn / 2u + j] : 0.0f;
    const float b = ci >= 0 && (uint32_t)ci < n / 2u ? cur[(uint32_t)ci] : 0.0f;
    return a + b;
}

// V5, and V6: what is not a number is stored as 0 -- no float reaches the conversion unclamped
VB_HD int32_t to_pcm16(float x)
{
    const float v = floorf(x * 32768.0f + 0.5f);
    if (v != v) return 0;
    return v < -32768.0f ? -32768 : v > 32767.0f ? 32767 : (int32_t)v;
}


// ---- host only: the tables, and the setup parse
inline void db_table(float out[256]) { for (int i = 0; i < 256; i++) out[i] = (float)std::pow(10.0, 7.0 * (i - 255) / 256.0); }
inline void window_slope(uint32_t n, float* out)      // n / 2 values
{
    const double pi = 3.14159265358979323846;
    for (uint32_t i = 0; i < n / 2u; i++) { const double s = std::sin((i + 0.5) / n * pi); out[i] = (float)std::sin(0.5 * pi * s * s); }
}

// Codewords from lengths: free subtrees as (depth, prefix); an entry takes the one whose leftmost leaf at its length is lowest.
inline int assign_codewords(const uint8_t* lengths, size_t n, uint32_t* codewords)
{
    struct Free { uint32_t depth; uint64_t prefix; };
    std::vector<Free> free_{{0u, 0u}};
    for (size_t i = 0; i < n; i++) {
        codewords[i] = 0;
        const uint32_t L = lengths[i];
        if (!L) continue;
        if (L > 32) return kParseInvalid;
        size_t best = free_.size();
        uint64_t best_cw = 0;
        for (size_t k = 0; k < free_.size(); k++) {
            if (free_[k].depth > L) continue;
            const uint64_t cw = free_[k].prefix << (L - free_[k].depth);
            if (best == free_.size() || cw < best_cw) { best = k; best_cw = cw; }
        }
        if (best == free_.size()) return kParseInvalid;                     // over-specified
        const uint32_t d = free_[best].depth;
        free_.erase(free_.begin() + (long)best);
        for (uint32_t k = d + 1; k <= L; k++) free_.push_back(Free{k, (best_cw >> (L - k)) | 1u});
        codewords[i] = (uint32_t)best_cw;
    }
    return kParseOk;
}

inline float float32_unpack(uint32_t x)
{
    const double mant = (double)(x & 0x1fffffu), e = (double)((x >> 21) & 0x3ffu);
    return (float)std::ldexp((x & 0x80000000u) ? -mant : mant, (int)e - 788);
}
inline uint32_t lookup1_values(uint32_t entries, uint32_t dim)
{
    uint32_t r = 0;
    for (;;) {                                                             // the greatest r with r^dim <= entries
        uint64_t pw = 1;
        bool over = false;
        for (uint32_t k = 0; k < dim && !over; k++) { pw *= (uint64_t)(r + 1u); over = pw > entries; }
        if (over) return r;
        r++;
    }
}

struct ParsedInfo { uint32_t channels, rate, bs0, bs1, books, modes; };

// The two header packets -> the image's words.  kParseOk, kParseInvalid or kParseUnsupported; *why names the reason.
inline int parse_setup(const uint8_t* id, size_t id_bytes, const uint8_t* setup, size_t setup_bytes, std::vector<uint32_t>* words, ParsedInfo* info, const char** why)
{
#define VB_FAIL(code, text) do { *why = text; return code; } while (0)
    if (id_bytes > 0x7fffffffu || setup_bytes > 0x7fffffffu) VB_FAIL(kParseInvalid, "header packet too large");
    Bits b = bits_open(id, (uint32_t)id_bytes);
    const auto magic = [&](uint32_t type) {
        bool ok = get(b, 8) == type;
        for (const char* c = "vorbis"; *c; c++) ok = (get(b, 8) == (uint32_t)(uint8_t)*c) && ok;
        return ok && !b.eop;
    };
    if (!magic(1)) VB_FAIL(kParseInvalid, "not an identification header");
    if (get(b, 32) != 0) VB_FAIL(kParseInvalid, "vorbis version");
    Image im;
    memset(&im, 0, sizeof(im));
    im.magic = kMagic;
    im.channels = get(b, 8); im.rate = get(b, 32);
    (void)get(b, 32); (void)get(b, 32); (void)get(b, 32);
    const uint32_t e0 = get(b, 4), e1 = get(b, 4);
    if (get(b, 1) != 1 || b.eop) VB_FAIL(kParseInvalid, "identification header framing");
    if (im.channels == 0 || im.rate == 0 || e0 < 6 || e1 > 13 || e0 > e1) VB_FAIL(kParseInvalid, "identification header values");
    if (im.channels > kMaxChannels) VB_FAIL(kParseUnsupported, "more than 8 channels");
    im.bs0 = 1u << e0; im.bs1 = 1u << e1;
    const uint32_t ch = im.channels;

    b = bits_open(setup, (uint32_t)setup_bytes);
    if (!magic(5)) VB_FAIL(kParseInvalid, "not a setup header");
    std::vector<uint32_t>& w = *words;
    w.assign(sizeof(Image) / 4, 0u);
    // codebooks
    im.n_books = get(b, 8) + 1u;
    std::vector<Book> books(im.n_books);
    for (uint32_t bi = 0; bi < im.n_books; bi++) {
        Book& bk = books[bi];
        memset(&bk, 0, sizeof(bk));
        if (get(b, 24) != 0x564342u) VB_FAIL(kParseInvalid, "codebook sync");
        bk.dim = get(b, 16); bk.entries = get(b, 24);
        if (b.eop) VB_FAIL(kParseInvalid, "setup header ends in a codebook");
        if ((uint64_t)bk.entries > (uint64_t)setup_bytes * 8u + 32u) VB_FAIL(kParseInvalid, "codebook entries beyond the header's bits");
        std::vector<uint8_t> len(bk.entries, 0);
        if (!get(b, 1)) {
            const uint32_t sparse = get(b, 1);
            for (uint32_t e = 0; e < bk.entries && !b.eop; e++)
                if (!sparse || get(b, 1)) len[e] = (uint8_t)(get(b, 5) + 1u);
        } else {
            uint32_t cur = 0, L = get(b, 5) + 1u;
            while (cur < bk.entries && !b.eop) {
                const uint32_t number = get(b, ilog(bk.entries - cur));
                if (number > bk.entries - cur || L > 32) VB_FAIL(kParseInvalid, "ordered codebook lengths");
                for (uint32_t k = 0; k < number; k++) len[cur + k] = (uint8_t)L;
                cur += number; L++;
            }
        }
        if (b.eop) VB_FAIL(kParseInvalid, "setup header ends in a codebook");
        std::vector<uint32_t> cws(bk.entries);
        if (assign_codewords(len.data(), len.size(), cws.data()) != kParseOk) VB_FAIL(kParseInvalid, "over-specified codebook");
        std::vector<int32_t> tree{-1, -1};
        for (uint32_t e = 0; e < bk.entries; e++) {
            if (!len[e]) continue;
            bk.used++;
            int32_t node = 0;
            for (uint32_t k = len[e]; k-- > 0;) {
                const uint32_t bit = (cws[e] >> k) & 1u;
                if (k == 0) { tree[(size_t)node * 2 + bit] = -(int32_t)e - 2; break; }
                int32_t c = tree[(size_t)node * 2 + bit];
                if (c < 0) { c = (int32_t)(tree.size() / 2); tree[(size_t)node * 2 + bit] = c; tree.push_back(-1); tree.push_back(-1); }
                node = c;
            }
        }
        bk.off_tree = (uint32_t)w.size(); bk.n_nodes = (uint32_t)(tree.size() / 2);
        for (int32_t v : tree) w.push_back((uint32_t)v);
        bk.lookup = get(b, 4);
        if (bk.lookup > 2) VB_FAIL(kParseInvalid, "codebook lookup type");
        if (bk.lookup) {
            const float vmin = float32_unpack(get(b, 32)), delta = float32_unpack(get(b, 32));
            const uint32_t vbits = get(b, 4) + 1u, seq = get(b, 1);
            if (bk.dim == 0) VB_FAIL(kParseInvalid, "codebook of dimension 0 with values");
            const uint64_t total = (uint64_t)bk.entries * bk.dim;
            if (total * 4u + (uint64_t)w.size() * 4u > kMaxImageBytes) VB_FAIL(kParseUnsupported, "setup image beyond its cap");
            const uint64_t nmult = bk.lookup == 1 ? lookup1_values(bk.entries, bk.dim) : total;
            if (nmult * vbits > (uint64_t)setup_bytes * 8u) VB_FAIL(kParseInvalid, "codebook values beyond the header's bits");
            std::vector<uint32_t> mult((size_t)nmult);
            for (uint64_t k = 0; k < nmult; k++) mult[(size_t)k] = get(b, vbits);
            if (b.eop) VB_FAIL(kParseInvalid, "setup header ends in a codebook");
            bk.off_values = (uint32_t)w.size();
            for (uint32_t e = 0; e < bk.entries; e++) {
                float last = 0.0f;
                uint64_t div = 1;
                for (uint32_t d = 0; d < bk.dim; d++) {
                    const uint64_t off = bk.lookup == 1 ? (e / div) % nmult : (uint64_t)e * bk.dim + d;
                    volatile float prod = (float)mult[(size_t)off] * delta;      // one float32 operation at a time
                    volatile float sum = prod + vmin;
                    const float v = sum + last;
                    if (!std::isfinite(v)) VB_FAIL(kParseInvalid, "codebook value vector entry not finite");   // V6
                    if (seq) last = v;
                    uint32_t raw; memcpy(&raw, &v, 4);
                    w.push_back(raw);
                    if (bk.lookup == 1) div *= nmult;
                }
            }
        }
    }
    // time domain transforms
    for (uint32_t k = get(b, 6) + 1u; k-- > 0;) if (get(b, 16) != 0) VB_FAIL(kParseInvalid, "time domain transform");
    // floors
    im.n_floors = get(b, 6) + 1u;
    std::vector<Floor> floors(im.n_floors);
    for (Floor& f : floors) {
        memset(&f, 0, sizeof(f));
        const uint32_t type = get(b, 16);
        if (b.eop) VB_FAIL(kParseInvalid, "setup header ends in the floors");
        if (type == 0) VB_FAIL(kParseUnsupported, "floor type 0");
        if (type != 1) VB_FAIL(kParseInvalid, "floor type");
        f.partitions = get(b, 5);
        int32_t maxclass = -1;
        for (uint32_t i = 0; i < f.partitions; i++) { f.part_class[i] = (uint8_t)get(b, 4); if ((int32_t)f.part_class[i] > maxclass) maxclass = f.part_class[i]; }
        for (int32_t c = 0; c <= maxclass; c++) {
            f.class_dim[c] = (uint8_t)(get(b, 3) + 1u); f.class_sub[c] = (uint8_t)get(b, 2);
            f.class_master[c] = -1;
            if (f.class_sub[c]) { f.class_master[c] = (int16_t)get(b, 8); if ((uint32_t)f.class_master[c] >= im.n_books) VB_FAIL(kParseInvalid, "floor master book"); }
            for (uint32_t j = 0; j < 8; j++) f.sub_book[c][j] = -1;
            for (uint32_t j = 0; j < (1u << f.class_sub[c]); j++) {
                f.sub_book[c][j] = (int16_t)((int32_t)get(b, 8) - 1);
                if (f.sub_book[c][j] >= (int32_t)im.n_books) VB_FAIL(kParseInvalid, "floor subclass book");
            }
        }
        f.multiplier = get(b, 2) + 1u; f.rangebits = get(b, 4);
        f.x[0] = 0; f.x[1] = (uint16_t)(1u << f.rangebits);
        f.values = 2;
        for (uint32_t i = 0; i < f.partitions; i++)
            for (uint32_t j = 0; j < f.class_dim[f.part_class[i]]; j++) {
                if (f.values >= kMaxFloorValues) VB_FAIL(kParseInvalid, "more than 65 floor values");
                f.x[f.values++] = (uint16_t)get(b, f.rangebits);
            }
        if (b.eop) VB_FAIL(kParseInvalid, "setup header ends in the floors");
        for (uint32_t i = 0; i < f.values; i++) f.sorted[i] = (uint8_t)i;
        for (uint32_t i = 1; i < f.values; i++)                             // by x (the values are few)
            for (uint32_t k = i; k > 0 && f.x[f.sorted[k - 1]] > f.x[f.sorted[k]]; k--) { const uint8_t t = f.sorted[k]; f.sorted[k] = f.sorted[k - 1]; f.sorted[k - 1] = t; }
        for (uint32_t i = 1; i < f.values; i++) if (f.x[f.sorted[i]] == f.x[f.sorted[i - 1]]) VB_FAIL(kParseInvalid, "floor values repeat");
        for (uint32_t i = 2; i < f.values; i++) {
            int32_t lo = -1, hi = -1;
            for (uint32_t k = 0; k < i; k++) {
                if (f.x[k] < f.x[i] && (lo < 0 || f.x[k] > f.x[lo])) lo = (int32_t)k;
                if (f.x[k] > f.x[i] && (hi < 0 || f.x[k] < f.x[hi])) hi = (int32_t)k;
            }
            if (lo < 0 || hi < 0) VB_FAIL(kParseInvalid, "floor value outside its range");
            f.low[i] = (uint8_t)lo; f.high[i] = (uint8_t)hi;
        }
    }
    // residues
    im.n_residues = get(b, 6) + 1u;
    std::vector<Residue> residues(im.n_residues);
    for (Residue& r : residues) {
        memset(&r, 0, sizeof(r));
        r.type = get(b, 16);
        if (r.type > 2 || b.eop) VB_FAIL(kParseInvalid, "residue type");
        r.begin = get(b, 24); r.end = get(b, 24); r.psize = get(b, 24) + 1u; r.classifications = get(b, 6) + 1u; r.classbook = get(b, 8);
        if (r.classbook >= im.n_books || books[r.classbook].dim == 0) VB_FAIL(kParseInvalid, "residue classbook");
        for (uint32_t c = 0; c < r.classifications; c++) {
            const uint32_t low = get(b, 3), high = get(b, 1) ? get(b, 5) : 0u;
            r.cascade[c] = (uint8_t)(high * 8u + low);
        }
        for (uint32_t c = 0; c < 64; c++) for (uint32_t j = 0; j < 8; j++) r.books[c][j] = -1;
        for (uint32_t c = 0; c < r.classifications; c++)
            for (uint32_t j = 0; j < 8; j++)
                if ((r.cascade[c] >> j) & 1u) {
                    const uint32_t book = get(b, 8);
                    if (b.eop || book >= im.n_books || !books[book].lookup || !books[book].dim) VB_FAIL(kParseInvalid, "residue book without value vectors");
                    r.books[c][j] = (int16_t)book;
                }
        if (b.eop) VB_FAIL(kParseInvalid, "setup header ends in the residues");
        const uint64_t vecs = r.type == 2 ? 1u : ch, actual = r.type == 2 ? (uint64_t)(im.bs1 / 2u) * ch : im.bs1 / 2u;
        const uint64_t lb = r.begin < actual ? r.begin : actual, le = r.end < actual ? r.end : actual;
        const uint64_t need = le > lb ? vecs * ((le - lb) / r.psize + books[r.classbook].dim) : 0u;
        if (need > kMaxClassBytes) VB_FAIL(kParseUnsupported, "residue classifications beyond their cap");
        if (need > im.class_bytes) im.class_bytes = (uint32_t)need;
    }
    // mappings
    im.n_mappings = get(b, 6) + 1u;
    std::vector<Mapping> mappings(im.n_mappings);
    for (Mapping& m : mappings) {
        memset(&m, 0, sizeof(m));
        if (get(b, 16) != 0 || b.eop) VB_FAIL(kParseInvalid, "mapping type");
        m.submaps = get(b, 1) ? get(b, 4) + 1u : 1u;
        if (get(b, 1)) {
            m.steps = get(b, 8) + 1u;
            if (m.steps > kMaxCoupling) VB_FAIL(kParseUnsupported, "more than 32 coupling steps");
            for (uint32_t s = 0; s < m.steps; s++) {
                const uint32_t mag = get(b, ilog(ch - 1u)), ang = get(b, ilog(ch - 1u));
                if (mag == ang || mag >= ch || ang >= ch) VB_FAIL(kParseInvalid, "coupling channels");
                m.mag[s] = (uint8_t)mag; m.ang[s] = (uint8_t)ang;
            }
        }
        if (get(b, 2) != 0) VB_FAIL(kParseInvalid, "mapping reserved bits");
        if (m.submaps > 1)
            for (uint32_t c = 0; c < ch; c++) { m.mux[c] = (uint8_t)get(b, 4); if (m.mux[c] >= m.submaps) VB_FAIL(kParseInvalid, "mapping mux"); }
        for (uint32_t s = 0; s < m.submaps; s++) {
            (void)get(b, 8);
            m.sub_floor[s] = (uint8_t)get(b, 8); m.sub_residue[s] = (uint8_t)get(b, 8);
            if (m.sub_floor[s] >= im.n_floors || m.sub_residue[s] >= im.n_residues) VB_FAIL(kParseInvalid, "submap floor or residue");
        }
        if (b.eop) VB_FAIL(kParseInvalid, "setup header ends in the mappings");
    }
    // modes
    im.n_modes = get(b, 6) + 1u;
    im.mode_bits = ilog(im.n_modes - 1u);
    std::vector<Mode> modes(im.n_modes);
    for (Mode& m : modes) {
        m.blockflag = get(b, 1);
        if (get(b, 16) != 0 || get(b, 16) != 0) VB_FAIL(kParseInvalid, "mode window or transform type");
        m.mapping = get(b, 8);
        if (m.mapping >= im.n_mappings) VB_FAIL(kParseInvalid, "mode mapping");
    }
    if (get(b, 1) != 1 || b.eop) VB_FAIL(kParseInvalid, "setup header framing");
    const auto append = [&](const void* p, size_t bytes) { const size_t at = w.size(); w.resize(at + bytes / 4); memcpy(&w[at], p, bytes); return (uint32_t)at; };
    im.off_books = append(books.data(), books.size() * sizeof(Book));
    im.off_floors = append(floors.data(), floors.size() * sizeof(Floor));
    im.off_residues = append(residues.data(), residues.size() * sizeof(Residue));
    im.off_mappings = append(mappings.data(), mappings.size() * sizeof(Mapping));
    im.off_modes = append(modes.data(), modes.size() * sizeof(Mode));
    if ((uint64_t)w.size() * 4u > kMaxImageBytes) VB_FAIL(kParseUnsupported, "setup image beyond its cap");
    im.words = (uint32_t)w.size();
    memcpy(w.data(), &im, sizeof(im));
    *info = ParsedInfo{im.channels, im.rate, im.bs0, im.bs1, im.n_books, im.n_modes};
    return kParseOk;
#undef VB_FAIL
}


// Is this blob an image the device text can follow without a check of its own?  The head's counts and table places, every codebook's
// tree and value vectors inside the image and every child inside its tree, every index of a floor, residue, mapping and mode in range,
// the limits of V1.  (ohgpu_vorbis_batch_check runs it on every descriptor's image.)
inline bool image_valid(const uint32_t* img, uint64_t bytes)
{
    if (bytes < sizeof(Image) || bytes % 4u) return false;
    const Image& im = image_head(img);
    const uint64_t w = im.words;
    const auto pow2 = [](uint32_t v) { return v && !(v & (v - 1u)); };
    if (im.magic != kMagic || w * 4u != bytes || im.channels < 1 || im.channels > kMaxChannels || !pow2(im.bs0) || !pow2(im.bs1) || im.bs0 < 64 || im.bs1 > 8192 || im.bs0 > im.bs1) return false;
    if (im.n_books < 1 || im.n_books > 256 || im.n_floors < 1 || im.n_floors > 64 || im.n_residues < 1 || im.n_residues > 64 || im.n_mappings < 1 || im.n_mappings > 64 ||
        im.n_modes < 1 || im.n_modes > 64 || im.mode_bits != ilog(im.n_modes - 1u) || im.class_bytes > kMaxClassBytes) return false;
    const auto table = [&](uint32_t off, uint32_t count, size_t record) { return off >= sizeof(Image) / 4 && off + (uint64_t)count * (record / 4) <= w; };
    if (!table(im.off_books, im.n_books, sizeof(Book)) || !table(im.off_floors, im.n_floors, sizeof(Floor)) || !table(im.off_residues, im.n_residues, sizeof(Residue)) ||
        !table(im.off_mappings, im.n_mappings, sizeof(Mapping)) || !table(im.off_modes, im.n_modes, sizeof(Mode))) return false;
    for (uint32_t i = 0; i < im.n_books; i++) {
        const Book& b = image_book(img, i);
        if (b.n_nodes < 1 || b.off_tree + 2ull * b.n_nodes > w || b.lookup > 2 || b.entries > (1u << 24)) return false;
        const int32_t* tree = (const int32_t*)(img + b.off_tree);
        for (uint64_t k = 0; k < 2ull * b.n_nodes; k++)
            if (tree[k] >= (int32_t)b.n_nodes || (tree[k] <= -2 && (uint32_t)(-(tree[k] + 2)) >= b.entries)) return false;
        if (b.lookup && (b.dim < 1 || b.off_values + (uint64_t)b.entries * b.dim > w)) return false;
    }
    for (uint32_t i = 0; i < im.n_floors; i++) {
        const Floor& f = image_floor(img, i);
        if (f.partitions > 31 || f.multiplier < 1 || f.multiplier > 4 || f.values < 2 || f.values > kMaxFloorValues) return false;
        uint32_t values = 2;
        for (uint32_t k = 0; k < f.partitions; k++) {
            const uint32_t c = f.part_class[k];
            if (c > 15 || f.class_dim[c] < 1 || f.class_dim[c] > 8 || f.class_sub[c] > 3) return false;
            if (f.class_sub[c] && (f.class_master[c] < 0 || (uint32_t)f.class_master[c] >= im.n_books)) return false;
            for (uint32_t j = 0; j < 8; j++) if (f.sub_book[c][j] < -1 || f.sub_book[c][j] >= (int32_t)im.n_books) return false;
            values += f.class_dim[c];
        }
        if (values != f.values) return false;
        for (uint32_t k = 0; k < f.values; k++) {
            if (f.sorted[k] >= f.values || (k && f.x[f.sorted[k]] <= f.x[f.sorted[k - 1]])) return false;
            if (k >= 2 && (f.low[k] >= k || f.high[k] >= k || f.x[f.low[k]] >= f.x[k] || f.x[f.high[k]] <= f.x[k])) return false;
        }
    }
    for (uint32_t i = 0; i < im.n_residues; i++) {
        const Residue& r = image_residue(img, i);
        if (r.type > 2 || r.psize < 1 || r.classifications < 1 || r.classifications > 64 || r.classbook >= im.n_books || image_book(img, r.classbook).dim < 1) return false;
        const uint64_t vecs = r.type == 2 ? 1u : im.channels, actual = r.type == 2 ? (uint64_t)(im.bs1 / 2u) * im.channels : im.bs1 / 2u;
        const uint64_t lb = r.begin < actual ? r.begin : actual, le = r.end < actual ? r.end : actual;
        if (le > lb && vecs * ((le - lb) / r.psize + image_book(img, r.classbook).dim) > im.class_bytes) return false;
        for (uint32_t c = 0; c < 64; c++)
            for (uint32_t j = 0; j < 8; j++) {
                const int32_t k = r.books[c][j];
                if (k < -1 || k >= (int32_t)im.n_books || (k >= 0 && !image_book(img, (uint32_t)k).lookup)) return false;
            }
    }
    for (uint32_t i = 0; i < im.n_mappings; i++) {
        const Mapping& m = image_mapping(img, i);
        if (m.submaps < 1 || m.submaps > 16 || m.steps > kMaxCoupling) return false;
        for (uint32_t k = 0; k < m.steps; k++) if (m.mag[k] >= im.channels || m.ang[k] >= im.channels || m.mag[k] == m.ang[k]) return false;
        for (uint32_t c = 0; c < im.channels; c++) if (m.mux[c] >= m.submaps) return false;
        for (uint32_t k = 0; k < m.submaps; k++) if (m.sub_floor[k] >= im.n_floors || m.sub_residue[k] >= im.n_residues) return false;
    }
    for (uint32_t i = 0; i < im.n_modes; i++) if (image_mode(img, i).blockflag > 1 || image_mode(img, i).mapping >= im.n_mappings) return false;
    return true;
}

}  // namespace vorbiscore
