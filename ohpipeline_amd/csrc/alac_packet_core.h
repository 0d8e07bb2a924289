// alac_packet_core.h -- Apple Lossless packets, written from the format's behaviour: the 24-byte stream configuration, the packet's
// elements, the adaptive Golomb code of the residuals, the sign-sign adaptive predictor, the channel-pair matrix and the three output
// forms.  Everything here is __host__ __device__: csrc/alac_packet_kernel.hip runs this text on the device,
// tests/cpp/alac_core_driver.cpp runs the same text on the CPU under the sanitizers.
//
// Reading of the format:
//   packet     elements behind a 3-bit tag: 0 single channel, 1 channel pair, 3 LFE (a single channel), 4 data (skipped), 6 fill
//              (skipped), 7 end; 2 and 5 are refused.  The walk ends once the stream's channels are there; an end tag, or a pair that
//              does not fit any more, leaves the channels still missing silent.
//   element    4-bit instance, 12 zero bits, partial flag, 2 bits "bytes shifted" (3 refused), escape flag; partial: a 32-bit sample
//              count.  Sample width w = depth - 8 * shifted, one more for a pair.
//              compressed: matrix bits (u8) and weight (s8); per channel mode, rounding shift, code factor, order and the
//              coefficients; the shifted-off low bytes, a pair's interleaved; per channel the residuals.
//              escape: depth bits per sample, a pair's interleaved; no shift, no matrix.
//   residuals  a running mean m picks the code: k = min(floor(log2((m >> 9) + 3)), kb); a unary prefix of up to eight ones, nine meaning
//              "w raw bits follow"; k bits whose values 0 and 1 are one bit shorter; the lowest bit of the decoded number is the sign.
//              A mean below 128 switches to a run of zeros with its own 16-bit escape.
//   predictor  order 0 copies, order 31 is a running sum, anything else warms up with a running sum and then adapts its coefficients
//              by the signs of the residual and of the history; every sum wraps at 32 bits and every coefficient at 16.
//
// Where this text is stricter than the reference decoder (include/ohgpu.h lists the same): bits past the packet's end read as zero
// and an element that needed one is corrupt; a compressed element's w outside 1..32 is corrupt; a sample count above the stream's
// frame length, or audio elements of one packet that disagree about it, is corrupt; depth 20, and a kb outside 1..31, are
// unsupported; a rounding shift of zero rounds with nothing (the reference shifts one by minus one); a matrix shift above 31 shifts
// by 31; an escaped element always carries depth bits per sample.  A packet that fails writes nothing.
//
// Every loop is bounded by the packet's bit count or the frame length, and no load goes past the packet.
#pragma once

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define ALAC_HD __host__ __device__ inline
#else
#define ALAC_HD inline
#endif

namespace alaccore {

enum { kStatusOk = 0, kStatusCorrupt = 1, kStatusUnsupported = 2 };            // OHGPU_ALAC_*
enum { kFlagPackedLe = 1, kFlagPackedBe = 2 };                                 // OHGPU_ALAC_OUT_*
enum { kMaxChannels = 8, kMaxOrder = 32, kMaxFrameLength = 16384, kGroupRows = 64 };
enum { kChanCompressed = 0, kChanRaw = 1, kChanSilent = 2 };

struct Stream {                  // a descriptor as the device sees it: 48 bytes
    uint64_t dst_offset, dst_plane_stride;
    uint32_t first_packet, n_packets;
    uint32_t frame_length, sample_rate;
    uint16_t max_run;
    uint8_t  bit_depth, pb, mb, kb, channels, flags;
    uint64_t reserved;
};

struct Packet {                  // one packet of the table: 32 bytes
    uint64_t src_offset;
    uint32_t bytes, stream;
    uint32_t index;              // its place within the stream: it lands at sample index * frame_length
    uint32_t row0;               // its first row of scratch (one row per channel of its stream)
    uint64_t reserved;
};

struct PacketOut { uint32_t status, samples; };

struct Chan {                    // one channel of one packet: 80 bytes
    int16_t  coef[kMaxOrder];
    uint8_t  kind, mode, den_shift, order;
    uint8_t  mix_bits, shifted, width, place;     // place: 0 a single channel, 1 / 2 the first / second of a pair
    int8_t   mix_res;
    uint8_t  pad[3];
    uint32_t low_bit0;           // where the element's shifted-off low bytes begin, in bits from the packet's start
};

// A row of scratch: sample i at p[i * stride].  The plain layout has stride 1; the transposed one keeps kGroupRows rows side by side.
struct Row {
    int32_t* p;
    uint32_t stride;
    ALAC_HD int32_t get(uint32_t i) const { return p[(uint64_t)i * stride]; }
    ALAC_HD void put(uint32_t i, int32_t v) const { p[(uint64_t)i * stride] = v; }
};

// Row `row` of the transposed scratch: groups of kGroupRows rows, group g starting at word group_base[g] * kGroupRows.
ALAC_HD Row transposed_row(int32_t* scratch, const uint64_t* group_base, uint32_t row)
{
    Row r;
    r.p = scratch + group_base[row / kGroupRows] * kGroupRows + row % kGroupRows;
    r.stride = kGroupRows;
    return r;
}

// Row `row` of the plain layout: the same groups, each row's samples side by side (a group's length is the next group's start less its own).
ALAC_HD Row plain_row(int32_t* scratch, const uint64_t* group_base, uint32_t row)
{
    const uint32_t g = row / kGroupRows;
    Row r;
    r.p = scratch + group_base[g] * kGroupRows + (uint64_t)(row % kGroupRows) * (group_base[g + 1] - group_base[g]);
    r.stride = 1;
    return r;
}

struct TransposedRows {
    int32_t* scratch; const uint64_t* group_base; uint32_t row0;
    ALAC_HD Row operator()(uint32_t c) const { return transposed_row(scratch, group_base, row0 + c); }
};
struct PlainRows {
    int32_t* scratch; const uint64_t* group_base; uint32_t row0;
    ALAC_HD Row operator()(uint32_t c) const { return plain_row(scratch, group_base, row0 + c); }
};

// The rows of a batch (host).  A packet's rows are consecutive and never straddle a group; a group holds rows of one frame length.
// group_base gets one entry per group and the end of the last; row_packet one per row, padding included (~0u there); packets[].row0 is set.
inline void plan_rows(const Stream* streams, Packet* packets, size_t n_packets, std::vector<uint64_t>* group_base, std::vector<uint32_t>* row_packet)
{
    group_base->clear();
    row_packet->clear();
    uint64_t lines = 0;
    uint32_t length = 0;
    for (size_t i = 0; i < n_packets; i++) {
        const Stream& s = streams[packets[i].stream];
        const uint32_t used = (uint32_t)(row_packet->size() % kGroupRows);
        if (used != 0 && (s.frame_length != length || used + s.channels > kGroupRows)) row_packet->resize(row_packet->size() + (kGroupRows - used), ~0u);
        if (row_packet->size() % kGroupRows == 0) {
            group_base->push_back(lines);
            length = s.frame_length;
            lines += length;
        }
        packets[i].row0 = (uint32_t)row_packet->size();
        row_packet->insert(row_packet->end(), s.channels, (uint32_t)i);
    }
    if (row_packet->size() % kGroupRows) row_packet->resize(row_packet->size() + (kGroupRows - row_packet->size() % kGroupRows), ~0u);
    group_base->push_back(lines);
}

// ---- bits, most significant first; a position past the end reads zeros and is the caller's to notice (pos > bits) ----
struct Bits {
    const uint8_t* p;
    uint32_t bytes, bits, pos;
};

ALAC_HD uint32_t peek32(const Bits& b, uint32_t pos)            // the 32 bits from `pos` on
{
    const uint32_t at = pos >> 3;
    uint64_t w = 0;
    for (uint32_t i = 0; i < 5; i++) w = (w << 8) | (at + i < b.bytes ? b.p[at + i] : 0u);
    return (uint32_t)(w >> (8u - (pos & 7u)));
}
ALAC_HD uint32_t peek(const Bits& b, uint32_t pos, uint32_t k) { return k == 0 ? 0u : peek32(b, pos) >> (32u - k); }     // k <= 32
ALAC_HD uint32_t take(Bits* b, uint32_t k) { const uint32_t v = peek(*b, b->pos, k); b->pos += k; return v; }
ALAC_HD bool dry(const Bits& b) { return b.pos > b.bits; }
ALAC_HD uint32_t ones_in_front(uint32_t w) { const uint32_t z = ~w; return z ? (uint32_t)__builtin_clz(z) : 32u; }
ALAC_HD int32_t sign_extend(uint32_t v, uint32_t width) { const uint32_t s = 32u - width; return (int32_t)(v << s) >> s; }    // width 1..32

// ---- the residuals of one channel: n numbers into `row`.  False: a run went past n, or the packet ended first. ----
ALAC_HD bool read_residuals(Bits* b, const Stream& s, uint32_t pb, uint32_t width, uint32_t n, const Row& row)
{
    const uint32_t run_mask = (1u << s.kb) - 1u;                 // (kb is 1..31 here)
    uint32_t mean = s.mb, after_run = 0, c = 0;
    while (c < n) {
        if (dry(*b)) return false;
        uint32_t k = 31u - (uint32_t)__builtin_clz((mean >> 9) + 3u);
        if (k > s.kb) k = s.kb;
        const uint32_t step = (1u << k) - 1u;
        const uint32_t prefix = ones_in_front(peek32(*b, b->pos));
        uint32_t v;
        if (prefix >= 9u) {
            b->pos += 9u;
            v = take(b, width);
        } else {
            b->pos += prefix + 1u;
            v = prefix * step;
            if (k > 1u) {
                const uint32_t low = peek(*b, b->pos, k);
                if (low >= 2u) { v += low - 1u; b->pos += k; } else b->pos += k - 1u;
            }
        }
        const uint32_t coded = v + after_run;
        const uint32_t half = (coded + 1u) >> 1;
        row.put(c++, (int32_t)((coded & 1u) ? 0u - half : half));
        mean = pb * coded + mean - ((pb * mean) >> 9);
        if (v > 0xffffu) mean = 0xffffu;
        after_run = 0;
        if (mean < 128u && c < n) {                              // ((mean << 2) < 512: the mean never reaches 2^30)
            after_run = 1;
            const uint32_t kz = (uint32_t)__builtin_clz(mean | 1u) + (mean ? 0u : 1u) - 24u + ((mean + 16u) >> 6);
            const uint32_t stepz = ((1u << kz) - 1u) & run_mask;
            const uint32_t pre = ones_in_front(peek32(*b, b->pos));
            uint32_t run;
            if (pre >= 9u) {
                b->pos += 9u;
                run = take(b, 16);
            } else {
                b->pos += pre + 1u;
                const uint32_t low = peek(*b, b->pos, kz);
                run = pre * stepz;
                if (low >= 2u) { run += low - 1u; b->pos += kz; } else b->pos += kz - 1u;
            }
            if (run > n - c) return false;
            for (uint32_t j = 0; j < run; j++) row.put(c++, 0);
            if (run >= 65535u) after_run = 0;
            mean = 0;
        }
    }
    return !dry(*b);
}

// ---- the predictor, in place over a row's first n words ----
ALAC_HD int32_t sign_of(int32_t v) { return (v > 0) - (v < 0); }

ALAC_HD void running_sum(const Row& row, uint32_t from, uint32_t to, uint32_t width)      // out[j] = in[j] + out[j - 1], j in [from, to)
{
    if (from >= to) return;
    uint32_t prev = (uint32_t)row.get(from - 1u);
    for (uint32_t j = from; j < to; j++) {
        prev = (uint32_t)sign_extend((uint32_t)row.get(j) + prev, width);
        row.put(j, (int32_t)prev);
    }
}

ALAC_HD void predict_pass(const Row& row, uint32_t n, int16_t* coef, uint32_t order, uint32_t width, uint32_t den_shift)
{
    if (order == 0 || n < 2) return;
    if (order == 31) { running_sum(row, 1, n, width); return; }
    const uint32_t lim = order + 1u;
    running_sum(row, 1, lim < n ? lim : n, width);
    const uint32_t round = den_shift ? 1u << (den_shift - 1u) : 0u;
    for (uint32_t j = lim; j < n; j++) {
        const uint32_t top = (uint32_t)row.get(j - lim);
        uint32_t sum = 0;
        for (uint32_t k = 0; k < order; k++) sum += (uint32_t)(int32_t)coef[k] * ((uint32_t)row.get(j - 1u - k) - top);
        const int32_t res = row.get(j);
        row.put(j, sign_extend((uint32_t)res + top + (uint32_t)((int32_t)(sum + round) >> den_shift), width));
        const int32_t sg = sign_of(res);
        if (sg == 0) continue;
        uint32_t left = (uint32_t)res;
        for (uint32_t k = order; k-- > 0;) {
            const uint32_t dd = top - (uint32_t)row.get(j - 1u - k);
            const int32_t sgn = sign_of((int32_t)dd) * sg;        // the history's sign, turned by the residual's
            coef[k] = (int16_t)((uint32_t)(int32_t)coef[k] - (uint32_t)sgn);
            left -= (order - k) * (uint32_t)((int32_t)((uint32_t)sgn * dd) >> den_shift);
            if (sg > 0 ? (int32_t)left <= 0 : (int32_t)left >= 0) break;
        }
    }
}

ALAC_HD void predict_row(const Chan& ch, const Row& row, uint32_t n)
{
    if (ch.kind != kChanCompressed) return;
    int16_t coef[kMaxOrder];
    for (uint32_t k = 0; k < kMaxOrder; k++) coef[k] = ch.coef[k];
    if (ch.mode != 0) predict_pass(row, n, coef, 31, ch.width, 0);
    predict_pass(row, n, coef, ch.order, ch.width, ch.den_shift);
}

// ---- one packet's elements: the channel records, the residuals / raw samples in the rows, the sample count ----
// rows(c) gives channel c's row.  Nothing but the rows and `chans` is written.
template <typename Rows>
ALAC_HD int parse_packet(const uint8_t* p, uint32_t bytes, const Stream& s, Chan* chans, const Rows& rows, uint32_t* samples)
{
    *samples = 0;
    if (s.bit_depth != 16 && s.bit_depth != 24 && s.bit_depth != 32) return kStatusUnsupported;
    if (s.kb < 1 || s.kb > 31) return kStatusUnsupported;
    Bits b;
    b.p = p; b.bytes = bytes; b.bits = bytes * 8u; b.pos = 0;
    uint32_t done = 0, n = s.frame_length;
    bool have_count = false;
    while (done < s.channels) {
        if (b.pos >= b.bits) return kStatusCorrupt;
        const uint32_t tag = take(&b, 3);
        if (tag == 7u) { if (dry(b)) return kStatusCorrupt; break; }
        if (tag == 2u || tag == 5u) return kStatusCorrupt;
        if (tag == 4u) {
            b.pos += 4;
            const uint32_t align = take(&b, 1);
            uint32_t count = take(&b, 8);
            if (count == 255u) count += take(&b, 8);
            if (align) b.pos = (b.pos + 7u) & ~7u;
            b.pos += count * 8u;
            if (dry(b)) return kStatusCorrupt;
            continue;
        }
        if (tag == 6u) {
            uint32_t count = take(&b, 4);
            if (count == 15u) count += take(&b, 8) - 1u;
            b.pos += count * 8u;
            if (dry(b)) return kStatusCorrupt;
            continue;
        }
        const uint32_t nch = tag == 1u ? 2u : 1u;
        if (done + nch > s.channels) break;                       // a pair too many: the rest stays silent
        b.pos += 4;                                               // the instance tag
        if (take(&b, 12) != 0u) return kStatusCorrupt;
        const uint32_t partial = take(&b, 1), shifted = take(&b, 2), escape = take(&b, 1);
        if (shifted == 3u) return kStatusCorrupt;
        if (partial) n = take(&b, 32);
        if (dry(b)) return kStatusCorrupt;
        if (n > s.frame_length || (have_count && n != *samples)) return kStatusCorrupt;
        have_count = true;
        *samples = n;
        const int32_t width = (int32_t)s.bit_depth - 8 * (int32_t)shifted + (nch == 2u ? 1 : 0);
        if (!escape && (width < 1 || width > 32)) return kStatusCorrupt;
        if (escape) {
            for (uint32_t c = 0; c < nch; c++) {
                Chan& ch = chans[done + c];
                ch.kind = kChanRaw; ch.mode = 0; ch.den_shift = 0; ch.order = 0; ch.mix_bits = 0; ch.mix_res = 0; ch.shifted = 0;
                ch.width = s.bit_depth; ch.place = (uint8_t)(nch == 2u ? c + 1u : 0u); ch.low_bit0 = 0;
            }
            if ((uint64_t)b.pos + (uint64_t)n * nch * s.bit_depth > b.bits) return kStatusCorrupt;
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t c = 0; c < nch; c++) rows(done + c).put(i, sign_extend(take(&b, s.bit_depth), s.bit_depth));
        } else {
            const uint32_t mix_bits = take(&b, 8);
            const int8_t mix_res = (int8_t)take(&b, 8);
            uint32_t factor[2] = {0, 0};
            for (uint32_t c = 0; c < nch; c++) {
                Chan& ch = chans[done + c];
                ch.kind = kChanCompressed;
                ch.mode = (uint8_t)take(&b, 4); ch.den_shift = (uint8_t)take(&b, 4);
                factor[c] = take(&b, 3); ch.order = (uint8_t)take(&b, 5);
                for (uint32_t k = 0; k < kMaxOrder; k++) ch.coef[k] = k < ch.order ? (int16_t)take(&b, 16) : (int16_t)0;
                ch.mix_bits = (uint8_t)mix_bits; ch.mix_res = mix_res; ch.shifted = (uint8_t)shifted; ch.width = (uint8_t)width;
                ch.place = (uint8_t)(nch == 2u ? c + 1u : 0u); ch.low_bit0 = 0;
            }
            if (dry(b)) return kStatusCorrupt;
            if (shifted) {
                const uint64_t low_bits = (uint64_t)n * nch * 8u * shifted;
                if (b.pos + low_bits > b.bits) return kStatusCorrupt;
                for (uint32_t c = 0; c < nch; c++) chans[done + c].low_bit0 = b.pos;
                b.pos += (uint32_t)low_bits;
            }
            for (uint32_t c = 0; c < nch; c++)
                if (!read_residuals(&b, s, ((uint32_t)s.pb * factor[c]) / 4u, (uint32_t)width, n, rows(done + c))) return kStatusCorrupt;
        }
        done += nch;
    }
    if (!have_count) *samples = s.frame_length;
    for (; done < s.channels; done++) {
        Chan& ch = chans[done];
        ch.kind = kChanSilent; ch.mode = 0; ch.den_shift = 0; ch.order = 0; ch.mix_bits = 0; ch.mix_res = 0; ch.shifted = 0; ch.width = s.bit_depth;
        ch.place = 0; ch.low_bit0 = 0;
    }
    return kStatusOk;
}

// ---- sample i of channel c of a parsed and predicted packet (mine / other: this channel's word and, in a pair, its partner's) ----
ALAC_HD int32_t finish_sample(const Chan& ch, int32_t mine, int32_t other, const uint8_t* p, uint32_t bytes, uint32_t i)
{
    if (ch.kind == kChanSilent) return 0;
    uint32_t v = (uint32_t)mine;
    if (ch.place != 0 && ch.mix_res != 0) {
        const uint32_t u = ch.place == 1 ? (uint32_t)mine : (uint32_t)other, w = ch.place == 1 ? (uint32_t)other : (uint32_t)mine;
        const uint32_t sh = ch.mix_bits > 31 ? 31u : ch.mix_bits;
        const uint32_t left = u + w - (uint32_t)((int32_t)((uint32_t)(int32_t)ch.mix_res * w) >> sh);
        v = ch.place == 1 ? left : left - w;
    }
    if (ch.shifted) {
        Bits b;
        b.p = p; b.bytes = bytes; b.bits = bytes * 8u; b.pos = 0;
        const uint32_t each = 8u * ch.shifted, nch = ch.place ? 2u : 1u, which = ch.place == 2 ? 1u : 0u;
        v = (v << each) | peek(b, ch.low_bit0 + (i * nch + which) * each, each);
    }
    return v;
}

ALAC_HD void store_sample(const Stream& s, uint8_t* dst, uint64_t index, uint32_t ch, int32_t v)
{
    if (s.flags & (kFlagPackedLe | kFlagPackedBe)) {
        const uint32_t bytes = s.bit_depth / 8u;
        uint8_t* q = dst + s.dst_offset + (index * s.channels + ch) * bytes;
        for (uint32_t b = 0; b < bytes; b++) q[(s.flags & kFlagPackedBe) ? bytes - 1u - b : b] = (uint8_t)((uint32_t)v >> (8u * b));
    } else {
        *(int32_t*)(dst + s.dst_offset + (uint64_t)ch * s.dst_plane_stride + index * 4u) = sign_extend((uint32_t)v, s.bit_depth);
    }
}

// All of one packet by one thread: parse, predict, finish, store.  `rows` is its work space.
template <typename Rows>
ALAC_HD void decode_packet(const uint8_t* p, const Packet& pk, const Stream& s, Chan* chans, const Rows& rows, uint8_t* dst, PacketOut* out)
{
    uint32_t n = 0;
    const int st = parse_packet(p, pk.bytes, s, chans, rows, &n);
    out->status = (uint32_t)st;
    out->samples = st == kStatusOk ? n : 0u;
    if (st != kStatusOk) return;
    for (uint32_t c = 0; c < s.channels; c++) predict_row(chans[c], rows(c), n);
    for (uint32_t c = 0; c < s.channels; c++) {
        const Chan& ch = chans[c];
        const uint32_t partner = ch.place == 1 ? c + 1u : ch.place == 2 ? c - 1u : c;
        for (uint32_t i = 0; i < n; i++) {
            const int32_t mine = ch.kind == kChanSilent ? 0 : rows(c).get(i), other = ch.place ? rows(partner).get(i) : 0;
            store_sample(s, dst, (uint64_t)pk.index * s.frame_length + i, c, finish_sample(ch, mine, other, p, pk.bytes, i));
        }
    }
}

}  // namespace alaccore
