// flac_frame_core.h -- native FLAC frames, written from the format's definition: bit reader, the two CRCs, frame header, subframe and
// residual parse, predictor restore, inter-channel decorrelation and the per-stream chain rule.  Everything here is
// __host__ __device__: csrc/flac_frame_kernel.hip runs this text on the device, tests/cpp/flac_core_driver.cpp runs the same text on
// the CPU under the sanitizers.
//
// Reading of the format (the numbers are the format document's):
//   frame header   14-bit sync 11111111111110, reserved 0, blocking strategy; block-size code (0 reserved; 6 / 7: an 8- / 16-bit
//                  "size - 1" trailer), rate code (15 invalid; 12 kHz, 13 Hz, 14 tens of Hz in a trailer), channel assignment (0-7
//                  independent, 8 left/side, 9 side/right, 10 mid/side, above reserved), sample-size code (3, 7 reserved), reserved 0,
//                  the UTF-8 style coded number (1..7 bytes, up to 36 bits), the trailers, CRC-8 (x^8 + x^2 + x + 1) of all of it.
//   subframe       pad bit 0, type (0 CONSTANT, 1 VERBATIM, 8..12 FIXED 0..4, 32..63 LPC 1..32, the rest reserved), wasted-bits flag
//                  and unary count; LPC: precision - 1 (15 invalid), shift (5 bits signed; negative is refused), coefficients.
//   residual       method (0 RICE 4-bit parameters, 1 RICE2 5-bit, the rest reserved), partition order; a parameter of all ones is an
//                  escape: 5 bits of width, then raw signed residuals (width 0: zeros).
//   frame end      zero bits up to a byte boundary (non-zero bits fail the frame), CRC-16 (x^16 + x^15 + x^2 + 1) of the whole frame.
// A sample is what the mathematics gives, computed in 64 bits and kept as its low 32: on a well-formed stream nothing is cut off.
// A residual that does not fit 32 bits, an order above the block size, a partition that is not a whole share of the block, wasted
// bits that leave no sample bits are all refused.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FLAC_HD __host__ __device__ inline
#else
#define FLAC_HD inline
#endif

namespace flaccore {

struct Tables { uint16_t crc16[256]; uint8_t crc8[256]; };

// The tables are generated: entry x is the remainder of x * X^8 (X^16) by the polynomial, most significant bit first.
FLAC_HD void make_tables(Tables* t)
{
    for (uint32_t x = 0; x < 256; x++) {
        uint32_t a = x, b = x << 8;
        for (int k = 0; k < 8; k++) {
            a = (a & 0x80u) ? ((a << 1) ^ 0x07u) & 0xffu : (a << 1) & 0xffu;
            b = (b & 0x8000u) ? ((b << 1) ^ 0x8005u) & 0xffffu : (b << 1) & 0xffffu;
        }
        t->crc8[x] = (uint8_t)a;
        t->crc16[x] = (uint16_t)b;
    }
}

enum { kParseBad = 0, kParseOk = 1, kParseShort = 2 };      // a probe's outcome: SHORT = the range ended first ("need more")
enum { kSubConstant = 0, kSubVerbatim = 1, kSubFixed = 2, kSubLpc = 3 };
enum { kStatusOk = 0, kStatusCorrupt = 1, kStatusUnsupported = 2, kStatusOverflow = 3 };   // OHGPU_FLAC_*
enum { kMaxChannels = 8, kMaxOrder = 32 };

// Bytes [p, p + n) most significant bit first.  A byte is fetched only when a bit of it is asked for, and every fetched byte goes
// through both CRCs, so that at a byte boundary `crc16` covers exactly the bytes consumed.
struct BitReader {
    const uint8_t* p;
    const Tables* t;
    uint32_t n, at;          // bytes in the range / fetched so far
    uint64_t acc;            // the low `have` bits are the unread ones
    uint32_t have;
    uint32_t crc16;
    uint32_t crc8;
    bool     dry;            // a read went past the range: every value since is 0
};

FLAC_HD void br_init(BitReader* r, const uint8_t* p, uint32_t n, const Tables* t)
{
    r->p = p; r->t = t; r->n = n; r->at = 0; r->acc = 0; r->have = 0; r->crc16 = 0; r->crc8 = 0; r->dry = false;
}

FLAC_HD bool br_fetch(BitReader* r)
{
    if (r->at >= r->n) { r->dry = true; return false; }
    const uint32_t b = r->p[r->at++];
    r->crc16 = ((r->crc16 << 8) & 0xffffu) ^ r->t->crc16[((r->crc16 >> 8) ^ b) & 0xffu];
    r->crc8 = r->t->crc8[(r->crc8 ^ b) & 0xffu];
    r->acc = (r->acc << 8) | b;
    r->have += 8;
    return true;
}

FLAC_HD uint32_t br_bits(BitReader* r, uint32_t k)          // k <= 32
{
    if (k == 0) return 0;
    while (r->have < k) if (!br_fetch(r)) return 0;
    r->have -= k;
    return (uint32_t)((r->acc >> r->have) & ((1ull << k) - 1ull));
}

FLAC_HD int32_t br_signed(BitReader* r, uint32_t k)         // k <= 32; k == 0 reads nothing and is 0
{
    if (k == 0) return 0;
    const uint32_t v = br_bits(r, k);
    const uint32_t sign = 1u << (k - 1);
    return (int32_t)((v ^ sign) - sign);
}

FLAC_HD uint32_t br_unary(BitReader* r)                      // zeros in front of the next one bit (which is consumed)
{
    uint32_t q = 0;
    for (;;) {
        if (r->have == 0 && !br_fetch(r)) return 0;
        const uint64_t v = r->acc & ((1ull << r->have) - 1ull);
        if (v == 0) { q += r->have; r->have = 0; continue; }
        const uint32_t top = 63u - (uint32_t)__builtin_clzll(v);   // position of the first one among the unread bits
        q += r->have - 1u - top;
        r->have = top;
        return q;
    }
}

struct Header {
    uint64_t number;         // frame number (fixed blocking) or first sample number (variable)
    uint32_t blocksize, rate;
    uint8_t  channels, bits, assignment, variable;
    uint32_t bytes;          // the header's length, CRC-8 included
};

struct Sub {                 // one channel of one frame: 80 bytes
    uint8_t  type, order, shift, wasted;
    int32_t  constant;
    int16_t  coef[kMaxOrder];
    uint8_t  pad[8];
};

// What a stream's frames must be (its descriptor's STREAMINFO fields): header codes of "as STREAMINFO says" take them from here.
struct StreamCfg { uint32_t channels, bits, sample_rate, max_blocksize; };

// Header at r's start.  Ok: every code legal, number well formed, CRC-8 right.  Short: the range ended before that could be told.
FLAC_HD int parse_header(BitReader* r, const StreamCfg& cfg, Header* h)
{
    const uint32_t sync = br_bits(r, 15);
    if (r->dry) return (r->n == 0 || r->p[0] == 0xffu) ? kParseShort : kParseBad;      // (fewer than two bytes)
    if (sync != 0x7ffcu) return kParseBad;
    h->variable = (uint8_t)br_bits(r, 1);
    const uint32_t bs_code = br_bits(r, 4), rate_code = br_bits(r, 4), asg = br_bits(r, 4), size_code = br_bits(r, 3), rsv = br_bits(r, 1);
    if (r->dry) return kParseShort;
    if (bs_code == 0 || rate_code == 15 || asg > 10 || size_code == 3 || size_code == 7 || rsv != 0) return kParseBad;
    // the coded number: the first byte's leading ones give the length
    const uint32_t lead = br_bits(r, 8);
    if (r->dry) return kParseShort;
    uint32_t extra = 0;
    uint64_t v = 0;
    if (lead < 0x80u) v = lead;
    else if (lead < 0xc0u) return kParseBad;
    else if (lead < 0xe0u) { extra = 1; v = lead & 0x1fu; }
    else if (lead < 0xf0u) { extra = 2; v = lead & 0x0fu; }
    else if (lead < 0xf8u) { extra = 3; v = lead & 0x07u; }
    else if (lead < 0xfcu) { extra = 4; v = lead & 0x03u; }
    else if (lead < 0xfeu) { extra = 5; v = lead & 0x01u; }
    else if (lead == 0xfeu) { extra = 6; v = 0; }
    else return kParseBad;
    for (uint32_t k = 0; k < extra; k++) {
        const uint32_t c = br_bits(r, 8);
        if (r->dry) return kParseShort;
        if ((c & 0xc0u) != 0x80u) return kParseBad;
        v = (v << 6) | (c & 0x3fu);
    }
    h->number = v;
    uint32_t bs = 0;
    if (bs_code == 1) bs = 192;
    else if (bs_code <= 5) bs = 576u << (bs_code - 2);
    else if (bs_code == 6) bs = br_bits(r, 8) + 1;
    else if (bs_code == 7) bs = br_bits(r, 16) + 1;
    else bs = 256u << (bs_code - 8);
    uint32_t rate = 0;
    switch (rate_code) {
    case 0: rate = cfg.sample_rate; break;
    case 1: rate = 88200; break;   case 2: rate = 176400; break;  case 3: rate = 192000; break;
    case 4: rate = 8000; break;    case 5: rate = 16000; break;   case 6: rate = 22050; break;
    case 7: rate = 24000; break;   case 8: rate = 32000; break;   case 9: rate = 44100; break;
    case 10: rate = 48000; break;  case 11: rate = 96000; break;
    case 12: rate = br_bits(r, 8) * 1000u; break;
    case 13: rate = br_bits(r, 16); break;
    default: rate = br_bits(r, 16) * 10u; break;
    }
    const uint32_t crc_before = r->crc8;
    const uint32_t crc = br_bits(r, 8);
    if (r->dry) return kParseShort;
    if (crc != crc_before) return kParseBad;
    h->blocksize = bs;
    h->rate = rate;
    h->assignment = (uint8_t)asg;
    h->channels = (uint8_t)(asg < 8 ? asg + 1 : 2);
    const uint32_t sizes[8] = {0, 8, 12, 0, 16, 20, 24, 0};
    h->bits = (uint8_t)(size_code == 0 ? cfg.bits : sizes[size_code]);
    h->bytes = r->at;
    return kParseOk;
}

// Residuals of one subframe into row[order .. n): kParseOk / kParseBad; a dry reader is the caller's to see.
template <bool kStore>
FLAC_HD int parse_residual(BitReader* r, uint32_t n, uint32_t order, int32_t* row)
{
    const uint32_t method = br_bits(r, 2);
    if (method > 1) return r->dry ? kParseOk : kParseBad;
    const uint32_t pbits = method == 0 ? 4u : 5u, escape = (1u << pbits) - 1u;
    const uint32_t po = br_bits(r, 4);
    if (r->dry) return kParseOk;
    const uint32_t share = n >> po;
    if (po > 0 && ((share << po) != n || share < order)) return kParseBad;
    if (order > n) return kParseBad;
    uint32_t i = order;
    for (uint32_t part = 0; part < (1u << po); part++) {
        const uint32_t count = (po == 0) ? n - order : (part == 0 ? share - order : share);
        const uint32_t k = br_bits(r, pbits);
        if (r->dry) return kParseOk;
        if (k == escape) {
            const uint32_t width = br_bits(r, 5);
            for (uint32_t j = 0; j < count; j++, i++) {
                const int32_t v = br_signed(r, width);
                if (r->dry) return kParseOk;
                if (kStore) row[i] = v;
            }
        } else {
            for (uint32_t j = 0; j < count; j++, i++) {
                const uint64_t q = br_unary(r);
                const uint64_t u = (q << k) | br_bits(r, k);
                if (r->dry) return kParseOk;
                if (u > 0xffffffffull) return kParseBad;
                if (kStore) row[i] = (int32_t)((uint32_t)(u >> 1) ^ (0u - (uint32_t)(u & 1u)));
            }
        }
    }
    return kParseOk;
}

// One subframe of `bps` bits a sample: the record, and in row[0 .. n) the verbatim samples / the warm-up samples then the residuals.
template <bool kStore>
FLAC_HD int parse_subframe(BitReader* r, uint32_t n, uint32_t bps, Sub* s, int32_t* row)
{
    const uint32_t head = br_bits(r, 8);
    if (r->dry) return kParseOk;
    if (head & 0x80u) return kParseBad;
    const uint32_t type = (head >> 1) & 0x3fu;
    uint32_t wasted = 0;
    if (head & 1u) {
        wasted = br_unary(r) + 1;
        if (r->dry) return kParseOk;
        if (wasted >= bps) return kParseBad;
        bps -= wasted;
    }
    s->wasted = (uint8_t)wasted;
    s->order = 0; s->shift = 0; s->constant = 0;
    if (type == 0) {
        s->type = kSubConstant;
        s->constant = br_signed(r, bps);
        return kParseOk;
    }
    if (type == 1) {
        s->type = kSubVerbatim;
        for (uint32_t i = 0; i < n; i++) {
            const int32_t v = br_signed(r, bps);
            if (r->dry) return kParseOk;
            if (kStore) row[i] = v;
        }
        return kParseOk;
    }
    uint32_t order;
    if (type >= 8 && type <= 12) { s->type = kSubFixed; order = type - 8; }
    else if (type >= 32) { s->type = kSubLpc; order = type - 31; }
    else return kParseBad;
    if (order > n) return kParseBad;
    s->order = (uint8_t)order;
    for (uint32_t i = 0; i < order; i++) {
        const int32_t v = br_signed(r, bps);
        if (r->dry) return kParseOk;
        if (kStore) row[i] = v;
    }
    if (s->type == kSubLpc) {
        const uint32_t prec = br_bits(r, 4) + 1;
        const int32_t shift = br_signed(r, 5);
        if (r->dry) return kParseOk;
        if (prec == 16 || shift < 0) return kParseBad;
        s->shift = (uint8_t)shift;
        for (uint32_t j = 0; j < order; j++) s->coef[j] = (int16_t)br_signed(r, prec);
        if (r->dry) return kParseOk;
    }
    return parse_residual<kStore>(r, n, order, row);
}

// A whole frame at p: header, subframes, padding, CRC-16.  rows: channel c's row is rows + c * row_stride (kStore only; at least
// cfg.max_blocksize long, which bounds every store since a larger block fails first).  *end = the frame's length in bytes.
template <bool kStore>
FLAC_HD int parse_frame(const uint8_t* p, uint32_t n, const Tables* t, const StreamCfg& cfg, Header* h, Sub* subs, int32_t* rows,
                        uint32_t row_stride, uint32_t* end)
{
    BitReader r;
    br_init(&r, p, n, t);
    const int hs = parse_header(&r, cfg, h);
    if (hs != kParseOk) return hs;
    // (the stream's channel count bounds a candidate's scratch: a frame of another count is no frame of this stream)
    if (h->blocksize > cfg.max_blocksize || h->channels != cfg.channels) return kParseBad;
    for (uint32_t c = 0; c < h->channels; c++) {
        const bool side = (h->assignment == 8 && c == 1) || (h->assignment == 9 && c == 0) || (h->assignment == 10 && c == 1);
        Sub scratch;
        Sub* s = subs ? subs + c : &scratch;
        const int st = parse_subframe<kStore>(&r, h->blocksize, h->bits + (side ? 1u : 0u), s, kStore ? rows + (uint64_t)c * row_stride : nullptr);
        if (r.dry) return kParseShort;
        if (st != kParseOk) return st;
    }
    if ((r.have & 7u) != 0 && br_bits(&r, r.have & 7u) != 0) return kParseBad;
    const uint32_t crc_before = r.crc16;
    const uint32_t crc = br_bits(&r, 16);
    if (r.dry) return kParseShort;
    if (crc != crc_before) return kParseBad;
    *end = r.at;
    return kParseOk;
}

// Residuals -> samples in place: the predictor recurrence in 64 bits, then the wasted-bits shift.
FLAC_HD void restore_channel(const Sub& s, int32_t* row, uint32_t n)
{
    if (s.type == kSubConstant) {
        for (uint32_t i = 0; i < n; i++) row[i] = s.constant;
    } else if (s.type == kSubFixed) {
        for (uint32_t i = s.order; i < n; i++) {
            int64_t pred = 0;
            switch (s.order) {
            case 1: pred = (int64_t)row[i - 1]; break;
            case 2: pred = 2 * (int64_t)row[i - 1] - (int64_t)row[i - 2]; break;
            case 3: pred = 3 * (int64_t)row[i - 1] - 3 * (int64_t)row[i - 2] + (int64_t)row[i - 3]; break;
            case 4: pred = 4 * (int64_t)row[i - 1] - 6 * (int64_t)row[i - 2] + 4 * (int64_t)row[i - 3] - (int64_t)row[i - 4]; break;
            default: break;
            }
            row[i] = (int32_t)(uint32_t)(uint64_t)((int64_t)row[i] + pred);
        }
    } else if (s.type == kSubLpc) {
        for (uint32_t i = s.order; i < n; i++) {
            int64_t sum = 0;
            for (uint32_t j = 0; j < s.order; j++) sum += (int64_t)s.coef[j] * (int64_t)row[i - 1 - j];
            row[i] = (int32_t)(uint32_t)(uint64_t)((int64_t)row[i] + (sum >> s.shift));
        }
    }
    if (s.wasted) for (uint32_t i = 0; i < n; i++) row[i] = (int32_t)((uint32_t)row[i] << s.wasted);
}

// The two channels of a stereo frame from its two coded ones.
FLAC_HD void decorrelate(uint32_t assignment, int32_t a, int32_t b, int32_t* left, int32_t* right)
{
    if (assignment == 8) { *left = a; *right = (int32_t)(uint32_t)(uint64_t)((int64_t)a - (int64_t)b); }
    else if (assignment == 9) { *left = (int32_t)(uint32_t)(uint64_t)((int64_t)a + (int64_t)b); *right = b; }
    else if (assignment == 10) {
        const int64_t mid = (int64_t)((uint64_t)(int64_t)a << 1) | (int64_t)(b & 1), side = b;
        *left = (int32_t)(uint32_t)(uint64_t)((mid + side) >> 1);
        *right = (int32_t)(uint32_t)(uint64_t)((mid - side) >> 1);
    } else { *left = a; *right = b; }
}

// ---- scan, probe records, chain ----
struct Stream {              // a descriptor as the device sees it: 64 bytes
    uint64_t src_offset, dst_offset, dst_plane_stride, first_sample;
    uint32_t src_bytes, max_samples;
    uint32_t sample_rate, blocksize, max_blocksize;
    uint8_t  channels, bits, flags, pad;
    uint32_t cand_first, cand_count;     // its candidates in the sorted list
};
enum { kFlagAtFrame = 1, kFlagPackedBe = 2 };

struct Probe {               // one candidate: 56 bytes
    uint32_t stream, pos;    // position within the stream's range
    uint32_t state;          // kParse* of the whole frame
    uint32_t end;            // pos + the frame's length; of a short one: 1 when its header was whole, 0 when the range cut that too
    uint64_t number;
    uint32_t blocksize, rate;
    uint8_t  channels, bits, assignment, variable;
    uint32_t accepted;       // the chain's mark
    int64_t  place;          // first sample's index in the stream's output
    uint32_t row0, pad;      // its first row of scratch (one row per channel of its stream)
};

struct Result {              // ohgpu_flac_stream_result: 48 bytes
    uint32_t status, frames;
    uint64_t samples, first_sample_decoded, bytes_consumed;
    uint32_t candidates, candidates_rejected;
    uint64_t reserved;
};

FLAC_HD StreamCfg cfg_of(const Stream& s) { StreamCfg c; c.channels = s.channels; c.bits = s.bits; c.sample_rate = s.sample_rate; c.max_blocksize = s.max_blocksize; return c; }

// Is there a candidate at p (n bytes to the range's end)?  kParseShort: as far as the range goes it could be one.
FLAC_HD int scan_position(const uint8_t* p, uint32_t n, const Tables* t, const StreamCfg& cfg)
{
    if (n == 0 || p[0] != 0xffu) return kParseBad;
    if (n == 1) return kParseShort;
    if ((p[1] & 0xfeu) != 0xf8u) return kParseBad;
    BitReader r;
    br_init(&r, p, n < 16u ? n : 16u, t);
    Header h;
    return parse_header(&r, cfg, &h);
}

// One stream's chain over its candidates c[0 .. n), sorted by position, each probed.  Marks the accepted ones and their places.
FLAC_HD void chain_stream(const Stream& s, Probe* c, uint32_t n, Result* out)
{
    Result res;
    res.status = kStatusOk; res.frames = 0; res.samples = 0; res.first_sample_decoded = 0; res.bytes_consumed = s.src_bytes;
    res.candidates = 0; res.candidates_rejected = 0; res.reserved = 0;
    uint32_t first = n, lowest_open = n;
    for (uint32_t i = 0; i < n; i++) {
        c[i].accepted = 0;
        if (c[i].state != kParseShort || c[i].end != 0) res.candidates++;      // (end == 0 marks a header the range cut short)
        if (c[i].state == kParseShort && lowest_open == n) lowest_open = i;
        if (c[i].state == kParseOk && first == n) first = i;
    }
    if (s.flags & kFlagAtFrame) {
        // the first frame is at the range's start or nowhere
        if (n == 0 || c[0].pos != 0 || c[0].state == kParseBad) { first = n; lowest_open = n; res.status = s.src_bytes ? (uint32_t)kStatusCorrupt : (uint32_t)kStatusOk; res.bytes_consumed = 0; }
        else if (c[0].state == kParseShort) { first = n; lowest_open = 0; }
        else first = 0;
    }
    if (first == n) {
        if (lowest_open != n) res.bytes_consumed = c[lowest_open].pos;
        res.candidates_rejected = res.candidates;
        *out = res;
        return;
    }
    uint32_t stream_bs = s.blocksize ? s.blocksize : c[first].blocksize;
    uint32_t i = first;
    uint64_t expect = 0;
    for (;;) {
        Probe& f = c[i];
        // what a frame of this stream must be
        if (f.bits != 8 && f.bits != 16 && f.bits != 24) { res.status = kStatusUnsupported; res.bytes_consumed = f.pos; break; }
        bool fits = f.channels == s.channels && f.bits == s.bits && f.rate == s.sample_rate && f.variable == c[first].variable;
        if (fits && !f.variable && f.blocksize > stream_bs) fits = false;
        if (fits && i != first && f.number != expect) fits = false;
        if (!fits) { res.status = kStatusCorrupt; res.bytes_consumed = f.pos; break; }
        const uint64_t first_sample = f.variable ? f.number : f.number * (uint64_t)stream_bs;
        if (first_sample < s.first_sample || first_sample - s.first_sample + f.blocksize > (uint64_t)s.max_samples) {
            res.status = kStatusOverflow; res.bytes_consumed = f.pos; break;
        }
        f.accepted = 1;
        f.place = (int64_t)(first_sample - s.first_sample);
        if (res.frames == 0) res.first_sample_decoded = first_sample;
        res.frames++;
        res.samples += f.blocksize;
        res.bytes_consumed = f.end;
        expect = f.variable ? f.number + f.blocksize : f.number + 1;
        if (f.end >= s.src_bytes) break;
        // the next frame starts where this one ends: find the candidate there
        uint32_t lo = i + 1, hi = n;
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (c[mid].pos < f.end) lo = mid + 1; else hi = mid; }
        if (lo == n || c[lo].pos != f.end || c[lo].state == kParseBad) { res.status = kStatusCorrupt; break; }
        if (c[lo].state == kParseShort) break;
        i = lo;
    }
    res.candidates_rejected = res.candidates - res.frames;
    *out = res;
}

// An accepted frame's samples to the destination: sample i of channel ch, decorrelated (v[] holds the channels' restored values).
FLAC_HD void store_sample(const Stream& s, uint8_t* dst, uint64_t index, uint32_t ch, int32_t v)
{
    if (s.flags & kFlagPackedBe) {
        const uint32_t bytes = s.bits / 8u;
        uint8_t* q = dst + s.dst_offset + (index * s.channels + ch) * bytes;
        for (uint32_t b = 0; b < bytes; b++) q[b] = (uint8_t)((uint32_t)v >> (8u * (bytes - 1u - b)));
    } else {
        *(int32_t*)(dst + s.dst_offset + (uint64_t)ch * s.dst_plane_stride + index * 4u) = v;
    }
}

}  // namespace flaccore
