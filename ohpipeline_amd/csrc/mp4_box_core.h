// mp4_box_core.h -- the MPEG-4 (ISO base media, ISO/IEC 14496-12) container in front of the Apple Lossless decoder:
// what stands between the bytes of an .m4a file and the packet table ohgpu_alac_* takes.  Every function is __host__ __device__:
// csrc/mp4_table_kernel.hip runs this text on the device, tests/cpp/mp4_core_driver.cpp runs the same text on the CPU under the
// sanitizers, csrc/api_mp4.hip runs it for ohgpu_mp4_seek.  Everything in the file is big-endian and lies at any address: the host reads
// it byte by byte, the device as aligned dwords (csrc/field_bytes.h).
//
//   a box      u32 size | fourcc | (size == 1: u64 size) | payload.  Size 0: to the end of the stream, at top level only.  A size below
//              its own header (8 or 16) is INVALID; so is a child that ends behind its parent.  Fewer than 8 bytes left in a parent are
//              slack and end it.
//   the walk   one pass in file order, at most kMaxBoxes headers; the first thing wrong gives the status and error_offset (the box).
//              top level: "ftyp" at bytes 4..8 or NOT_MP4 (fewer than 8 bytes: TRUNCATED); `moof` is UNSUPPORTED; the first `mdat` is
//              recorded; the first `moov` is entered (it reaches past the stream: TRUNCATED); every other box is skipped by its size,
//              and a box that reaches past the stream ends the walk.  No `moov` by then: TRUNCATED.
//              moov: `mvex` is UNSUPPORTED; a `trak` is entered until one has been taken.  trak > mdia > { mdhd, minf > stbl >
//              { stsd, stts, stsc, stsz, stco | co64 } }, the first of each kind counts, `stz2` is UNSUPPORTED.  Everything else is
//              skipped by its size.
//   a trak     is taken at its end when its first sample entry is `alac`; then its tables are held to the rules of finish_track().
//              The end of `moov` without one: NOT_ALAC, with the first trak's entry fourcc.
//   expansion  rows [0, min(N, packet_capacity)): include/ohgpu.h's MPEG-4 section has the arithmetic.  expand_serial() walks the
//              samples with running sums (the plain route, ohgpu_mp4_seek's tables); the fused route scans (tile sums, carries of
//              tiles / stsc runs / stts runs) and row_for() searches the carries.  Both end in emit_row().
#pragma once

#include <stdint.h>

#include "field_bytes.h"

#if defined(__HIPCC__)
#define MP4B_HD __host__ __device__ __forceinline__
#else
#define MP4B_HD inline
#endif
// the CPU driver counts loop trips through this (kind 0: a box header, 1: a table entry, 2: a sample, 3: a search step)
#ifndef MP4B_STEP
#define MP4B_STEP(kind)
#endif

namespace mp4box {

enum Status : uint32_t { kOk = 0, kNotMp4 = 1, kTruncated = 2, kInvalid = 3, kNotAlac = 4, kUnsupported = 5 };
constexpr uint32_t kMaxSamples = 1u << 24, kMaxBoxes = 4096, kNone = 0xffffffffu;
constexpr uint32_t kTile = 1024;                      // samples a tile: one workgroup's share of the sums and of the expansion
using fieldbytes::fourcc;

struct Stream {               // 32 bytes = ohgpu_mp4_stream_desc
    uint64_t src_offset;
    uint32_t src_bytes, flags, packet_first, packet_capacity;
    uint32_t reserved[2];
};
struct Config {               // 24 bytes = ohgpu_alac_config
    uint32_t frame_length;
    uint8_t  compatible_version, bit_depth, pb, mb, kb, channels;
    uint16_t max_run;
    uint32_t max_frame_bytes, avg_bit_rate, sample_rate;
};
struct Result {               // 112 bytes = ohgpu_mp4_stream_result
    uint32_t status, codec;
    Config   config;
    uint32_t timescale, entry_rate;
    uint64_t duration, frames;
    uint32_t samples, chunks, samples_available, samples_refused, first_bad_sample;
    uint16_t entry_channels, entry_bits;
    uint64_t moov_offset, mdat_offset, mdat_bytes, error_offset;
};
struct Sample { uint64_t first_frame; uint32_t frames, chunk; };      // 16 bytes = ohgpu_mp4_sample
struct Row { uint64_t src_offset; uint32_t bytes, reserved; };        // 16 bytes = ohgpu_alac_packet
// Where the walk found the taken trak's tables (positions of their first entries, from the stream's first byte), for the expansion.
struct Tables {
    uint32_t rows;            // min(N, packet_capacity) of a stream whose status is OK, else 0: the rows the expansion writes
    uint32_t n_samples, uniform_size, stsz_pos;
    uint32_t stsc_pos, stsc_entries, stsc_used;       // used: the entries a row < rows can lie in (S_k >= k: min(entries, rows))
    uint32_t stts_pos, stts_entries, stts_used;
    uint32_t co_pos, n_chunks, co64, pad;
    uint64_t packet_limit;    // frame_length x channels x 5 + 64
};
static_assert(sizeof(Stream) == 32 && sizeof(Config) == 24 && sizeof(Result) == 112 && sizeof(Sample) == 16 && sizeof(Row) == 16 && sizeof(Tables) == 64, "MPEG-4 layouts");

// ---- bytes: csrc/field_bytes.h's reader, aligned dwords on the device
using fieldbytes::be16;
using fieldbytes::be32;
using fieldbytes::be64;

struct Box { uint64_t size; uint32_t type, header; };
// The header at pos of [pos, limit).  1: read; 0: fewer than 8 bytes are left; 2: a 64-bit size is announced and fewer than 16 are;
// -1: a size below the header's, or size 0 below top level.
MP4B_HD int read_box(const uint8_t* p, uint64_t pos, uint64_t limit, bool top, Box* out)
{
    if (limit - pos < 8u) return 0;
    const uint32_t size32 = be32(p, pos);
    const uint32_t type = be32(p, pos + 4);
    uint64_t size = size32;
    uint32_t header = 8;
    if (size32 == 1u) {
        if (limit - pos < 16u) return 2;
        size = be64(p, pos + 8);
        header = 16;
    } else if (size32 == 0u) {
        if (!top) return -1;
        size = limit - pos;
    }
    out->size = size; out->type = type; out->header = header;
    return size < header ? -1 : 1;
}

// What one trak gave.
struct Track {
    uint32_t codec, have;     // have: bits of kHave*
    uint32_t timescale, channels, bits, rate;
    uint64_t duration;
    Config   cfg;
    Tables   t;
    uint32_t stsc_box, stts_box;
};
enum { kHaveMdhd = 1, kHaveStsd = 2, kHaveStts = 4, kHaveStsc = 8, kHaveStsz = 16, kHaveCo = 32, kHaveAll = 63 };

struct Walk {
    const uint8_t* p;         // the stream's first byte
    uint32_t n;               // its bytes
    uint32_t visited;
    uint64_t err_at;
    Track    tr;

    MP4B_HD uint32_t fail(uint32_t status, uint64_t at) { err_at = at; return status; }
    MP4B_HD bool visit() { MP4B_STEP(0); return ++visited <= kMaxBoxes; }

    // a full box of a table: version 0 and an entry count at `count_at` of the payload that fits it
    MP4B_HD bool table_head(uint64_t pay, uint64_t len, uint32_t fixed, uint32_t entry_bytes, uint32_t* entries)
    {
        if (len < fixed || p[pay] != 0) return false;
        *entries = be32(p, pay + fixed - 4u);
        return *entries <= (len - fixed) / entry_bytes;
    }

    MP4B_HD uint32_t mdhd(uint64_t box, uint64_t pay, uint64_t len)
    {
        if (len < 4u) return fail(kInvalid, box);
        const uint32_t version = p[pay];
        if (version == 0u) {
            if (len < 20u) return fail(kInvalid, box);
            tr.timescale = be32(p, pay + 12); tr.duration = be32(p, pay + 16);
        } else if (version == 1u) {
            if (len < 32u) return fail(kInvalid, box);
            tr.timescale = be32(p, pay + 20); tr.duration = be64(p, pay + 24);
        } else return fail(kInvalid, box);
        if (tr.timescale == 0u) return fail(kInvalid, box);
        return kOk;
    }

    // The inner `alac` box of a sample entry (at c, its header read into k): the configuration and the packet limit.
    MP4B_HD uint32_t alac_box(uint64_t c, const Box& k)
    {
        const uint64_t a = c + k.header;
        if (k.size - k.header < 28u) return fail(kUnsupported, c);
        const uint32_t w8 = be32(p, a + 8), w12 = be32(p, a + 12);   // (the six one-byte fields and max_run, as two words)
        if (w8 >> 24) return fail(kUnsupported, c);
        Config& g = tr.cfg;
        g.frame_length = be32(p, a + 4);
        g.compatible_version = (uint8_t)(w8 >> 24); g.bit_depth = (uint8_t)(w8 >> 16); g.pb = (uint8_t)(w8 >> 8); g.mb = (uint8_t)w8;
        g.kb = (uint8_t)(w12 >> 24); g.channels = (uint8_t)(w12 >> 16);
        g.max_run = (uint16_t)w12;
        g.max_frame_bytes = be32(p, a + 16); g.avg_bit_rate = be32(p, a + 20); g.sample_rate = be32(p, a + 24);
        // what ohgpu_alac_batch_check would refuse is refused here, where it costs one stream and not the batch
        const bool depth_ok = g.bit_depth == 16 || g.bit_depth == 20 || g.bit_depth == 24 || g.bit_depth == 32;
        if (g.channels < 1 || g.channels > 8 || g.frame_length < 1 || g.frame_length > 16384u || !depth_ok) return fail(kUnsupported, c);
        tr.t.packet_limit = (uint64_t)g.frame_length * g.channels * 5u + 64u;
        return kOk;
    }

    MP4B_HD uint32_t stsd(uint64_t box, uint64_t pay, uint64_t len)
    {
        uint32_t count;
        if (!table_head(pay, len, 8, 1, &count)) return fail(kInvalid, box);      // (an entry is 8 bytes at the least: read_box sees to it)
        if (count == 0u) return kOk;
        const uint64_t end = pay + len, entry = pay + 8u;
        Box e;
        if (!visit()) return fail(kInvalid, entry);
        if (read_box(p, entry, end, false, &e) != 1 || e.size > end - entry) return fail(kInvalid, entry);
        tr.codec = e.type;
        if (e.type == fourcc('e', 'n', 'c', 'a')) return fail(kUnsupported, entry);
        if (e.type != fourcc('a', 'l', 'a', 'c')) return kOk;
        const uint64_t q = entry + e.header, entry_end = entry + e.size;
        if (entry_end - q < 28u) return fail(kInvalid, entry);
        tr.channels = be16(p, q + 16); tr.bits = be16(p, q + 18); tr.rate = be16(p, q + 24);
        for (uint64_t c = q + 28u; entry_end - c >= 8u;) {
            Box k;
            if (!visit()) return fail(kInvalid, c);
            if (read_box(p, c, entry_end, false, &k) != 1 || k.size > entry_end - c) return fail(kInvalid, c);
            if (k.type != fourcc('a', 'l', 'a', 'c')) { c += k.size; continue; }
            return alac_box(c, k);
        }
        return fail(kUnsupported, entry);
    }

    MP4B_HD uint32_t leaf(uint32_t type, uint64_t box, uint64_t pay, uint64_t len)
    {
        Tables& t = tr.t;
        if (type == fourcc('s', 't', 'z', '2')) return fail(kUnsupported, box);
        if (type == fourcc('s', 't', 's', 'd') && !(tr.have & kHaveStsd)) { tr.have |= kHaveStsd; return stsd(box, pay, len); }
        if (type == fourcc('s', 't', 't', 's') && !(tr.have & kHaveStts)) {
            tr.have |= kHaveStts; tr.stts_box = (uint32_t)box; t.stts_pos = (uint32_t)pay + 8u;
            if (!table_head(pay, len, 8, 8, &t.stts_entries)) return fail(kInvalid, box);
        } else if (type == fourcc('s', 't', 's', 'c') && !(tr.have & kHaveStsc)) {
            tr.have |= kHaveStsc; tr.stsc_box = (uint32_t)box; t.stsc_pos = (uint32_t)pay + 8u;
            if (!table_head(pay, len, 8, 12, &t.stsc_entries)) return fail(kInvalid, box);
        } else if ((type == fourcc('s', 't', 'c', 'o') || type == fourcc('c', 'o', '6', '4')) && !(tr.have & kHaveCo)) {
            tr.have |= kHaveCo; t.co_pos = (uint32_t)pay + 8u; t.co64 = type == fourcc('c', 'o', '6', '4');
            if (!table_head(pay, len, 8, t.co64 ? 8 : 4, &t.n_chunks)) return fail(kInvalid, box);
        } else if (type == fourcc('s', 't', 's', 'z') && !(tr.have & kHaveStsz)) {
            tr.have |= kHaveStsz; t.stsz_pos = (uint32_t)pay + 12u;
            if (len < 12u || p[pay] != 0) return fail(kInvalid, box);
            t.uniform_size = be32(p, pay + 4); t.n_samples = be32(p, pay + 8);
            if (t.uniform_size == 0u && t.n_samples > (len - 12u) / 4u) return fail(kInvalid, box);
            if (t.n_samples > kMaxSamples) return fail(kUnsupported, box);
        }
        return kOk;
    }

    // The taken trak's tables against each other.  *frames: the sum of stts over the N samples.
    MP4B_HD uint32_t finish_track(uint64_t trak, uint64_t* frames)
    {
        const Tables& t = tr.t;
        if (tr.have != kHaveAll) return fail(kInvalid, trak);
        uint64_t covered = 0;
        uint32_t last_fc = 0;
        for (uint32_t k = 0; k < t.stsc_entries; k++) {
            MP4B_STEP(1);
            const uint64_t at = t.stsc_pos + 12ull * k;
            const uint32_t fc = be32(p, at), spc = be32(p, at + 4);
            if (k == 0 ? fc != 1u : fc <= last_fc) return fail(kInvalid, tr.stsc_box);
            if (fc > t.n_chunks || spc < 1u) return fail(kInvalid, tr.stsc_box);
            if (k) covered += (uint64_t)(fc - last_fc) * be32(p, at - 8);
            last_fc = fc;
            if (k + 1u == t.stsc_entries) covered += (uint64_t)(t.n_chunks + 1u - fc) * spc;
        }
        if (covered < t.n_samples) return fail(kInvalid, tr.stsc_box);
        uint64_t counted = 0, sum = 0;
        for (uint32_t m = 0; m < t.stts_entries && counted < t.n_samples; m++) {
            MP4B_STEP(1);
            const uint64_t at = t.stts_pos + 8ull * m, count = be32(p, at), left = t.n_samples - counted;
            if (count == 0u) return fail(kInvalid, tr.stts_box);      // (a run of no samples: the carries' search wants runs that advance)
            sum += (count < left ? count : left) * be32(p, at + 4);
            counted += count;
        }
        if (counted < t.n_samples) return fail(kInvalid, tr.stts_box);
        *frames = sum;
        return kOk;
    }

    MP4B_HD uint32_t run(const Stream& s, Result* out, Tables* tab)
    {
        // the levels: the stream itself, then the containers of the path; start[] / end[] of the level the walk stands in
        enum { kTop = 0, kMoov = 1, kTrak = 2, kMdia = 3, kMinf = 4, kStbl = 5, kLevels = 6 };
        if (n < 8u) return fail(kTruncated, 0);
        if (be32(p, 4) != fourcc('f', 't', 'y', 'p')) return fail(kNotMp4, 0);
        uint64_t start[kLevels] = {}, end[kLevels] = {}, pos = 0;
        uint32_t depth = kTop;
        end[kTop] = n;
        bool moov_seen = false, mdat_seen = false, taken = false, any_trak = false;
        for (;;) {
            const bool top = depth == kTop;
            const uint64_t limit = end[depth];
            Box b;
            const int got = read_box(p, pos, limit, top, &b);
            if (got == 0 || (got == 2 && top)) {                      // this level ends here
                if (top) break;
                pos = limit;
                if (depth == kTrak) {
                    if (!any_trak) { any_trak = true; out->codec = tr.codec; }
                    if (tr.codec == fourcc('a', 'l', 'a', 'c')) {
                        uint64_t frames = 0;
                        const uint32_t st = finish_track(start[kTrak], &frames);
                        if (st != kOk) return st;
                        taken = true;
                        out->frames = frames;
                    }
                }
                if (depth == kMoov && !taken) return fail(kNotAlac, start[kMoov]);
                depth--;
                continue;
            }
            if (!visit()) return fail(kInvalid, pos);
            if (got != 1) return fail(kInvalid, pos);
            const bool fits = b.size <= limit - pos;
            bool enter = false;
            if (top) {
                if (b.type == fourcc('m', 'o', 'o', 'f')) return fail(kUnsupported, pos);
                if (b.type == fourcc('m', 'd', 'a', 't') && !mdat_seen) { mdat_seen = true; out->mdat_offset = pos; out->mdat_bytes = b.size - b.header; }
                if (b.type == fourcc('m', 'o', 'o', 'v') && !moov_seen) {
                    if (!fits) return fail(kTruncated, pos);
                    moov_seen = true; out->moov_offset = pos;
                    enter = true;
                } else if (!fits) break;
            } else {
                if (!fits) return fail(kInvalid, pos);
                if (depth == kMoov && b.type == fourcc('m', 'v', 'e', 'x')) return fail(kUnsupported, pos);
                const uint32_t inner = depth == kMoov ? fourcc('t', 'r', 'a', 'k') : depth == kTrak ? fourcc('m', 'd', 'i', 'a')
                                     : depth == kMdia ? fourcc('m', 'i', 'n', 'f') : depth == kMinf ? fourcc('s', 't', 'b', 'l') : 0u;
                enter = depth < kStbl && b.type == inner && !(depth == kMoov && taken);
                if (enter && depth == kMoov) { Track fresh = {}; tr = fresh; }
            }
            if (enter) {
                depth++; start[depth] = pos; end[depth] = pos + b.size; pos += b.header;
                continue;
            }
            uint32_t st = kOk;
            if (depth == kMdia && b.type == fourcc('m', 'd', 'h', 'd') && !(tr.have & kHaveMdhd)) { tr.have |= kHaveMdhd; st = mdhd(pos, pos + b.header, b.size - b.header); }
            else if (depth == kStbl) st = leaf(b.type, pos, pos + b.header, b.size - b.header);
            if (st != kOk) return st;
            pos += b.size;
        }
        if (!moov_seen) return fail(kTruncated, pos);
        // (the trak that was taken is still in `tr`: no other was entered behind it)
        Tables& t = tr.t;
        out->codec = tr.codec; out->config = tr.cfg;
        out->timescale = tr.timescale; out->duration = tr.duration;
        out->entry_channels = (uint16_t)tr.channels; out->entry_bits = (uint16_t)tr.bits; out->entry_rate = tr.rate;
        out->samples = t.n_samples; out->chunks = t.n_chunks;
        t.rows = t.n_samples < s.packet_capacity ? t.n_samples : s.packet_capacity;
        t.stsc_used = t.stsc_entries < t.rows ? t.stsc_entries : t.rows;
        t.stts_used = t.stts_entries < t.rows ? t.stts_entries : t.rows;
        *tab = t;
        return kOk;
    }
};

// One stream: the result record (whole: every field is written) and the record of its tables.  `base`: the stream's first byte.
MP4B_HD void walk(const Stream& s, const uint8_t* base, Result* out, Tables* tab)
{
    Result r = {};
    Tables t = {};
    Walk w;
    w.p = base; w.n = s.src_bytes; w.visited = 0; w.err_at = 0;
    Track fresh = {};
    w.tr = fresh;
    const uint32_t status = w.run(s, &r, &t);
    if (status != kOk) {                                              // a refusal says what, where, and (NOT_ALAC) what the first trak holds
        const uint32_t codec = status == kNotAlac ? r.codec : 0u;
        Result none = {};
        r = none;
        Tables no_tables = {};
        t = no_tables;
        r.status = status; r.codec = codec; r.error_offset = w.err_at;
    }
    r.first_bad_sample = kNone;
    *out = r;
    *tab = t;
}

// ---- the expansion
MP4B_HD uint32_t size_at(const uint8_t* p, const Tables& t, uint32_t s) { return t.uniform_size ? t.uniform_size : be32(p, t.stsz_pos + 4ull * s); }
MP4B_HD uint32_t stsc_fc(const uint8_t* p, const Tables& t, uint32_t k) { return be32(p, t.stsc_pos + 12ull * k); }
MP4B_HD uint32_t stsc_spc(const uint8_t* p, const Tables& t, uint32_t k) { return be32(p, t.stsc_pos + 12ull * k + 4u); }
MP4B_HD uint64_t stsc_run_samples(const uint8_t* p, const Tables& t, uint32_t k)      // run_k x spc_k
{
    const uint32_t next = k + 1u < t.stsc_entries ? stsc_fc(p, t, k + 1u) : t.n_chunks + 1u;
    return (uint64_t)(next - stsc_fc(p, t, k)) * stsc_spc(p, t, k);
}
MP4B_HD uint32_t stts_count(const uint8_t* p, const Tables& t, uint32_t m) { return be32(p, t.stts_pos + 8ull * m); }
MP4B_HD uint32_t stts_delta(const uint8_t* p, const Tables& t, uint32_t m) { return be32(p, t.stts_pos + 8ull * m + 4u); }
// The last index of carry[0, n) whose value is <= s.  carry[0] == 0 and n >= 1.
MP4B_HD uint32_t last_at_most(const uint64_t* carry, uint32_t n, uint64_t s)
{
    uint32_t lo = 0, hi = n;                                          // carry[lo] <= s < carry[hi] (carry[n]: infinite)
    while (hi - lo > 1u) {
        MP4B_STEP(3);
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (carry[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}
// Sample s of size `size`, `before` bytes into chunk c, `within` samples into an stts run that began at frame run_frame: both rows.
// true: refused (its bytes leave the stream, or it is larger than an Apple Lossless packet may be).
MP4B_HD bool emit_row(const Stream& st, const uint8_t* p, const Tables& t, uint32_t size, uint64_t before, uint32_t c, uint64_t run_frame, uint64_t within,
                      uint32_t delta, Row* row, Sample* sample)
{
    const uint64_t co = t.co64 ? be64(p, t.co_pos + 8ull * c) : be32(p, t.co_pos + 4ull * c), n = st.src_bytes;
    const bool inside = co <= n && before <= n - co && size <= n - co - before;
    const bool refused = !inside || size > t.packet_limit;
    row->src_offset = st.src_offset + (refused ? 0u : co + before);
    row->bytes = refused ? 0u : size;
    row->reserved = 0;
    sample->first_frame = run_frame + within * delta;
    sample->frames = delta;
    sample->chunk = c;
    return refused;
}
// The fused route's row: sample s through the carries (stsc_carry[k] = S_k, stts_carry[m] = the samples in front of run m, stts_frames[m]
// = the frames in front of it).  prefix(i): the sum of the sizes of the samples in front of sample i, for i = s and i = s - j.
template <typename Prefix>
MP4B_HD bool row_for(const Stream& st, const uint8_t* p, const Tables& t, uint32_t s, const uint64_t* stsc_carry, const uint64_t* stts_carry, const uint64_t* stts_frames,
                     Prefix& prefix, Row* row, Sample* sample)
{
    MP4B_STEP(2);
    const uint32_t k = last_at_most(stsc_carry, t.stsc_used, s), spc = stsc_spc(p, t, k);
    const uint64_t r = s - stsc_carry[k];
    const uint32_t c = stsc_fc(p, t, k) - 1u + (uint32_t)(r / spc), j = (uint32_t)(r % spc);
    const uint32_t m = last_at_most(stts_carry, t.stts_used, s);
    return emit_row(st, p, t, size_at(p, t, s), prefix(s) - prefix(s - j), c, stts_frames[m], s - stts_carry[m], stts_delta(p, t, m), row, sample);
}
// The plain route: every row of one stream with running sums, and the three counts into the result.
MP4B_HD void expand_serial(const Stream& st, const uint8_t* p, const Tables& t, Row* rows, Sample* samples, Result* out)
{
    uint32_t k = 0, m = 0, refused = 0, first_bad = kNone;
    uint64_t run_first = 0, run_samples = 0, stts_first = 0, stts_frame = 0, before = 0;
    uint32_t fc = 0, spc = 1, count = 0, delta = 0;
    if (t.rows) {
        run_samples = stsc_run_samples(p, t, 0); fc = stsc_fc(p, t, 0); spc = stsc_spc(p, t, 0);
        count = stts_count(p, t, 0); delta = stts_delta(p, t, 0);
    }
    for (uint32_t s = 0; s < t.rows; s++) {
        MP4B_STEP(2);
        while (s - run_first >= run_samples) {                        // (S_E >= N: k stays below the entry count)
            MP4B_STEP(1);
            run_first += run_samples; k++;
            run_samples = stsc_run_samples(p, t, k); fc = stsc_fc(p, t, k); spc = stsc_spc(p, t, k);
        }
        while (s - stts_first >= count) {
            MP4B_STEP(1);
            stts_frame += (uint64_t)count * delta; stts_first += count; m++;
            count = stts_count(p, t, m); delta = stts_delta(p, t, m);
        }
        const uint64_t r = s - run_first;
        if (r % spc == 0u) before = 0;
        const uint32_t size = size_at(p, t, s);
        if (emit_row(st, p, t, size, before, fc - 1u + (uint32_t)(r / spc), stts_frame, s - stts_first, delta, &rows[s], &samples[s])) {
            refused++;
            if (first_bad == kNone) first_bad = s;
        }
        before += size;
    }
    out->samples_refused = refused;
    out->first_bad_sample = first_bad;
    out->samples_available = first_bad < t.rows ? first_bad : t.rows;
}
// Host only: the row that holds `frame` in a sample table (ohgpu_mp4_seek): the last row whose first_frame is <= frame.
inline bool seek(const Sample* samples, uint64_t n, uint64_t frame, uint64_t* index)
{
    if (n == 0 || frame >= samples[n - 1].first_frame + samples[n - 1].frames) return false;
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (samples[mid].first_frame <= frame) lo = mid; else hi = mid;
    }
    *index = lo;
    return true;
}

}  // namespace mp4box
