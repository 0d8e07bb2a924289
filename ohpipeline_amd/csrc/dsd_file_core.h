// dsd_file_core.h -- DSF and DFF files in front of the pipeline's DSD format: the chunk walk that finds the format and
// the audio, the record the conversion works from, and the conversion of the audio run at any address.  Every function compiles for the
// host, for the device and for a stand-alone CPU driver: csrc/dsd_file_kernel.hip runs this text on the device, csrc/api_dsd_file.hip
// runs it for ohgpu_dsd_file_head, tests/cpp/dsd_file_core_driver.cpp runs it under the sanitizers.  The rules are written out in
// include/ohgpu.h's DSD file section; this file is their one implementation.
//
//   the walk      DSF: three chunks at fixed places (`DSD ` of 28 bytes, `fmt ` at 28, `data` behind it), little-endian.  DFF: `FRM8`,
//                 then chunks from byte 16 -- id, u64 size, payload, a pad byte behind an odd size --, big-endian; the first `PROP` of
//                 type `SND ` (whose local chunks `FS  `, `CHNL`, `CMPR` are walked the same way) and the first `DSD `, in either
//                 order, after at most kMaxChunks headers, local ones counted.
//   the record    what the conversion needs of a stream: the kind, where the audio lies, the first chunk, how many chunks, and where
//                 the 0x69 fill of a last partial sample block begins and ends.
//   the pieces    the run is cut into pieces of kPieceChunks chunks (a wave's share) and a piece into units of eight chunks (a
//                 lane's).  A unit's source -- sixteen bytes of each DSF plane, or 32 consecutive DFF bytes -- lies at any address:
//                 the aligned 16-byte lines that cover it are joined by a byte funnel and a choice among four dwords, both by the
//                 stream's one phase; DSF dwords are bit-reversed; csrc/dsd_perm.h's selectors make each output dword with one byte
//                 permute.  A unit that crosses into the next DSF plane pair, one whose lines do not lie whole inside the stream, the
//                 last one to seven chunks and every (W, P) with P above 4 go through convert_bytes(), which is also the whole of
//                 the plain route.
#pragma once

#include <stdint.h>

#include "dsd_perm.h"
#include "field_bytes.h"

#if defined(__HIPCC__)
#define DSDF_HD __host__ __device__ __forceinline__
#else
#define DSDF_HD inline
#endif
// the CPU driver counts the walk's chunk headers through this
#ifndef DSDF_STEP
#define DSDF_STEP()
#endif

namespace dsdfile {

enum Status : uint32_t { kOk = 0, kNotDsd = 1, kTruncated = 2, kInvalid = 3, kUnsupported = 4 };
enum Kind : uint32_t { kNoKind = 0, kDsf = 2, kDff = 3 };            // OHGPU_DSD_DSF, OHGPU_DSD_DFF: the packers' kinds
constexpr uint32_t kMaxChunks = 4096, kPieceChunks = 2048, kUnitChunks = 8, kFillByte = 0x69;
constexpr uint32_t kPlane = 4096, kPair = 2 * kPlane, kPairChunks = kPlane / 2;
using fieldbytes::fourcc;

struct Stream {               // 64 bytes = ohgpu_dsd_file_stream_desc
    uint64_t src_offset;
    uint32_t src_bytes, flags;
    uint64_t dst_offset, dst_bytes_capacity, chunk_first;
    uint32_t sample_block_words, pad_bytes_per_chunk;
    uint32_t reserved[4];
};
struct Result {               // 96 bytes = ohgpu_dsd_file_stream_result
    uint32_t status, kind, channels, sample_rate, format_version, channel_type;
    uint64_t sample_count, chunks_total, chunks_available, chunks_written, bytes_written;
    uint64_t data_offset, data_bytes, metadata_offset, error_offset;
};
struct Rec {                  // 48 bytes: the walk's record for the conversion
    uint64_t dst_pos;         // of the destination arena
    uint64_t fill_from, fill_to;   // the 0x69 fill, from dst_pos (equal: none)
    uint32_t kind, pad;       // kDsf / kDff; P
    uint32_t data_offset;     // of the stream: its first audio byte
    uint32_t chunk_first, n;  // chunks [chunk_first, chunk_first + n) of the audio; n == 0: nothing to convert
    uint32_t spare;
};
static_assert(sizeof(Stream) == 64 && sizeof(Result) == 96 && sizeof(Rec) == 48, "DSD file layouts");

// ---- bytes: csrc/field_bytes.h's reader, aligned dwords on the device
using fieldbytes::u8;
using fieldbytes::le32;
using fieldbytes::le64;
using fieldbytes::be16;
using fieldbytes::be32;
using fieldbytes::be64;

struct Found { uint32_t kind, rate, version, channel_type; uint64_t sample_count, chunks_total, data_offset, data_bytes, metadata; };

struct Walk {
    const uint8_t* p;         // the stream's first byte
    uint64_t n;               // its bytes
    uint64_t err_at;
    uint32_t visited;

    DSDF_HD uint32_t fail(uint32_t status, uint64_t at) { err_at = at; return status; }
    DSDF_HD bool holds(uint64_t pos, uint64_t bytes) const { return pos <= n && bytes <= n - pos; }

    DSDF_HD uint32_t dsf(Found* f)
    {
        DSDF_STEP();
        if (!holds(0, 28)) return fail(kTruncated, 0);
        if (le64(p, 4) != 28u || le64(p, 12) == 0u) return fail(kInvalid, 0);
        f->metadata = le64(p, 20);
        const uint64_t fmt = 28;
        DSDF_STEP();
        if (!holds(fmt, 12)) return fail(kTruncated, fmt);
        if (be32(p, fmt) != fourcc('f', 'm', 't', ' ')) return fail(kInvalid, fmt);
        const uint64_t fmt_size = le64(p, fmt + 4);
        if (fmt_size < 52u || fmt_size >= 0x80000000ull) return fail(kInvalid, fmt);
        if (!holds(fmt, 52)) return fail(kTruncated, fmt);
        f->version = le32(p, fmt + 12);
        if (le32(p, fmt + 16) != 0u) return fail(kUnsupported, fmt);           // the format id: 0 is raw DSD
        f->channel_type = le32(p, fmt + 20);
        if (le32(p, fmt + 24) != 2u) return fail(kUnsupported, fmt);
        f->rate = le32(p, fmt + 28);
        if (f->rate == 0u) return fail(kInvalid, fmt);
        if (le32(p, fmt + 32) != 1u) return fail(kUnsupported, fmt);           // bits per sample: 8 would be MSB first
        f->sample_count = le64(p, fmt + 36);
        if (le32(p, fmt + 44) != kPlane) return fail(kUnsupported, fmt);
        const uint64_t data = fmt + fmt_size;
        DSDF_STEP();
        if (!holds(data, 12)) return fail(kTruncated, data);
        if (be32(p, data) != fourcc('d', 'a', 't', 'a')) return fail(kInvalid, data);
        const uint64_t size = le64(p, data + 4);
        if (size < 12u || ((size - 12u) & 1u)) return fail(kInvalid, data);
        if (2u * (f->sample_count / 8u) > size - 12u) return fail(kInvalid, data);
        f->data_offset = data + 12u;
        f->data_bytes = size - 12u;
        f->chunks_total = f->sample_count / 16u;
        return kOk;
    }

    // the local chunks of a `PROP` of `size` bytes whose payload (inside the stream) begins at pay
    DSDF_HD uint32_t prop(uint64_t chunk, uint64_t pay, uint64_t size, Found* f)
    {
        const uint64_t end = pay + size;
        bool have_rate = false, have_channels = false;
        for (uint64_t pos = pay + 4u; pos < end;) {
            DSDF_STEP();
            if (++visited > kMaxChunks) return fail(kInvalid, pos);
            if (end - pos < 12u) return fail(kInvalid, chunk);
            const uint32_t id = be32(p, pos);
            const uint64_t local = be64(p, pos + 4), at = pos + 12u;
            if (local > end - at) return fail(kInvalid, chunk);
            if (id == fourcc('F', 'S', ' ', ' ')) {
                if (local != 4u) return fail(kInvalid, chunk);
                f->rate = be32(p, at);
                if (f->rate == 0u) return fail(kInvalid, chunk);
                have_rate = true;
            } else if (id == fourcc('C', 'H', 'N', 'L')) {
                if (local < 2u) return fail(kInvalid, chunk);
                if (be16(p, at) != 2u) return fail(kUnsupported, chunk);
                have_channels = true;
            } else if (id == fourcc('C', 'M', 'P', 'R')) {
                if (local < 4u) return fail(kInvalid, chunk);
                if (be32(p, at) != fourcc('D', 'S', 'D', ' ')) return fail(kUnsupported, chunk);
            }
            pos = at + local + (local & 1u);
        }
        if (!have_rate || !have_channels) return fail(kInvalid, chunk);
        return kOk;
    }

    DSDF_HD uint32_t dff(Found* f)
    {
        bool have_prop = false, have_audio = false;
        for (uint64_t pos = 16; !(have_prop && have_audio);) {
            DSDF_STEP();
            if (++visited > kMaxChunks) return fail(kInvalid, pos);
            if (!holds(pos, 12)) return fail(kTruncated, pos);
            const uint32_t id = be32(p, pos);
            const uint64_t size = be64(p, pos + 4), pay = pos + 12u;
            if (size >> 63) return fail(kInvalid, pos);                        // (so that no position wraps)
            if (id == fourcc('F', 'V', 'E', 'R')) {
                if (size != 4u) return fail(kInvalid, pos);
                if (!holds(pay, 4)) return fail(kTruncated, pos);
                if (u8(p, pay) != 1u) return fail(kUnsupported, pos);
                f->version = be32(p, pay);
            } else if (id == fourcc('D', 'S', 'T', ' ') && !have_audio) {
                return fail(kUnsupported, pos);
            } else if (id == fourcc('P', 'R', 'O', 'P') && !have_prop) {
                if (size < 4u) return fail(kInvalid, pos);
                if (!holds(pay, size)) return fail(kTruncated, pos);
                if (be32(p, pay) == fourcc('S', 'N', 'D', ' ')) {
                    const uint32_t st = prop(pos, pay, size, f);
                    if (st != kOk) return st;
                    have_prop = true;
                }
            } else if (id == fourcc('D', 'S', 'D', ' ') && !have_audio) {
                if (size & 1u) return fail(kInvalid, pos);
                f->data_offset = pay;
                f->data_bytes = size;
                f->chunks_total = size / 4u;
                f->sample_count = 16u * f->chunks_total;
                have_audio = true;
            }
            pos = pay + size + (size & 1u);
        }
        return kOk;
    }

    DSDF_HD uint32_t run(const Stream& s, Result* out, Rec* rec)
    {
        if (n < 16u) return fail(kNotDsd, 0);
        Found f = {};
        const uint32_t id = be32(p, 0);
        uint32_t st;
        if (id == fourcc('D', 'S', 'D', ' ')) { f.kind = kDsf; st = dsf(&f); }
        else if (id == fourcc('F', 'R', 'M', '8') && be32(p, 12) == fourcc('D', 'S', 'D', ' ')) { f.kind = kDff; st = dff(&f); }
        else return fail(kNotDsd, 0);
        if (st != kOk) return st;
        // the chunks whose four source bytes all lie inside the stream
        const uint64_t present = f.data_offset < n ? n - f.data_offset : 0u;
        uint64_t available;
        if (f.kind == kDsf) {
            const uint64_t rest = present % kPair;                             // chunk r of a pair ends 4096 + 2 r + 2 bytes into it
            available = present / kPair * kPairChunks + (rest >= kPlane + 2u ? (rest - kPlane) / 2u : 0u);
        } else available = present / 4u;
        if (available > f.chunks_total) available = f.chunks_total;
        const uint32_t W = s.sample_block_words, cs = 4u + s.pad_bytes_per_chunk, per_block = W * 4u / cs;
        const uint64_t room = s.dst_bytes_capacity / (W * 4u) * per_block;
        uint64_t count = s.chunk_first < available ? available - s.chunk_first : 0u;
        if (count > room) count = room;
        uint64_t blocks = count / per_block;
        if (count && s.chunk_first + count == f.chunks_total) blocks = (count + per_block - 1u) / per_block;     // the stream's end: its last block is filled
        else count = blocks * per_block;
        out->kind = f.kind; out->channels = 2; out->sample_rate = f.rate; out->format_version = f.version; out->channel_type = f.channel_type;
        out->sample_count = f.sample_count; out->chunks_total = f.chunks_total; out->chunks_available = available;
        out->chunks_written = count; out->bytes_written = blocks * W * 4u;
        out->data_offset = f.data_offset; out->data_bytes = f.data_bytes; out->metadata_offset = f.metadata;
        rec->dst_pos = s.dst_offset;
        rec->fill_from = count * cs; rec->fill_to = blocks * W * 4u;
        rec->kind = f.kind; rec->pad = s.pad_bytes_per_chunk;
        rec->data_offset = (uint32_t)f.data_offset;
        rec->chunk_first = count ? (uint32_t)s.chunk_first : 0u;
        rec->n = (uint32_t)count;
        return kOk;
    }
};

// One stream: the result record (whole: every field is written) and the conversion's record.  `base`: the stream's first byte.
DSDF_HD void walk(const Stream& s, const uint8_t* base, Result* out, Rec* rec)
{
    Result r = {};
    Rec c = {};
    Walk w;
    w.p = base; w.n = s.src_bytes; w.err_at = 0; w.visited = 0;
    const uint32_t status = w.run(s, &r, &c);
    if (status != kOk) {                                              // a refusal says what and where; every other field reads 0
        Result none = {};
        Rec no_rec = {};
        r = none; c = no_rec;
        r.status = status; r.error_offset = w.err_at;
    }
    *out = r;
    *rec = c;
}

// ---- the conversion.  audio: the stream's first audio byte (base + data_offset).
DSDF_HD uint32_t reverse8(uint32_t b)
{
    b = ((b & 0xf0u) >> 4) | ((b & 0x0fu) << 4);
    b = ((b & 0xccu) >> 2) | ((b & 0x33u) << 2);
    return ((b & 0xaau) >> 1) | ((b & 0x55u) << 1);
}
// Byte o of chunk j of the audio in the pipeline's format: [P/2 x 00] L L [P/2 x 00] R R
DSDF_HD uint8_t chunk_byte(uint32_t kind, uint32_t P, const uint8_t* audio, uint64_t j, uint32_t o)
{
    const uint32_t h = P >> 1;
    if (o < h || (o >= h + 2u && o < 2u * h + 2u)) return 0;
    const uint32_t ch = o < h + 2u ? 0u : 1u, i = ch ? o - 2u * h - 2u : o - h;
    if (kind == kDsf) return (uint8_t)reverse8(audio[(j / kPairChunks) * kPair + ch * kPlane + (j % kPairChunks) * 2u + i]);
    return audio[j * 4u + ch + 2u * i];
}
// Output bytes [from, to) of the record's run, lane `lane` of `lanes`: the plain route, and what the fused route has outside its whole units
DSDF_HD void convert_bytes(const Rec& c, const uint8_t* audio, uint8_t* dst, uint64_t from, uint64_t to, uint32_t lane, uint32_t lanes)
{
    const uint32_t cs = 4u + c.pad;
    for (uint64_t t = from + lane; t < to; t += lanes) dst[t] = chunk_byte(c.kind, c.pad, audio, c.chunk_first + t / cs, (uint32_t)(t % cs));
}
DSDF_HD void fill_bytes(uint8_t* dst, uint64_t from, uint64_t to, uint32_t lane, uint32_t lanes)
{
    for (uint64_t t = from + lane; t < to; t += lanes) dst[t] = (uint8_t)kFillByte;
}

typedef uint32_t Line __attribute__((vector_size(16)));
DSDF_HD Line ld128(const uint8_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_nontemporal_load((const Line*)p);                 // read once
#else
    Line v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16);
    return v;
#endif
}
// v_alignbyte_b32: the low dword of hi:lo shifted right by `shift` bytes
DSDF_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t shift)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, shift);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * shift));
#endif
}
DSDF_HD uint32_t reverse32(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bitreverse32(v);                                  // v_bfrev_b32
#else
    return (reverse8(v & 0xffu) << 24) | (reverse8((v >> 8) & 0xffu) << 16) | (reverse8((v >> 16) & 0xffu) << 8) | reverse8(v >> 24);
#endif
}

// X aligned lines from `at` on; w[t], t < N = the N dwords that begin 4 quad + shift bytes into them (4 X >= N + 4)
template <uint32_t X, uint32_t N>
DSDF_HD void gather(const uint8_t* at, uint32_t shift, uint32_t quad, uint32_t* w)
{
    static_assert(4u * X >= N + 4u, "the lines hold the dwords at every quad and shift");
    uint32_t x[4u * X], f[N + 3u], g[N + 2u];
    const uint32_t odd = 0u - (quad & 1u), upper = 0u - ((quad >> 1) & 1u);   // all ones or none: a choice by mask, never by address
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t t = 0; t < X; t++) {
        const Line v = ld128(at + 16u * t);
        x[4u * t] = v[0]; x[4u * t + 1u] = v[1]; x[4u * t + 2u] = v[2]; x[4u * t + 3u] = v[3];
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t t = 0; t < N + 3u; t++) f[t] = funnel(x[t], x[t + 1u], shift);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t t = 0; t < N + 2u; t++) g[t] = (f[t] & ~odd) | (f[t + 1u] & odd);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t t = 0; t < N; t++) w[t] = (g[t] & ~upper) | (g[t + 2u] & upper);
}

// The permute and the stores of a unit: on the device csrc/dsd_perm.h's own; on the CPU the same selectors, read by hand
template <int KIND, int P, int V>
DSDF_HD void store_vec(const uint32_t (&in)[8], uint8_t* out)
{
#if defined(__HIP_DEVICE_COMPILE__)
    ohgpu::dsd_store_vec<KIND, P, V>(in, out);
#else
    uint32_t o[4] = {0, 0, 0, 0};
    for (int d = 0; d < 4; d++) {
        const ohgpu::DsdPerm p = ohgpu::dsd_perm(KIND, P, 4 * V + d);
        const uint64_t both = ((uint64_t)in[p.hi] << 32) | in[p.lo];
        for (int k = 0; k < 4; k++) {
            const uint32_t code = (p.sel >> (8 * k)) & 0xffu;
            if (code < 8u) o[d] |= (uint32_t)((both >> (8u * code)) & 0xffu) << (8 * k);      // (0x0c: a zero byte)
        }
    }
    __builtin_memcpy(__builtin_assume_aligned(out + 16 * V, 16), o, 16);
#endif
}

// How a stream's units are read: every unit's first source byte lies `quad` dwords and `shift` bytes into an aligned line -- the
// run's units are eight chunks apart, sixteen bytes of a plane or 32 of a DFF run, and the planes 4096 and 8192, so one phase serves
// all of them.  `end`: the end of the stream (base + src_bytes): no line is loaded that does not lie whole in front of it.
struct Phase { uint32_t shift, quad; };
DSDF_HD const uint8_t* unit_source(const Rec& c, const uint8_t* audio, uint32_t k)
{
    const uint64_t j = (uint64_t)c.chunk_first + k;
    return c.kind == kDsf ? audio + (j / kPairChunks) * kPair + (j % kPairChunks) * 2u : audio + j * 4u;
}
DSDF_HD Phase phase_of(const Rec& c, const uint8_t* audio)
{
    const uintptr_t a = (uintptr_t)unit_source(c, audio, 0);
    return Phase{(uint32_t)(a & 3u), (uint32_t)((a >> 2) & 3u)};
}

// Unit [k, k + 8) of the run (k a multiple of 8, so that its destination is a multiple of 16 bytes into the run); false where it has
// to go byte by byte
template <int KIND, int P>
DSDF_HD bool convert_unit(const Rec& c, const Phase ph, const uint8_t* audio, const uint8_t* end, uint8_t* dst, uint32_t k)
{
    const uint8_t* const a = unit_source(c, audio, k);
    const uint8_t* const line = a - ((uintptr_t)a & 15u);              // (from the pointer itself: the loads stay global loads)
    uint32_t in[8];
    if constexpr (KIND == (int)kDsf) {
        if (((c.chunk_first + k) % kPairChunks) > kPairChunks - kUnitChunks) return false;     // the unit runs on in the next pair
        if ((uintptr_t)(line + kPlane + 32u) > (uintptr_t)end) return false;
        gather<2, 4>(line, ph.shift, ph.quad, in);
        gather<2, 4>(line + kPlane, ph.shift, ph.quad, in + 4);
        for (int t = 0; t < 8; t++) in[t] = reverse32(in[t]);
    } else {
        if ((uintptr_t)(line + 48u) > (uintptr_t)end) return false;
        gather<3, 8>(line, ph.shift, ph.quad, in);
    }
    uint8_t* const out = dst + (uint64_t)k * (4u + P);
    store_vec<KIND, P, 0>(in, out);
    store_vec<KIND, P, 1>(in, out);
    if constexpr (P >= 2) store_vec<KIND, P, 2>(in, out);
    if constexpr (P >= 4) store_vec<KIND, P, 3>(in, out);
    return true;
}

// Chunks [k0, k1) of the run (k0 a multiple of 8), lane `lane` of `lanes`: whole units through convert_unit, the rest byte by byte
template <int KIND, int P>
DSDF_HD void convert_units(const Rec& c, const uint8_t* audio, const uint8_t* end, uint8_t* dst, uint32_t k0, uint32_t k1, uint32_t lane, uint32_t lanes)
{
    const uint32_t cs = 4u + P, units = (k1 - k0) / kUnitChunks;
    const Phase ph = phase_of(c, audio);
    for (uint32_t g = lane; g < units; g += lanes) {
        const uint32_t k = k0 + g * kUnitChunks;
        if (!convert_unit<KIND, P>(c, ph, audio, end, dst, k)) convert_bytes(c, audio, dst, (uint64_t)k * cs, (uint64_t)(k + kUnitChunks) * cs, 0, 1);
    }
    convert_bytes(c, audio, dst, (uint64_t)(k0 + units * kUnitChunks) * cs, (uint64_t)k1 * cs, lane, lanes);
}

// Whether a record's run has a body of whole units on the wide path (`dst_aligned`: the run's first destination byte is a multiple of 16)
DSDF_HD bool wide(const Rec& c, bool dst_aligned) { return dst_aligned && c.pad <= 4u; }

// Piece `piece` of a run -- chunks [piece x kPieceChunks, + kPieceChunks) of it, and the fill where the run ends inside the piece --,
// lane `lane` of `lanes`.  The caller leaves out the pieces that lie behind the run.
DSDF_HD void convert_piece(const Rec& c, const uint8_t* audio, const uint8_t* end, uint8_t* dst, uint32_t piece, bool dst_aligned, uint32_t lane, uint32_t lanes)
{
    const uint32_t k0 = piece * kPieceChunks, k1 = c.n - k0 < kPieceChunks ? c.n : k0 + kPieceChunks, cs = 4u + c.pad;
    if (!wide(c, dst_aligned)) convert_bytes(c, audio, dst, (uint64_t)k0 * cs, (uint64_t)k1 * cs, lane, lanes);
    else switch (c.kind * 8u + c.pad) {
    case kDsf * 8u + 0u: convert_units<kDsf, 0>(c, audio, end, dst, k0, k1, lane, lanes); break;
    case kDsf * 8u + 2u: convert_units<kDsf, 2>(c, audio, end, dst, k0, k1, lane, lanes); break;
    case kDsf * 8u + 4u: convert_units<kDsf, 4>(c, audio, end, dst, k0, k1, lane, lanes); break;
    case kDff * 8u + 0u: convert_units<kDff, 0>(c, audio, end, dst, k0, k1, lane, lanes); break;
    case kDff * 8u + 2u: convert_units<kDff, 2>(c, audio, end, dst, k0, k1, lane, lanes); break;
    default:             convert_units<kDff, 4>(c, audio, end, dst, k0, k1, lane, lanes); break;
    }
    if (k1 == c.n) fill_bytes(dst, c.fill_from, c.fill_to, lane, lanes);
}

// The pieces a stream's room can hold: what the plan makes workgroups from, before any walk
DSDF_HD uint64_t room_pieces(const Stream& s)
{
    const uint32_t W = s.sample_block_words, per_block = W * 4u / (4u + s.pad_bytes_per_chunk);
    const uint64_t room = s.dst_bytes_capacity / (W * 4u) * per_block;
    return (room + kPieceChunks - 1u) / kPieceChunks;
}

}  // namespace dsdfile
