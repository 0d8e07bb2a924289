// iff_chunk_core.h -- PCM files of the two IFF families (RIFF/WAVE, and FORM/AIFF with FORM/AIFC) in front of the pipeline's big-endian
// PCM: the chunk walk that finds the format and the audio, and the conversion of the audio run -- byte-order reversal
// and 32 -> 24 bit truncation of a run at any address.  Every function is __host__ __device__: csrc/iff_pcm_kernel.hip runs this text
// on the device, tests/cpp/iff_core_driver.cpp runs the same text on the CPU under the sanitizers.  The rules are written out in
// include/ohgpu.h's IFF section; this file is their one implementation.
//
//   the walk      12 bytes of form header, then chunks: id, u32 size (RIFF little-endian, FORM big-endian), payload, a pad byte behind
//                 an odd size.  The first `fmt ` and the first `data`, or the first `COMM` and the first `SSND`, in either order; it
//                 stops when it has both, after at most kMaxChunks headers.
//   the record    what the conversion needs of a stream: where its first source byte lies, how many output bytes there are, the sample
//                 widths, the byte order and the mode of the piece kernel.
//   the pieces    the destination run is cut into a head of up to 15 bytes, whole pieces of U output bytes that begin on a multiple of 16
//                 (U = 16, or 48 where an output sample has three bytes), and a tail.  A piece is made in three steps, all on
//                 registers with indices known at compile time: the aligned 16-byte source lines that hold its samples are joined by the
//                 64-bit-shift funnel and a choice among four dwords so that byte 0 is the first byte of its first sample; a byte permute per output dword reverses
//                 or truncates the samples; a second funnel shifts by the piece's phase inside its first output sample.  Head and
//                 tail go byte by byte through convert_byte(), which is also the whole of the plain route.
#pragma once

#include <stdint.h>

#include "field_bytes.h"

#if defined(__HIPCC__)
#define IFFC_HD __host__ __device__ __forceinline__
#else
#define IFFC_HD inline
#endif
// the CPU driver counts the walk's chunk headers through this
#ifndef IFFC_STEP
#define IFFC_STEP()
#endif

namespace iffchunk {

enum Status : uint32_t { kOk = 0, kNotIff = 1, kTruncated = 2, kInvalid = 3, kUnsupported = 4 };
enum Kind : uint32_t { kNoKind = 0, kWav = 1, kAiff = 2, kAifc = 3 };
enum : uint32_t { kLittle = 1, kBig = 2 };                            // OHGPU_ENDIAN_*
enum : uint32_t { kFlagWav8Unsigned = 1 };
constexpr uint32_t kMaxChunks = 4096, kMaxChannels = 10;
using fieldbytes::fourcc;

struct Stream {               // 64 bytes = ohgpu_iff_stream_desc
    uint64_t src_offset;
    uint32_t src_bytes, flags;
    uint64_t dst_offset, dst_bytes_capacity, frame_first;
    uint32_t dst_frame_capacity, max_bit_depth;
    uint32_t reserved[4];
};
struct Result {               // 80 bytes = ohgpu_iff_stream_result
    uint32_t status, kind, channels, sample_rate, src_bit_depth, out_bit_depth, src_endian, bit_rate;
    uint64_t frames_total, frames_available, frames_written;
    uint64_t data_offset, data_bytes, error_offset;
};
// the modes of the piece kernel; out_unit()/src_unit(): the output bytes of a piece and the source bytes they come from
enum Mode : uint32_t { kCopy = 0, kSwap16 = 1, kSwap32 = 2, kRev24 = 3, kLe32To24 = 4, kBe32To24 = 5 };
struct Rec {                  // 40 bytes: the walk's record for the conversion
    uint64_t dst_pos;         // of the destination arena
    uint32_t src_pos;         // of the stream: the first source byte of frame frame_first
    uint32_t out_bytes;       // n frames x channels x out sample bytes; 0: nothing to convert
    uint32_t in_sample, out_sample, little, xor8, mode, pad;
};
static_assert(sizeof(Stream) == 64 && sizeof(Result) == 80 && sizeof(Rec) == 40, "IFF layouts");

// ---- bytes: csrc/field_bytes.h's reader, aligned dwords on the device
using fieldbytes::le16;
using fieldbytes::le32;
using fieldbytes::be16;
using fieldbytes::be32;

struct Format { uint32_t channels, rate, depth, sample_bytes, little, bit_rate; };

struct Walk {
    const uint8_t* p;         // the stream's first byte
    uint64_t n;               // its bytes
    uint64_t err_at;

    IFFC_HD uint32_t fail(uint32_t status, uint64_t at) { err_at = at; return status; }

    // `fmt ` of `size` bytes at pay (inside the stream)
    IFFC_HD uint32_t wav_fmt(uint64_t chunk, uint64_t pay, uint32_t size, Format* f)
    {
        const uint32_t tag = le16(p, pay), channels = le16(p, pay + 2), rate = le32(p, pay + 4), byte_rate = le32(p, pay + 8), depth = le16(p, pay + 14);
        if (tag != 1u && tag != 0xfffeu) return fail(kUnsupported, chunk);
        if (tag == 0xfffeu && size == 40u && le16(p, pay + 24) != 1u) return fail(kUnsupported, chunk);
        if (channels == 0u) return fail(kInvalid, chunk);
        if (channels > kMaxChannels) return fail(kUnsupported, chunk);
        if (rate == 0u || byte_rate == 0u) return fail(kInvalid, chunk);
        if (depth == 0u || depth % 8u) return fail(kInvalid, chunk);
        if (depth > 32u) return fail(kUnsupported, chunk);
        f->channels = channels; f->rate = rate; f->depth = depth; f->sample_bytes = depth / 8u; f->little = 1; f->bit_rate = byte_rate * 8u;
        return kOk;
    }

    // `COMM` of `size` bytes at pay (inside the stream); *frames: its sample frames
    IFFC_HD uint32_t comm(uint64_t chunk, uint64_t pay, bool aifc, Format* f, uint32_t* frames)
    {
        const uint32_t channels = be16(p, pay), depth = be16(p, pay + 6), sign_exp = be16(p, pay + 8), mant = be32(p, pay + 10);
        *frames = be32(p, pay + 2);
        if (channels == 0u) return fail(kInvalid, chunk);
        if (channels > kMaxChannels) return fail(kUnsupported, chunk);
        if (depth != 8u && depth != 16u && depth != 20u && depth != 24u && depth != 32u) return fail(kUnsupported, chunk);
        if (sign_exp < 0x3fffu || sign_exp > 0x401eu) return fail(kInvalid, chunk);      // (a set sign bit lies above the range too)
        uint32_t rate = mant >> (0x401eu - sign_exp);
        if (rate == 0u) return fail(kInvalid, chunk);
        if (rate == 22255u) rate = 22050u;
        if (rate == 11127u) rate = 11025u;
        uint32_t little = 0;
        if (aifc) {
            const uint32_t how = be32(p, pay + 18);
            if (how == fourcc('s', 'o', 'w', 't') || how == fourcc('S', 'O', 'W', 'T')) little = 1;
            else if (how != fourcc('N', 'O', 'N', 'E')) return fail(kUnsupported, chunk);
        }
        f->channels = channels; f->rate = rate; f->depth = depth == 20u ? 24u : depth; f->sample_bytes = (depth + 7u) / 8u; f->little = little;
        f->bit_rate = rate * (channels * f->sample_bytes) * 8u;
        return kOk;
    }

    IFFC_HD uint32_t run(const Stream& s, Result* out, Rec* rec)
    {
        if (n < 12u) return fail(kNotIff, 0);
        const uint32_t form = be32(p, 0), type = be32(p, 8);
        uint32_t kind = kNoKind;
        if (form == fourcc('R', 'I', 'F', 'F') && type == fourcc('W', 'A', 'V', 'E')) kind = kWav;
        else if (form == fourcc('F', 'O', 'R', 'M') && type == fourcc('A', 'I', 'F', 'F')) kind = kAiff;
        else if (form == fourcc('F', 'O', 'R', 'M') && type == fourcc('A', 'I', 'F', 'C')) kind = kAifc;
        else return fail(kNotIff, 0);
        const bool wav = kind == kWav, continuous = wav && le32(p, 4) == 0u;
        const uint32_t id_format = wav ? fourcc('f', 'm', 't', ' ') : fourcc('C', 'O', 'M', 'M'), id_audio = wav ? fourcc('d', 'a', 't', 'a') : fourcc('S', 'S', 'N', 'D');
        Format f = {};
        bool have_format = false, have_audio = false;
        uint64_t audio_chunk = 0, audio_at = 0, audio_held = 0;       // the audio chunk, its first audio byte, the bytes it holds from there on
        uint32_t comm_frames = 0, visited = 0;
        for (uint64_t pos = 12; !(have_format && have_audio);) {
            IFFC_STEP();
            if (++visited > kMaxChunks) return fail(kInvalid, pos);
            if (pos > n || n - pos < 8u) return fail(kTruncated, pos);
            const uint32_t id = be32(p, pos), size = wav ? le32(p, pos + 4) : be32(p, pos + 4);
            const uint64_t pay = pos + 8u;
            if (id == id_format && !have_format) {
                if (wav ? (size != 16u && size != 18u && size != 40u) : (kind == kAiff ? size != 18u : size < 22u)) return fail(kInvalid, pos);
                if (size > n - pay) return fail(kTruncated, pos);
                const uint32_t st = wav ? wav_fmt(pos, pay, size, &f) : comm(pos, pay, kind == kAifc, &f, &comm_frames);
                if (st != kOk) return st;
                have_format = true;
            } else if (id == id_audio && !have_audio) {
                audio_chunk = pos;
                if (wav) {
                    audio_at = pay;
                    if (continuous) {                                 // the audio runs to the end of what there is: nothing lies behind it
                        if (!have_format) return fail(kInvalid, pos);
                        audio_held = n - pay;
                    } else audio_held = size;
                } else {
                    if (size < 8u) return fail(kInvalid, pos);
                    if (n - pay < 8u) return fail(kTruncated, pos);
                    const uint32_t offset = be32(p, pay);
                    if (offset > size - 8u) return fail(kInvalid, pos);
                    audio_at = pay + 8u + offset;
                    audio_held = size - 8u - offset;
                }
                have_audio = true;
            }
            pos = pay + size + (size & 1u);
        }
        const uint32_t frame_bytes = f.channels * f.sample_bytes;
        uint64_t data_bytes = audio_held, frames_total = audio_held / frame_bytes;
        if (!wav) {
            data_bytes = (uint64_t)comm_frames * frame_bytes;
            if (data_bytes > audio_held) return fail(kInvalid, audio_chunk);
            frames_total = comm_frames;
        }
        const uint64_t present = audio_at < n ? n - audio_at : 0u;
        const uint64_t available = (data_bytes < present ? data_bytes : present) / frame_bytes;
        const uint32_t out_depth = f.depth < s.max_bit_depth ? f.depth : s.max_bit_depth, out_sample = out_depth / 8u, out_frame = f.channels * out_sample;
        uint64_t frames = s.frame_first < available ? available - s.frame_first : 0u;
        if (frames > s.dst_frame_capacity) frames = s.dst_frame_capacity;
        if (frames > s.dst_bytes_capacity / out_frame) frames = s.dst_bytes_capacity / out_frame;
        out->kind = kind; out->channels = f.channels; out->sample_rate = f.rate; out->src_bit_depth = f.depth; out->out_bit_depth = out_depth;
        out->src_endian = f.little ? kLittle : kBig; out->bit_rate = f.bit_rate;
        out->frames_total = continuous ? 0u : frames_total; out->frames_available = available; out->frames_written = frames;
        out->data_offset = audio_at; out->data_bytes = data_bytes;
        rec->dst_pos = s.dst_offset;
        rec->src_pos = frames ? (uint32_t)(audio_at + s.frame_first * frame_bytes) : 0u;
        rec->out_bytes = (uint32_t)(frames * out_frame);
        rec->in_sample = f.sample_bytes; rec->out_sample = out_sample; rec->little = f.little;
        rec->xor8 = wav && f.depth == 8u && (s.flags & kFlagWav8Unsigned) ? 0x80u : 0u;
        // a run whose bytes keep their order is a copy, whatever its samples' width
        const bool same = out_sample == f.sample_bytes;
        rec->mode = (!f.little || f.sample_bytes == 1u) ? (same ? kCopy : kBe32To24)
                  : !same ? kLe32To24 : f.sample_bytes == 2u ? kSwap16 : f.sample_bytes == 3u ? kRev24 : kSwap32;
        rec->pad = 0;
        return kOk;
    }
};

// One stream: the result record (whole: every field is written) and the conversion's record.  `base`: the stream's first byte.
IFFC_HD void walk(const Stream& s, const uint8_t* base, Result* out, Rec* rec)
{
    Result r = {};
    Rec c = {};
    Walk w;
    w.p = base; w.n = s.src_bytes; w.err_at = 0;
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

// ---- the conversion.  run: the first source byte of the record's frames.
// Output byte o of the run: byte k = o % out_sample of sample o / out_sample, the most significant first.
IFFC_HD uint8_t convert_byte(const Rec& c, const uint8_t* run, uint32_t o)
{
    const uint32_t i = o / c.out_sample, k = o % c.out_sample;
    return (uint8_t)(run[(uint64_t)i * c.in_sample + (c.little ? c.in_sample - 1u - k : k)] ^ c.xor8);
}
// The plain route, and what a stream of the fused route has outside its whole pieces
IFFC_HD void convert_bytes(const Rec& c, const uint8_t* run, uint8_t* dst, uint32_t from, uint32_t to, uint32_t lane, uint32_t lanes)
{
    for (uint32_t o = from + lane; o < to; o += lanes) dst[o] = convert_byte(c, run, o);
}

IFFC_HD constexpr uint32_t out_unit(uint32_t mode) { return mode >= kRev24 ? 48u : 16u; }
IFFC_HD constexpr uint32_t src_unit(uint32_t mode) { return mode == kRev24 ? 48u : mode >= kLe32To24 ? 64u : 16u; }
IFFC_HD constexpr uint32_t mode_out_sample(uint32_t mode) { return mode == kCopy ? 1u : mode == kSwap16 ? 2u : mode == kSwap32 ? 4u : 3u; }
IFFC_HD constexpr uint32_t mode_in_sample(uint32_t mode) { return mode == kCopy ? 1u : mode == kSwap16 ? 2u : mode == kRev24 ? 3u : 4u; }
// the dwords of a piece in its sample-aligned form (one more than the source unit: the phase reaches into the next sample), and the
// aligned 16-byte lines loaded to make them: the first sample lies at any address, up to 15 bytes into the first line
IFFC_HD constexpr uint32_t piece_words(uint32_t mode) { return src_unit(mode) / 4u + 1u; }
IFFC_HD constexpr uint32_t piece_lines(uint32_t mode) { return (piece_words(mode) + 4u + 3u) / 4u; }

// How a run is cut.  Pieces j < pieces write dst[head + U j, + U) and load piece_lines aligned 16-byte lines from run + from + src_unit j
// on (src_unit is a multiple of 16, so every piece's first sample lies `quad` dwords and `shift` bytes into its first line); every such
// load lies inside [(run & ~15) - 12, (run + source bytes) & ~3): no load leaves the dwords that lie whole inside the stream, whose
// audio begins 20 bytes or more behind its first byte.
struct Cut { uint32_t head, pieces, tail_from, phase, shift, quad; int64_t from; };
IFFC_HD Cut cut(const Rec& c, uintptr_t run, uintptr_t dst)
{
    const uint32_t U = out_unit(c.mode), S = src_unit(c.mode), os = mode_out_sample(c.mode), is = mode_in_sample(c.mode);
    Cut k = {};
    k.head = (uint32_t)(-dst & 15u);
    if (k.head > c.out_bytes) k.head = c.out_bytes;
    k.phase = k.head % os;
    const uint64_t first = (uint64_t)(k.head / os) * is;              // piece 0's first sample, from the run's first byte
    k.shift = (uint32_t)((run + first) & 3u);
    k.quad = (uint32_t)(((run + first) >> 2) & 3u);
    k.from = (int64_t)first - (int64_t)(4u * k.quad + k.shift);
    const uint64_t src_bytes = (uint64_t)c.out_bytes / c.out_sample * c.in_sample;
    const int64_t limit = (int64_t)(((run + src_bytes) & ~(uintptr_t)3) - run);           // the end of the last whole dword, from the run's first byte
    const int64_t room = limit - k.from - 16 * (int64_t)piece_lines(c.mode);
    const uint32_t by_src = room < 0 ? 0u : (uint32_t)(room / S) + 1u, by_dst = (c.out_bytes - k.head) / U;
    k.pieces = by_src < by_dst ? by_src : by_dst;
    k.tail_from = k.head + U * k.pieces;
    return k;
}

typedef uint32_t Line __attribute__((vector_size(16)));
IFFC_HD Line ld128(const uint8_t* p)
{
    Line v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16);
    return v;
}
IFFC_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t shift_bytes) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * shift_bytes)); }
// v_perm_b32: byte i of the result is byte sel.byte[i] of the eight bytes hi:lo (0..3 lie in lo, 4..7 in hi)
IFFC_HD uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t v = 0;
    for (uint32_t i = 0; i < 4u; i++) v |= (uint32_t)((both >> (8u * ((sel >> (8u * i)) & 7u))) & 0xffu) << (8u * i);
    return v;
#endif
}
IFFC_HD void st128(uint8_t* p, const uint32_t* v) { __builtin_memcpy(__builtin_assume_aligned(p, 16), v, 16); }

// The permute step: y[t], t <= U / 4, from w[] (byte 0 of w: the first byte of the piece's first sample).  The last dword serves the
// phase alone (fewer than out-sample bytes of it are used), so it reads no source dword beyond piece_words.
template <uint32_t M>
IFFC_HD void permute(const uint32_t* w, uint32_t* y, uint32_t xor_mask)
{
    if constexpr (M == kCopy) {
        _Pragma("unroll") for (uint32_t t = 0; t < 5u; t++) y[t] = w[t] ^ xor_mask;
    } else if constexpr (M == kSwap16) {
        _Pragma("unroll") for (uint32_t t = 0; t < 5u; t++) y[t] = perm(0u, w[t], 0x02030001u);
    } else if constexpr (M == kSwap32) {
        _Pragma("unroll") for (uint32_t t = 0; t < 5u; t++) y[t] = perm(0u, w[t], 0x00010203u);
    } else if constexpr (M == kRev24) {
        // output bytes 0..11 of four samples <- source bytes 2 1 0 5 | 4 3 8 7 | 6 11 10 9
        _Pragma("unroll") for (uint32_t g = 0; g < 4u; g++) {
            const uint32_t* a = w + 3u * g;
            y[3u * g] = perm(a[1], a[0], 0x05000102u);
            y[3u * g + 1u] = perm(a[2], perm(a[1], a[0], 0x07040300u), 0x03040102u);   // (bytes 0 3 4 7 first, then 4 3 8 7 of them and the third dword)
            y[3u * g + 2u] = perm(a[2], a[1], 0x05060702u);
        }
        y[12] = perm(0u, w[12], 0x00000102u);
    } else if constexpr (M == kLe32To24) {
        // <- source bytes 3 2 1 7 | 6 5 11 10 | 9 15 14 13
        _Pragma("unroll") for (uint32_t g = 0; g < 4u; g++) {
            const uint32_t* a = w + 4u * g;
            y[3u * g] = perm(a[1], a[0], 0x07010203u);
            y[3u * g + 1u] = perm(a[2], a[1], 0x06070102u);
            y[3u * g + 2u] = perm(a[3], a[2], 0x05060701u);
        }
        y[12] = perm(0u, w[16], 0x00000203u);
    } else {
        // <- source bytes 0 1 2 4 | 5 6 8 9 | 10 12 13 14
        _Pragma("unroll") for (uint32_t g = 0; g < 4u; g++) {
            const uint32_t* a = w + 4u * g;
            y[3u * g] = perm(a[1], a[0], 0x04020100u);
            y[3u * g + 1u] = perm(a[2], a[1], 0x05040201u);
            y[3u * g + 2u] = perm(a[3], a[2], 0x06050402u);
        }
        y[12] = perm(0u, w[16], 0x00000100u);
    }
}

// Piece j of a run in mode M: `at` = the piece's first aligned source line, `to` = its 16-byte-aligned destination.  The byte funnel
// first, then the choice among four dwords (quad is the run's: two bit-field inserts under a uniform mask), so that every index is a constant.
template <uint32_t M>
IFFC_HD void convert_piece(const uint8_t* at, uint8_t* to, uint32_t shift, uint32_t quad, uint32_t phase, uint32_t xor_mask)
{
    constexpr uint32_t W = piece_words(M), X = piece_lines(M), Y = out_unit(M) / 4u;
    static_assert(4u * X >= W + 4u, "the lines hold the piece's dwords at every quad and shift");
    uint32_t x[4u * X], f[W + 3u], g[W + 2u], w[W], y[Y + 1u], z[Y];
    const uint32_t odd = 0u - (quad & 1u), upper = 0u - ((quad >> 1) & 1u);   // all ones or none: a choice by mask (a bit-field insert), never by address
    _Pragma("unroll") for (uint32_t t = 0; t < X; t++) {
        const Line v = ld128(at + 16u * t);
        x[4u * t] = v[0]; x[4u * t + 1u] = v[1]; x[4u * t + 2u] = v[2]; x[4u * t + 3u] = v[3];
    }
    _Pragma("unroll") for (uint32_t t = 0; t < W + 3u; t++) f[t] = funnel(x[t], x[t + 1u], shift);
    _Pragma("unroll") for (uint32_t t = 0; t < W + 2u; t++) g[t] = (f[t] & ~odd) | (f[t + 1u] & odd);
    _Pragma("unroll") for (uint32_t t = 0; t < W; t++) w[t] = (g[t] & ~upper) | (g[t + 2u] & upper);
    permute<M>(w, y, xor_mask);
    _Pragma("unroll") for (uint32_t t = 0; t < Y; t++) z[t] = funnel(y[t], y[t + 1u], phase);
    _Pragma("unroll") for (uint32_t t = 0; t < Y; t += 4u) st128(to + 4u * t, z + t);
}

// Lane `lane` of `lanes`: pieces [first, last) of a run (the caller keeps last <= cut.pieces)
template <uint32_t M>
IFFC_HD void convert_pieces(const Cut& k, const uint8_t* run, uint8_t* dst, uint32_t xor8, uint32_t first, uint32_t last, uint32_t lane, uint32_t lanes)
{
    const uint32_t xor_mask = xor8 * 0x01010101u;
    for (uint32_t j = first + lane; j < last; j += lanes)
        convert_piece<M>(run + k.from + (int64_t)src_unit(M) * j, dst + k.head + out_unit(M) * j, k.shift, k.quad, k.phase, xor_mask);
}
IFFC_HD void convert_pieces_of(const Rec& c, const Cut& k, const uint8_t* run, uint8_t* dst, uint32_t first, uint32_t last, uint32_t lane, uint32_t lanes)
{
    switch (c.mode) {
    case kCopy:     convert_pieces<kCopy>(k, run, dst, c.xor8, first, last, lane, lanes); break;
    case kSwap16:   convert_pieces<kSwap16>(k, run, dst, 0, first, last, lane, lanes); break;
    case kSwap32:   convert_pieces<kSwap32>(k, run, dst, 0, first, last, lane, lanes); break;
    case kRev24:    convert_pieces<kRev24>(k, run, dst, 0, first, last, lane, lanes); break;
    case kLe32To24: convert_pieces<kLe32To24>(k, run, dst, 0, first, last, lane, lanes); break;
    default:        convert_pieces<kBe32To24>(k, run, dst, 0, first, last, lane, lanes); break;
    }
}

}  // namespace iffchunk
