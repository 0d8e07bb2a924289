// mp4_frag_core.h -- fragmented MPEG-4 (ISO/IEC 14496-12 movie fragments: DASH / CMAF segments) in front of the FLAC and Apple Lossless
// decoders: what stands between the bytes of an initialisation segment and its media segments and the sample table, the
// packet table and the gathered run the decoders take.  Every function is __host__ __device__: csrc/mp4_frag_kernel.hip runs this text
// on the device, tests/cpp/mp4f_core_driver.cpp runs the same text on the CPU under the sanitizers, csrc/api_mp4f.hip runs the walk for
// ohgpu_mp4f_head.  The box reader and the big-endian fields are csrc/mp4_box_core.h's; include/ohgpu.h's section has the rules in words.
//
//   the walk    one pass in file order, at most kMaxBoxes headers: ftyp, the first moov (trak > tkhd, mdia > mdhd, minf > stbl > stsd,
//               stsz; the first mvex, read at moov's end, when the track is known: trex, mehd), then every moof > traf > tfhd, tfdt,
//               trun.  It writes the result's head and one RunRec a trun of the taken track that has samples: where its entries lie,
//               which fields an entry has, the defaults, and what the boxes say of its place and its time.
//   the totals  a run's bytes and duration: counts x defaults where an entry has neither field (the walk), else a sum over the entries.
//   the carries serial over a stream's runs: the samples, the frames and the gathered bytes in front of each, and the place of a run
//               that follows its predecessor.  They write the public run rows.
//   expansion   sample i of run r lies at place_r + the sizes of the run's samples in front of it, and begins at frame_r + their
//               durations.  emit() writes both rows and judges the refusal.
//   the gather  a piece is the part of a run's bytes that belongs to rows [gather_first_row, samples_available): piece_of().
// The walk takes a policy (WalkT<P>): Clear, this layer's, admits clear tracks only; csrc/cenc_core.h's reads the protection boxes where
// the hooks stand (an `enca` entry, moov's end, a traf's other boxes and its end) and shares everything else with this walk.
// A run has at most kMaxRunSamples samples: that bounds what one workgroup of the expansion sums in front of its tile, and what the walk's
// lane sums for a run beyond run_capacity.
// Places are signed 64-bit (a data_offset may be negative), a base_data_offset beyond kFar counts as kFar, and a stream has at most
// kMaxSamples samples: no sum of places and sizes wraps.  Frames are counted modulo 2^64 (a tfdt may be anything).
#pragma once

#include "mp4_box_core.h"

namespace mp4frag {

using mp4box::be16;
using mp4box::be32;
using mp4box::be64;
using mp4box::Box;
using mp4box::Config;
using mp4box::fourcc;
using mp4box::read_box;
using mp4box::Row;
using mp4box::Sample;

enum Status : uint32_t { kOk = 0, kNotMp4 = 1, kTruncated = 2, kInvalid = 3, kNotCodec = 4, kUnsupported = 5, kNotFragmented = 6,
                         kNoKey = 7 };     // (kNoKey: the protected family's alone, csrc/cenc_core.h -- this walk never gives it)
constexpr uint32_t kMaxSamples = 1u << 24, kMaxRunSamples = 1u << 16, kMaxBoxes = 65536, kNone = 0xffffffffu;
constexpr uint32_t kTile = 1024;                      // samples a tile: one workgroup's share of the expansion
constexpr uint32_t kCodecAlac = 1, kCodecFlac = 2, kGather = 1;
constexpr uint64_t kFar = 1ull << 62;

struct Stream {               // 64 bytes = ohgpu_mp4f_stream_desc
    uint64_t src_offset;
    uint32_t src_bytes, codecs, flags, packet_first, packet_capacity, run_first, run_capacity, gather_first_row;
    uint64_t dst_offset, dst_capacity;
    uint32_t reserved[2];
};
struct FlacInfo {             // 48 bytes = ohgpu_flac_streaminfo_t
    uint32_t min_blocksize, max_blocksize, sample_rate;
    uint8_t  channels, bits, reserved[2];
    uint64_t total_samples;
    uint8_t  md5[16];
    uint32_t min_framesize, max_framesize;
};
struct Result {               // 168 bytes = ohgpu_mp4f_stream_result
    uint32_t status, codec, track_id, timescale;
    Config   config;
    FlacInfo flac;
    uint64_t duration, frames, samples;
    uint32_t runs, samples_available, samples_refused, first_bad_sample;
    uint32_t entry_rate;
    uint16_t entry_channels, entry_bits;
    uint64_t bytes_gathered, moov_offset, first_moof_offset, error_offset;
};
struct Run {                  // 32 bytes = ohgpu_mp4f_run
    uint64_t data_offset, first_frame;
    uint32_t first_sample, samples;
    uint64_t bytes;
};
// What the walk found of one run, and what the later phases add (device scratch; nothing of it is public).
struct RunRec {
    uint32_t entries_pos, stride;         // the first entry, from the stream's first byte; the bytes an entry (0: it has no fields)
    uint32_t size_at, dur_at;             // the field's place in an entry; kNone: every sample has def_size / def_dur
    uint32_t def_size, def_dur;
    uint32_t samples, flags;              // kPlaced | kTimed
    int64_t  place;                       // kPlaced: the run's first byte, from the stream's; the carries set it otherwise
    uint64_t time;                        // kTimed: the run's first frame; the carries set it otherwise
    uint64_t bytes, frames;               // the totals
    uint64_t gathered;                    // the bytes of the stream's runs in front of it (the carries)
    uint32_t first_sample;
    uint32_t iv_pos;                      // a protected track's: its first sample's IV, from the stream's first byte (the traf's end sets it); else 0
};
enum { kPlaced = 1, kTimed = 2 };
// What the walk and the later phases keep of one stream.
struct Rec {
    uint32_t runs_written, rows;          // min(runs, run_capacity); min(the samples of those runs, packet_capacity)
    uint32_t gather_run, gather_last;     // the runs that hold rows gather_first_row and samples_available - 1 (bytes_gathered != 0)
    uint64_t limit;                       // the codec's: a larger sample is refused
    uint64_t frames_beyond;               // the durations of the runs beyond run_capacity
    int64_t  gather_skip;                 // the bytes of gather_run that lie in front of row gather_first_row
};
static_assert(sizeof(Stream) == 64 && sizeof(FlacInfo) == 48 && sizeof(Result) == 168 && sizeof(Run) == 32 && sizeof(RunRec) == 80 && sizeof(Rec) == 40, "fragmented MPEG-4 layouts");

MP4B_HD uint32_t entry_size(const uint8_t* p, const RunRec& r, uint32_t i) { return r.size_at == kNone ? r.def_size : be32(p, r.entries_pos + (uint64_t)i * r.stride + r.size_at); }
MP4B_HD uint32_t entry_dur(const uint8_t* p, const RunRec& r, uint32_t i) { return r.dur_at == kNone ? r.def_dur : be32(p, r.entries_pos + (uint64_t)i * r.stride + r.dur_at); }
MP4B_HD bool needs_sums(const RunRec& r) { return r.size_at != kNone || r.dur_at != kNone; }
// the totals of a run's first `count` samples, one entry after the other
MP4B_HD void totals_serial(const uint8_t* p, const RunRec& r, uint32_t count, uint64_t* bytes, uint64_t* frames)
{
    if (!needs_sums(r)) { *bytes = (uint64_t)count * r.def_size; *frames = (uint64_t)count * r.def_dur; return; }
    uint64_t b = 0, f = 0;
    for (uint32_t i = 0; i < count; i++) { MP4B_STEP(1); b += entry_size(p, r, i); f += entry_dur(p, r, i); }
    *bytes = b; *frames = f;
}

// What a walk admits besides clear tracks.  Clear admits nothing: an `enca` entry stays UNSUPPORTED and a traf's other boxes are passed
// over.  csrc/cenc_core.h has the policy that reads the protection boxes; its hooks are called where these are, with the walk itself.
struct Clear {
    static constexpr bool kAdmits = false;
    template <class W> MP4B_HD uint32_t entry(W&, uint64_t, uint64_t, uint64_t, bool*) { return kOk; }       // an `enca` sample entry
    template <class W> MP4B_HD uint32_t after_moov(W&) { return kOk; }
    MP4B_HD void trak_begin() {}
    MP4B_HD void traf_begin() {}
    template <class W> MP4B_HD void traf_box(W&, uint32_t, uint64_t, uint64_t, uint64_t) {}                   // a traf's child that is no tfhd, tfdt or trun
    template <class W> MP4B_HD uint32_t traf_end(W&, uint64_t, uint32_t, uint32_t) { return kOk; }           // (the traf, its first run, its samples)
};

template <class P>
struct WalkT {
    P prot;
    const uint8_t* p;         // the stream's first byte
    uint32_t n;               // its bytes
    uint32_t visited;
    uint64_t err_at;
    uint32_t mask;            // the descriptor's codecs
    // the taken trak
    bool     taken, any_trak;
    uint32_t codec, first_codec, track_id, timescale, channels, bits, rate;
    uint64_t duration, limit, stsz_samples;
    Config   cfg;
    FlacInfo flac;
    // mvex
    bool     have_trex, have_mehd;
    uint32_t trex_dur, trex_size;
    uint64_t mehd_duration;
    // the runs
    RunRec*  runs;
    uint32_t run_capacity, n_runs, n_moofs;
    uint64_t samples, frames_beyond, first_moof;
    uint32_t traf_def_size;   // at a traf's end, for the policy: the size of a sample whose trun entry has none (tfhd's, else trex's)

    MP4B_HD uint32_t fail(uint32_t status, uint64_t at) { err_at = at; return status; }
    MP4B_HD bool visit() { MP4B_STEP(0); return ++visited <= kMaxBoxes; }

    // every child box of [pos, end) in order: f(type, box, payload, payload bytes) -> a status
    template <typename F>
    MP4B_HD uint32_t children(uint64_t pos, uint64_t end, F&& f)
    {
        for (;;) {
            Box b;
            const int got = read_box(p, pos, end, false, &b);
            if (got == 0) return kOk;
            if (!visit() || got != 1 || b.size > end - pos) return fail(kInvalid, pos);
            const uint32_t st = f(b.type, pos, pos + b.header, b.size - b.header);
            if (st != kOk) return st;
            pos += b.size;
        }
    }

    MP4B_HD uint32_t dfla(uint64_t box, uint64_t pay, uint64_t len)
    {
        if (len < 4u) return fail(kInvalid, box);
        if (be32(p, pay) != 0u) return fail(kUnsupported, box);
        const uint64_t end = pay + len;
        uint64_t at = pay + 4u;
        for (uint32_t k = 0;; k++) {
            MP4B_STEP(1);
            if (end - at < 4u) return fail(kInvalid, box);
            const uint32_t head = be32(p, at), type = (head >> 24) & 0x7fu, length = head & 0xffffffu;
            if (length > end - at - 4u) return fail(kInvalid, box);
            if (k == 0) {
                if (type != 0u || length != 34u) return fail(kInvalid, box);
                const uint64_t q = at + 4u;
                const uint32_t w10 = be32(p, q + 10), w14 = be32(p, q + 14);
                flac.min_blocksize = be16(p, q); flac.max_blocksize = be16(p, q + 2);
                flac.min_framesize = be32(p, q + 4) >> 8; flac.max_framesize = be32(p, q + 7) >> 8;
                flac.sample_rate = w10 >> 12;
                flac.channels = (uint8_t)(((w10 >> 9) & 7u) + 1u);
                flac.bits = (uint8_t)(((w10 >> 4) & 31u) + 1u);
                flac.total_samples = ((uint64_t)(w10 & 15u) << 32) | w14;
                for (uint32_t j = 0; j < 4u; j++) {
                    const uint32_t w = be32(p, q + 18 + 4u * j);
                    flac.md5[4 * j] = (uint8_t)(w >> 24); flac.md5[4 * j + 1] = (uint8_t)(w >> 16); flac.md5[4 * j + 2] = (uint8_t)(w >> 8); flac.md5[4 * j + 3] = (uint8_t)w;
                }
                if (flac.bits != 8 && flac.bits != 16 && flac.bits != 24) return fail(kUnsupported, box);
                limit = (uint64_t)flac.max_blocksize * flac.channels * (flac.bits / 8u + 1u) + 64u;
            }
            at += 4u + length;
            if ((head >> 31) || at == end) return kOk;
        }
    }

    // The first sample entry.  An `alac` entry, the count and the entry's own box are csrc/mp4_box_core.h's to judge (its boxes are
    // counted by a counter of their own, against that file's kMaxBoxes, and so are a fLaC entry's).
    MP4B_HD uint32_t stsd(uint64_t box, uint64_t pay, uint64_t len, bool* parsed)
    {
        mp4box::Walk w;
        w.p = p; w.n = n; w.visited = 0; w.err_at = 0;
        mp4box::Track fresh = {};
        w.tr = fresh;
        const uint32_t st = w.stsd(box, pay, len);
        if (P::kAdmits && st == kUnsupported && w.tr.codec == fourcc('e', 'n', 'c', 'a')) {      // (the entry's box was read and held to its parent)
            Box e;
            (void)read_box(p, pay + 8u, pay + len, false, &e);
            return prot.entry(*this, pay + 8u, pay + 8u + e.header, pay + 8u + e.size, parsed);
        }
        if (st != kOk) return fail(st, w.err_at);
        codec = w.tr.codec;
        if (codec == fourcc('a', 'l', 'a', 'c')) {
            cfg = w.tr.cfg; channels = w.tr.channels; bits = w.tr.bits; rate = w.tr.rate; limit = w.tr.t.packet_limit;
            *parsed = true;
            return kOk;
        }
        if (codec != fourcc('f', 'L', 'a', 'C') || !(mask & kCodecFlac)) return kOk;
        const uint64_t entry = pay + 8u;
        Box e;
        (void)read_box(p, entry, pay + len, false, &e);                   // (read and held to its parent above)
        const uint64_t q = entry + e.header, entry_end = entry + e.size;
        if (entry_end - q < 28u) return fail(kInvalid, entry);
        channels = be16(p, q + 16); bits = be16(p, q + 18); rate = be16(p, q + 24);
        for (uint64_t c = q + 28u; entry_end - c >= 8u;) {
            Box k;
            if (!w.visit()) return fail(kInvalid, c);
            if (read_box(p, c, entry_end, false, &k) != 1 || k.size > entry_end - c) return fail(kInvalid, c);
            if (k.type != fourcc('d', 'f', 'L', 'a')) { c += k.size; continue; }
            *parsed = true;
            return dfla(c, c + k.header, k.size - k.header);
        }
        return fail(kUnsupported, entry);
    }

    MP4B_HD uint32_t trak(uint64_t box, uint64_t pay, uint64_t len)
    {
        bool have_tkhd = false, have_mdhd = false, have_stsd = false, have_stsz = false, parsed = false;
        codec = 0; stsz_samples = 0;
        prot.trak_begin();
        const uint32_t st = children(pay, pay + len, [&](uint32_t type, uint64_t at, uint64_t q, uint64_t m) -> uint32_t {
            if (type == fourcc('t', 'k', 'h', 'd') && !have_tkhd) {
                have_tkhd = true;
                if (m < 4u || p[q] > 1u || m < (p[q] ? 24u : 16u)) return fail(kInvalid, at);
                track_id = be32(p, q + (p[q] ? 20u : 12u));
                return kOk;
            }
            if (type != fourcc('m', 'd', 'i', 'a')) return kOk;
            return children(q, q + m, [&](uint32_t type2, uint64_t at2, uint64_t q2, uint64_t m2) -> uint32_t {
                if (type2 == fourcc('m', 'd', 'h', 'd') && !have_mdhd) {
                    have_mdhd = true;
                    mp4box::Walk w;
                    w.p = p; w.n = n; w.visited = 0; w.err_at = 0;
                    const uint32_t s2 = w.mdhd(at2, q2, m2);
                    if (s2 != kOk) return fail(s2, w.err_at);
                    timescale = w.tr.timescale; duration = w.tr.duration;
                    return kOk;
                }
                if (type2 != fourcc('m', 'i', 'n', 'f')) return kOk;
                return children(q2, q2 + m2, [&](uint32_t type3, uint64_t, uint64_t q3, uint64_t m3) -> uint32_t {
                    if (type3 != fourcc('s', 't', 'b', 'l')) return kOk;
                    return children(q3, q3 + m3, [&](uint32_t type4, uint64_t at4, uint64_t q4, uint64_t m4) -> uint32_t {
                        if (type4 == fourcc('s', 't', 's', 'd') && !have_stsd) { have_stsd = true; return stsd(at4, q4, m4, &parsed); }
                        if (type4 == fourcc('s', 't', 's', 'z') && !have_stsz) { have_stsz = true; if (m4 >= 12u) stsz_samples = be32(p, q4 + 8); }
                        return kOk;
                    });
                });
            });
        });
        if (st != kOk) return st;
        if (!any_trak) { any_trak = true; first_codec = codec; }
        const uint32_t bit = codec == fourcc('a', 'l', 'a', 'c') ? kCodecAlac : codec == fourcc('f', 'L', 'a', 'C') ? kCodecFlac : 0u;
        if (!(bit & mask)) return kOk;
        if (!have_tkhd || !have_mdhd || !parsed) return fail(kInvalid, box);
        taken = true;
        return kOk;
    }

    MP4B_HD uint32_t moov(uint64_t box, uint64_t pay, uint64_t len, bool* have_mvex)
    {
        uint64_t mvex_pay = 0, mvex_len = 0;
        uint32_t st = children(pay, pay + len, [&](uint32_t type, uint64_t at, uint64_t q, uint64_t m) -> uint32_t {
            if (type == fourcc('t', 'r', 'a', 'k') && !taken) return trak(at, q, m);
            if (type == fourcc('m', 'v', 'e', 'x') && !*have_mvex) { *have_mvex = true; mvex_pay = q; mvex_len = m; }
            return kOk;
        });
        if (st != kOk) return st;
        if (!taken) return fail(kNotCodec, box);
        if (!*have_mvex) return kOk;
        return children(mvex_pay, mvex_pay + mvex_len, [&](uint32_t type, uint64_t at, uint64_t q, uint64_t m) -> uint32_t {
            if (type == fourcc('t', 'r', 'e', 'x') && !have_trex) {
                if (m < 24u) return fail(kInvalid, at);
                if (be32(p, q + 4) != track_id) return kOk;
                have_trex = true; trex_dur = be32(p, q + 12); trex_size = be32(p, q + 16);
            } else if (type == fourcc('m', 'e', 'h', 'd') && !have_mehd) {
                have_mehd = true;
                if (m < 4u || p[q] > 1u || m < (p[q] ? 12u : 8u)) return fail(kInvalid, at);
                mehd_duration = p[q] ? be64(p, q + 4) : be32(p, q + 4);
            }
            return kOk;
        });
    }

    MP4B_HD uint32_t traf(uint64_t moof, uint64_t box, uint64_t pay, uint64_t len, bool first_traf)
    {
        bool have_tfhd = false, mine = false, have_size = false, have_dur = false, first_run = true, timed = false;
        uint32_t def_size = 0, def_dur = 0;
        uint64_t base = moof, time = 0;
        const uint32_t run0 = n_runs;
        const uint64_t samples0 = samples;
        prot.traf_begin();
        const uint32_t st = children(pay, pay + len, [&](uint32_t type, uint64_t at, uint64_t q, uint64_t m) -> uint32_t {
            const bool tfhd = type == fourcc('t', 'f', 'h', 'd'), tfdt = type == fourcc('t', 'f', 'd', 't'), trun = type == fourcc('t', 'r', 'u', 'n');
            if (tfhd && !have_tfhd) {
                have_tfhd = true;
                if (m < 8u) return fail(kInvalid, at);
                const uint32_t fl = be32(p, q) & 0xffffffu;
                const uint32_t need = 8u + ((fl & 1u) ? 8u : 0u) + ((fl & 2u) ? 4u : 0u) + ((fl & 8u) ? 4u : 0u) + ((fl & 0x10u) ? 4u : 0u) + ((fl & 0x20u) ? 4u : 0u);
                if (m < need) return fail(kInvalid, at);
                mine = be32(p, q + 4) == track_id;
                if (!mine) return kOk;
                uint64_t f = q + 8u;
                if (fl & 1u) { base = be64(p, f); if (base > kFar) base = kFar; f += 8u; }
                else if (!(fl & 0x20000u) && !first_traf) return fail(kUnsupported, at);
                if (fl & 2u) f += 4u;
                have_dur = have_trex; def_dur = trex_dur; have_size = have_trex; def_size = trex_size;
                if (fl & 8u) { have_dur = true; def_dur = be32(p, f); f += 4u; }
                if (fl & 0x10u) { have_size = true; def_size = be32(p, f); f += 4u; }
                return kOk;
            }
            if (!tfdt && !trun) { prot.traf_box(*this, type, at, q, m); return kOk; }
            if (!have_tfhd) return fail(kInvalid, at);
            if (!mine) return kOk;
            if (tfdt) {
                if (!first_run || timed) return kOk;
                if (m < 4u || p[q] > 1u || m < (p[q] ? 12u : 8u)) return fail(kInvalid, at);
                timed = true; time = p[q] ? be64(p, q + 4) : be32(p, q + 4);
                return kOk;
            }
            if (m < 8u) return fail(kInvalid, at);
            const uint32_t fl = be32(p, q) & 0xffffffu, count = be32(p, q + 4);
            const uint32_t fixed = 8u + ((fl & 1u) ? 4u : 0u) + ((fl & 4u) ? 4u : 0u);
            if (m < fixed) return fail(kInvalid, at);
            RunRec r = {};
            r.dur_at = r.size_at = kNone;
            if (fl & 0x100u) { r.dur_at = r.stride; r.stride += 4u; }
            if (fl & 0x200u) { r.size_at = r.stride; r.stride += 4u; }
            if (fl & 0x400u) r.stride += 4u;
            if (fl & 0x800u) r.stride += 4u;
            if (r.stride && count > (m - fixed) / r.stride) return fail(kInvalid, at);
            if (count == 0u) return kOk;
            if ((r.size_at == kNone && !have_size) || (r.dur_at == kNone && !have_dur)) return fail(kInvalid, at);
            if (count > kMaxRunSamples || samples + count > kMaxSamples) return fail(kUnsupported, at);
            r.entries_pos = (uint32_t)(q + fixed); r.samples = count; r.def_size = def_size; r.def_dur = def_dur;
            if (fl & 1u) { r.flags |= kPlaced; r.place = (int64_t)base + (int32_t)be32(p, q + 8); }
            else if (first_run) { r.flags |= kPlaced; r.place = (int64_t)base; }
            if (first_run && timed) { r.flags |= kTimed; r.time = time; }
            first_run = false;
            if (!needs_sums(r)) totals_serial(p, r, count, &r.bytes, &r.frames);
            if (n_runs < run_capacity) runs[n_runs] = r;
            else {
                uint64_t b, f;
                totals_serial(p, r, count, &b, &f);
                frames_beyond += f;
            }
            n_runs++; samples += count;
            return kOk;
        });
        if (st != kOk) return st;
        if (!have_tfhd) return fail(kInvalid, box);
        traf_def_size = def_size;
        return mine ? prot.traf_end(*this, box, run0, (uint32_t)(samples - samples0)) : (uint32_t)kOk;
    }

    // head_only: the walk ends behind moov, as if the stream did
    MP4B_HD uint32_t run(bool head_only, Result* out)
    {
        if (n < 8u) return fail(kTruncated, 0);
        if (be32(p, 4) != fourcc('f', 't', 'y', 'p')) return fail(kNotMp4, 0);
        uint64_t pos = 0;
        bool moov_seen = false, have_mvex = false;
        for (;;) {
            Box b;
            const int got = read_box(p, pos, n, true, &b);
            if (got == 0 || got == 2) break;
            if (!visit() || got != 1) return fail(kInvalid, pos);
            const bool fits = b.size <= n - pos;
            if (b.type == fourcc('m', 'o', 'o', 'v') && !moov_seen) {
                if (!fits) return fail(kTruncated, pos);
                moov_seen = true; out->moov_offset = pos;
                const uint32_t st = moov(pos, pos + b.header, b.size - b.header, &have_mvex);
                if (st != kOk) return st;
                if (head_only) break;
                const uint32_t key = prot.after_moov(*this);
                if (key != kOk) return key;
            } else if (b.type == fourcc('m', 'o', 'o', 'f')) {
                if (!moov_seen) return fail(kInvalid, pos);
                if (!fits) break;
                if (!n_moofs++) first_moof = pos;
                uint32_t trafs = 0;
                const uint64_t moof = pos;
                const uint32_t st = children(pos + b.header, pos + b.size, [&](uint32_t type, uint64_t at, uint64_t q, uint64_t m) -> uint32_t {
                    return type == fourcc('t', 'r', 'a', 'f') ? traf(moof, at, q, m, !trafs++) : (uint32_t)kOk;
                });
                if (st != kOk) return st;
            } else if (!fits) break;
            pos += b.size;
        }
        if (!moov_seen) return fail(kTruncated, pos);
        if (!have_mvex && !n_moofs && stsz_samples) return fail(kNotFragmented, out->moov_offset);
        return kOk;
    }
};
using Walk = WalkT<Clear>;

// One stream: the result record (whole: every field is written), the stream's record and the records of its runs
// [0, min(runs, run_capacity)).  `base`: the stream's first byte.  `w`: a fresh walk (all zero but what its policy was given).
template <class P>
MP4B_HD void walk_into(WalkT<P>& w, const Stream& s, const uint8_t* base, bool head_only, Result* out, Rec* rec, RunRec* runs)
{
    Result r = {};
    Rec c = {};
    w.p = base; w.n = s.src_bytes; w.mask = s.codecs; w.runs = runs; w.run_capacity = s.run_capacity;
    const uint32_t status = w.run(head_only, &r);
    if (status != kOk && status != kNoKey) {
        Result none = {};
        r = none;
        r.status = status; r.error_offset = w.err_at;
        if (status == kNotCodec) r.codec = w.first_codec;
        if (status == kNotFragmented) r.codec = w.codec;
    } else {                  // (kNoKey: the walk ended behind moov -- what moov gave is kept, every count of a moof is 0)
        if (status == kNoKey) { r.status = status; r.error_offset = w.err_at; }
        r.codec = w.codec; r.track_id = w.track_id; r.timescale = w.timescale;
        if (w.codec == fourcc('a', 'l', 'a', 'c')) r.config = w.cfg; else r.flac = w.flac;
        r.duration = w.duration == 0u && w.have_mehd ? w.mehd_duration : w.duration;
        r.samples = w.samples; r.runs = w.n_runs;
        r.entry_rate = w.rate; r.entry_channels = (uint16_t)w.channels; r.entry_bits = (uint16_t)w.bits;
        r.first_moof_offset = w.first_moof;
        c.runs_written = w.n_runs < s.run_capacity ? w.n_runs : s.run_capacity;
        c.limit = w.limit; c.frames_beyond = w.frames_beyond;
    }
    r.first_bad_sample = kNone;
    *out = r;
    *rec = c;
}
MP4B_HD void walk(const Stream& s, const uint8_t* base, bool head_only, Result* out, Rec* rec, RunRec* runs)
{
    Walk w = {};
    walk_into(w, s, base, head_only, out, rec, runs);
}

// The carries of one stream, serial over its runs (their totals are there): the public rows, the result's frames, the record's rows.
MP4B_HD void carries(const Stream& s, Rec* rec, RunRec* runs, Run* rows, Result* out)
{
    uint64_t frame = 0, gathered = 0, frames = rec->frames_beyond;
    int64_t next_place = 0;
    uint32_t sample = 0;
    for (uint32_t k = 0; k < rec->runs_written; k++) {
        MP4B_STEP(1);
        RunRec& r = runs[k];
        if (!(r.flags & kPlaced)) r.place = next_place;
        if (!(r.flags & kTimed)) r.time = frame;
        r.first_sample = sample; r.gathered = gathered;
        next_place = r.place + (int64_t)r.bytes;
        frame = r.time + r.frames; frames += r.frames; gathered += r.bytes; sample += r.samples;
        Run row;
        row.data_offset = s.src_offset + (uint64_t)r.place; row.first_frame = r.time; row.first_sample = r.first_sample; row.samples = r.samples; row.bytes = r.bytes;
        rows[k] = row;
    }
    out->frames = frames;
    rec->rows = sample < s.packet_capacity ? sample : s.packet_capacity;
}

// Sample `index` of the stream, in run `run`, `before` bytes and `frames_before` frames behind the run's start: both rows.
// true: refused (its bytes leave the stream, or it is larger than the codec lets a sample be).
MP4B_HD bool emit(const Stream& st, const Rec& rec, const RunRec& r, uint32_t run, uint64_t before, uint64_t frames_before, uint32_t size, uint32_t dur, Row* row, Sample* sample)
{
    MP4B_STEP(2);
    const int64_t at = r.place + (int64_t)before, n = st.src_bytes;
    const bool inside = at >= 0 && at <= n && (int64_t)size <= n - at;
    const bool refused = !inside || size > rec.limit;
    row->src_offset = st.src_offset + (refused ? 0u : (uint64_t)at);
    row->bytes = refused ? 0u : size;
    row->reserved = 0;
    sample->first_frame = r.time + frames_before;
    sample->frames = dur;
    sample->chunk = run;
    return refused;
}

// The run that holds sample s of the stream (s < the samples of the written runs): the last whose first_sample is <= s.
MP4B_HD uint32_t run_of(const RunRec* runs, uint32_t n, uint32_t s)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        MP4B_STEP(3);
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (runs[mid].first_sample <= s) lo = mid; else hi = mid;
    }
    return lo;
}

// The plain route: every row of one stream with running sums, and the refusals into the result.
MP4B_HD void expand_serial(const Stream& st, const uint8_t* p, const Rec& rec, const RunRec* runs, Row* rows, Sample* samples, Result* out)
{
    uint32_t refused = 0, first_bad = kNone, s = 0;
    for (uint32_t k = 0; k < rec.runs_written && s < rec.rows; k++) {
        const RunRec& r = runs[k];
        uint64_t before = 0, frames_before = 0;
        for (uint32_t i = 0; i < r.samples && s < rec.rows; i++, s++) {
            const uint32_t size = entry_size(p, r, i), dur = entry_dur(p, r, i);
            if (emit(st, rec, r, k, before, frames_before, size, dur, &rows[s], &samples[s])) {
                refused++;
                if (first_bad == kNone) first_bad = s;
            }
            before += size; frames_before += dur;
        }
    }
    out->samples_refused = refused;
    out->first_bad_sample = first_bad;
}

// After the expansion: samples_available, and what the gather needs -- the runs its first and last rows lie in, the bytes of the first
// in front of its first row, and the sum (0, and no piece, where it exceeds dst_capacity).  `rows`: the stream's packet rows.
MP4B_HD void finish(const Stream& s, Rec* rec, const RunRec* runs, const Row* rows, Result* out)
{
    const uint32_t bad = out->first_bad_sample, avail = bad < rec->rows ? bad : rec->rows;
    out->samples_available = avail;
    out->bytes_gathered = 0;
    if (!(s.flags & kGather) || s.gather_first_row >= avail) return;
    const uint32_t g = run_of(runs, rec->runs_written, s.gather_first_row), last = run_of(runs, rec->runs_written, avail - 1u);
    const int64_t skip = (int64_t)(rows[s.gather_first_row].src_offset - s.src_offset) - runs[g].place;
    const int64_t end = (int64_t)(rows[avail - 1u].src_offset - s.src_offset) + rows[avail - 1u].bytes - runs[last].place;   // of the last run's bytes
    const uint64_t total = runs[last].gathered - runs[g].gathered + (uint64_t)(end - skip);
    if (total == 0u || total > s.dst_capacity) return;
    rec->gather_run = g; rec->gather_last = last; rec->gather_skip = skip;
    out->bytes_gathered = total;
}

// The piece of run k: false when the gather takes nothing of it.  *src: from the source arena's first byte; *dst: from the
// destination arena's.
MP4B_HD bool piece_of(const Stream& s, const Rec& rec, const RunRec* runs, const Row* rows, const Result& res, uint32_t k, uint64_t* src, uint64_t* dst, uint32_t* bytes)
{
    if (!res.bytes_gathered || k < rec.gather_run || k > rec.gather_last) return false;
    const RunRec& r = runs[k];
    const uint32_t a = r.first_sample > s.gather_first_row ? r.first_sample : s.gather_first_row;
    const uint32_t end = r.first_sample + r.samples, b = end < res.samples_available ? end : res.samples_available;
    const uint64_t from = rows[a].src_offset, to = rows[b - 1u].src_offset + rows[b - 1u].bytes;
    const int64_t in_run = (int64_t)(from - s.src_offset) - r.place;
    *src = from;
    *dst = s.dst_offset + (r.gathered - runs[rec.gather_run].gathered) + (uint64_t)(in_run - rec.gather_skip);
    *bytes = (uint32_t)(to - from);
    return to > from;
}

}  // namespace mp4frag
