// ts_packet_core.h -- the MPEG transport stream demultiplexer and the ADTS frame table (the rules are stated in
// include/ohgpu_ts.h, T1-T5, P1-P5, A1-A3).  Every function is __host__ __device__: csrc/ts_packet_kernel.hip runs this text on the
// device, tests/cpp/ts_core_driver.cpp runs the same text on the CPU under the sanitizers.  Fields are read through csrc/field_bytes.h.
//
//   the packet  0 0x47 | 1 tei 0x80, payload_unit_start 0x40, PID high 5 | 2 PID low | 3 scrambling 0xc0, adaptation 0x20, payload 0x10,
//               continuity counter 0x0f | [4 adaptation length L, L bytes] | payload.  188 bytes.
//   classify    a grid packet -> Pkt, two words: PID, start bit, counter, kind (T1, T2), where its payload lies and how long it is; for a
//               PAT candidate (PID 0, start) the section check and its verdict.  A lane a packet.
//   tables      the corrupt packet, the PAT, the PMT and the audio PID of a stream: three minima over its grid.
//   sums        the audio packets are a sequence of segments, each from a payload_unit_start to the next.  What a packet delivers depends
//               on its segment's head (the limit E) and on the payload in front of it in the segment.  Seg is that state and combine()
//               its associative operator: the device scans it, demux() below folds it.  Per packet the sums leave run_end (the delivered
//               bytes up to and including it) and src_at (where its first elementary byte lies in the stream).
//   gather      by 16-byte pieces of the destination ADDRESS: a piece finds the packet of its first byte by bisection in run_end, then
//               takes its one, two or more source payloads in turn; each output word is read as the one or two aligned source words
//               that hold its bytes, joined by the byte funnel; one 16-byte store, bytes at a run's two ends.
#pragma once

#include <stdint.h>

#include "field_bytes.h"

#if defined(__HIPCC__)
#define TSP_HD __host__ __device__ __forceinline__
#else
#define TSP_HD inline
#endif

namespace tspkt {

namespace fb = fieldbytes;

constexpr uint32_t kPacket = 188, kNone = 0xffffffffu, kPoly = 0x04c11db7u, kUnbounded = 0xffffffffu;
constexpr uint64_t kNoPts = ~0ull;
enum Status : uint32_t { kOk = 0, kNoPat = 1, kNoPmt = 2, kNoAudio = 3, kCorrupt = 4 };
enum { kPesOpen = 1, kKnownFlags = 1 };
enum { kContinuation = 1, kExcess = 2, kTruncated = 4, kCcJump = 8 };
enum Kind : uint32_t { kGood = 0, kBadSync = 1, kTei = 2, kScrambled = 3, kCorruptField = 4 };

struct Stream {               // 64 bytes = ohgpu_ts_stream_desc
    uint64_t src_offset, dst_offset, dst_capacity;
    uint32_t src_bytes, flags, pmt_pid, audio_pid, pes_open_bytes, pes_first, pes_capacity;
    uint32_t reserved[3];
};
struct Result {               // 64 bytes = ohgpu_ts_stream_result
    uint8_t  status, trailing_bytes;
    uint16_t reserved;
    uint16_t pmt_pid, audio_pid;
    uint32_t packets, bad_sync, tei_packets, scrambled_packets, pat_packet, pmt_packet, audio_packets, pes_packets, bad_pes_starts;
    uint32_t bytes_delivered, dropped_bytes, cc_jumps, pes_open_bytes, corrupt_packet;
};
struct Pes {                  // 32 bytes = ohgpu_ts_pes
    uint64_t es_offset, pts;
    uint32_t bytes, packet, flags;
    uint8_t  stream_id, reserved[3];
};
static_assert(sizeof(Stream) == 64 && sizeof(Result) == 64 && sizeof(Pes) == 32, "transport stream layouts");

// ---- a classified packet.  w0: PID 0..12, start 13, counter 14..17, kind 18..20, payload bit 21.  w1: payload offset 0..7, payload
// bytes 8..15, the PID a section check found 16..28, that check passed 29.
struct Pkt { uint32_t w0, w1; };
TSP_HD uint32_t pid_of(Pkt k) { return k.w0 & 0x1fffu; }
TSP_HD bool     start_of(Pkt k) { return (k.w0 >> 13) & 1u; }
TSP_HD uint32_t cc_of(Pkt k) { return (k.w0 >> 14) & 15u; }
TSP_HD uint32_t kind_of(Pkt k) { return (k.w0 >> 18) & 7u; }
TSP_HD bool     paybit_of(Pkt k) { return (k.w0 >> 21) & 1u; }
TSP_HD uint32_t off_of(Pkt k) { return k.w1 & 0xffu; }
TSP_HD uint32_t len_of(Pkt k) { return (k.w1 >> 8) & 0xffu; }
TSP_HD uint32_t found_pid(Pkt k) { return (k.w1 >> 16) & 0x1fffu; }
TSP_HD bool     section_ok(Pkt k) { return (k.w1 >> 29) & 1u; }

// ---- the section checksum: most significant bit first, no table (a stream has two sections)
TSP_HD uint32_t crc_byte(uint32_t c, uint32_t byte)
{
    c ^= byte << 24;
    for (int k = 0; k < 8; k++) c = (c << 1) ^ ((c >> 31) ? kPoly : 0u);
    return c;
}
TSP_HD uint32_t crc_run(const uint8_t* p, uint64_t at, uint32_t n)
{
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < n; i++) c = crc_byte(c, fb::u8(p, at + i));
    return c;
}

// T1, T2: the packet at `pos` of the stream that begins at p
TSP_HD Pkt parse_packet(const uint8_t* p, uint64_t pos)
{
    const uint32_t w = fb::be32(p, pos);
    const uint32_t b1 = (w >> 16) & 0xffu, b3 = w & 0xffu;
    uint32_t kind = kGood, off = 4, len = 0;
    if ((w >> 24) != 0x47u) kind = kBadSync;
    else if (b1 & 0x80u) kind = kTei;
    else if (b3 & 0xc0u) kind = kScrambled;
    else {
        if (b3 & 0x20u) {
            const uint32_t L = fb::u8(p, pos + 4);
            if (L > 183u) kind = kCorruptField;
            else off = 5u + L;
        }
        if (kind == kGood && (b3 & 0x10u)) len = kPacket - off;
    }
    Pkt k;
    k.w0 = (((b1 & 0x1fu) << 8) | ((w >> 8) & 0xffu)) | (((b1 >> 6) & 1u) << 13) | ((b3 & 15u) << 14) | (kind << 18) | (((b3 >> 4) & 1u) << 21);
    k.w1 = off | (len << 8);
    return k;
}

// T3, T4: the section behind the pointer field of the payload [at, at + len); table_id 0 gives the PMT's PID, 2 the audio PID (0: the
// table is good and has no stream of type 0x0f)
TSP_HD bool section(const uint8_t* p, uint64_t at, uint32_t len, uint32_t table_id, uint32_t* pid)
{
    if (len < 1u) return false;
    const uint32_t ptr = fb::u8(p, at);
    if (1u + ptr + 3u > len) return false;
    const uint64_t s = at + 1u + ptr;
    const uint32_t f = fb::u8(p, s + 1);
    if (fb::u8(p, s) != table_id) return false;
    if ((f & 0x80u) != 0x80u || (f & 0x40u) != 0u || (f & 0x30u) != 0x30u || (f & 0x0cu) != 0u) return false;
    const uint32_t sl = ((f & 3u) << 8) | fb::u8(p, s + 2);
    if (sl > 1021u || sl < (table_id == 0u ? 9u : 13u) || 1u + ptr + 3u + sl > len) return false;
    if ((fb::u8(p, s + 5) & 0xc0u) != 0xc0u) return false;
    if (crc_run(p, s, 3u + sl) != 0u) return false;
    const uint64_t end = s + 3u + sl - 4u;
    if (table_id == 0u) {
        for (uint64_t e = s + 8; e + 4 <= end; e += 4) {
            const uint32_t b = fb::u8(p, e + 2);
            if ((b & 0xe0u) != 0xe0u) return false;
            if (fb::be16(p, e) != 0u) {
                *pid = ((b & 0x1fu) << 8) | fb::u8(p, e + 3);
                return *pid != 0u;
            }
        }
        return false;
    }
    const uint64_t q = s + 8;
    const uint32_t b2 = fb::u8(p, q + 2);
    if ((fb::u8(p, q) & 0xe0u) != 0xe0u || (b2 & 0xf0u) != 0xf0u || (b2 & 0x0cu) != 0u) return false;
    uint64_t e = q + 4u + (((b2 & 3u) << 8) | fb::u8(p, q + 3));
    if (e > end) return false;
    *pid = 0;
    while (e < end) {
        if (end - e < 5u) return false;
        const uint32_t b1 = fb::u8(p, e + 1), b3 = fb::u8(p, e + 3);
        if ((b1 & 0xe0u) != 0xe0u || (b3 & 0xf0u) != 0xf0u || (b3 & 0x0cu) != 0u) return false;
        if (fb::u8(p, e) == 0x0fu) {
            *pid = ((b1 & 0x1fu) << 8) | fb::u8(p, e + 2);
            return true;
        }
        e += 5u + (((b3 & 3u) << 8) | fb::u8(p, e + 4));
        if (e > end) return false;
    }
    return true;
}
TSP_HD Pkt with_section(Pkt k, const uint8_t* p, uint64_t pos, uint32_t table_id)
{
    uint32_t pid = 0;
    if (section(p, pos + off_of(k), len_of(k), table_id, &pid)) k.w1 |= (pid << 16) | (1u << 29);
    return k;
}
// grid packet k of stream s, and the PAT check where T3 looks for one
TSP_HD Pkt classify(const Stream& s, const uint8_t* p, uint32_t k)
{
    const uint64_t pos = (uint64_t)k * kPacket;
    Pkt pk = parse_packet(p, pos);
    if (!s.pmt_pid && !s.audio_pid && kind_of(pk) == kGood && pid_of(pk) == 0u && start_of(pk)) pk = with_section(pk, p, pos, 0u);
    return pk;
}

// ---- the tables of a stream: what the minima are taken over, and what follows from them
struct Tab { uint32_t corrupt, pat, pmt, pmt_pid, audio_pid, first; };   // first: the first grid index an audio packet may have
TSP_HD bool pat_here(const Stream& s, Pkt k) { return !s.pmt_pid && !s.audio_pid && section_ok(k) && pid_of(k) == 0u; }
TSP_HD bool pmt_candidate(const Stream& s, const Tab& t, Pkt k, uint32_t i)
{
    if (s.audio_pid || !t.pmt_pid || kind_of(k) != kGood || !start_of(k) || pid_of(k) != t.pmt_pid || i >= t.corrupt) return false;
    return s.pmt_pid ? true : (t.pat != kNone && i > t.pat);
}
TSP_HD bool is_audio(const Tab& t, Pkt k, uint32_t i) { return t.audio_pid && kind_of(k) == kGood && pid_of(k) == t.audio_pid && i >= t.first && i < t.corrupt; }
TSP_HD uint32_t status_of(const Stream&, const Tab& t)
{
    if (t.corrupt != kNone) return kCorrupt;
    if (t.audio_pid) return kOk;
    if (t.pmt != kNone) return kNoAudio;
    return t.pmt_pid ? kNoPmt : kNoPat;
}

// ---- P1, P3: the head of a PES packet in the payload [at, at + len)
struct Elem { uint32_t c, skip, start, good, limit, sid; uint64_t pts; };   // c: the payload bytes that count towards A; skip: the header's
TSP_HD Elem audio_elem(const uint8_t* p, uint32_t i, Pkt k)
{
    Elem e = {len_of(k), 0u, start_of(k) ? 1u : 0u, 0u, 0u, 0u, kNoPts};
    if (!e.start) return e;
    const uint64_t at = (uint64_t)i * kPacket + off_of(k);
    const uint32_t len = len_of(k);
    if (len < 9u || (fb::be32(p, at) >> 8) != 1u) return e;
    const uint32_t sid = fb::u8(p, at + 3), N = fb::be16(p, at + 4), f7 = fb::u8(p, at + 7), h = fb::u8(p, at + 8);
    if (sid < 0xc0u || sid > 0xdfu || (fb::u8(p, at + 6) & 0xc0u) != 0x80u || 9u + h > len || (N != 0u && N < 3u + h)) return e;
    e.good = 1; e.skip = 9u + h; e.c = len - e.skip; e.sid = sid;
    e.limit = N ? N - 3u - h : kUnbounded;
    if ((f7 & 0x80u) && h >= 5u) {
        const uint64_t b9 = fb::u8(p, at + 9);
        const uint64_t r = fb::be32(p, at + 10);
        e.pts = (((b9 >> 1) & 7u) << 30) | (((r >> 24) & 0xffu) << 22) | (((r >> 17) & 0x7fu) << 15) | (((r >> 8) & 0xffu) << 7) | ((r >> 1) & 0x7fu);
    }
    return e;
}

// ---- P2, P4, P5: a segment's state and its operator.  sum: the payload bytes so far (A); limit: E of its head; bits: a head lies in
// the range, the segment has a record, a counter jumped in it.
enum { kSegHead = 1, kSegRec = 2, kSegJump = 4 };
struct Seg { uint32_t sum, limit, bits; };
TSP_HD Seg combine(Seg a, Seg b)
{
    if (b.bits & kSegHead) return b;
    return Seg{a.sum + b.sum, a.limit, a.bits | b.bits};
}
TSP_HD Seg seg_start(const Stream& s) { return Seg{0u, (s.flags & kPesOpen) ? s.pes_open_bytes : 0u, 0u}; }
// the element of an audio packet: `first` -- it is the stream's first audio packet; `jump` -- its counter does not follow
TSP_HD Seg seg_of(const Stream& s, const Elem& e, bool first, bool jump)
{
    uint32_t bits = jump ? (uint32_t)kSegJump : 0u;
    if (e.start) bits |= kSegHead | (e.good ? (uint32_t)kSegRec : 0u);
    else if (first && (s.flags & kPesOpen)) bits |= kSegRec;
    return Seg{e.c, e.start ? (e.good ? e.limit : 0u) : 0u, bits};
}
TSP_HD bool makes_record(const Stream& s, const Elem& e, bool first) { return e.start ? e.good != 0u : (first && (s.flags & kPesOpen)); }
// what a packet delivers: `before` is the state in front of it
TSP_HD uint32_t delivers(const Seg& before, const Elem& e)
{
    const uint32_t prefix = e.start ? 0u : before.sum, limit = e.start ? (e.good ? e.limit : 0u) : before.limit;
    if (limit <= prefix) return 0u;
    return limit - prefix < e.c ? limit - prefix : e.c;
}
// a record's two halves: its head's fields when the segment begins, the rest when the next one begins (or the input ends)
TSP_HD void record_head(const Stream& s, Pes* table, uint32_t r, uint32_t run_pos, uint32_t packet, const Elem& e)
{
    if (r >= s.pes_capacity) return;
    Pes& o = table[s.pes_first + r];
    o.es_offset = run_pos; o.pts = e.start ? e.pts : kNoPts; o.packet = packet; o.stream_id = (uint8_t)(e.start ? e.sid : 0u);
    o.reserved[0] = o.reserved[1] = o.reserved[2] = 0;
}
TSP_HD void record_tail(const Stream& s, Pes* table, uint32_t r, const Seg& g, bool before_start)
{
    if (r >= s.pes_capacity) return;
    Pes& o = table[s.pes_first + r];
    o.bytes = g.sum < g.limit ? g.sum : g.limit;
    o.flags = (g.sum > g.limit ? (uint32_t)kExcess : 0u) | (before_start && g.sum < g.limit && g.limit != kUnbounded ? (uint32_t)kTruncated : 0u) |
              ((g.bits & kSegJump) ? (uint32_t)kCcJump : 0u) | ((g.bits & kSegHead) ? 0u : (uint32_t)kContinuation);
}
TSP_HD uint32_t open_bytes_at_end(const Stream& s, const Seg& g, uint32_t n_audio)
{
    if (!n_audio) return (s.flags & kPesOpen) ? s.pes_open_bytes : 0u;
    if (!(g.bits & kSegRec)) return 0u;
    if (g.limit == kUnbounded) return kUnbounded;
    return g.sum < g.limit ? g.limit - g.sum : 0u;
}

// ---- the gather.  word(): the aligned 4-byte word at `a`, of which the bytes in [lo, hi) are wanted.  The device loads the word (it
// holds a wanted byte, so it lies in memory the stream's words lie in); the host reads the wanted bytes alone.
TSP_HD uint32_t word(const uint8_t* a, const uint8_t* lo, const uint8_t* hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lo; (void)hi;
    return *(const uint32_t*)a;
#else
    uint32_t v = 0;
    for (uint32_t b = 0; b < 4u; b++) if (a + b >= lo && a + b < hi) v |= (uint32_t)a[b] << (8u * b);
    return v;
#endif
}
TSP_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t shift_bytes) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * shift_bytes)); }
TSP_HD void store16(uint8_t* to, const uint32_t w[4])
{
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint4*)to = make_uint4(w[0], w[1], w[2], w[3]);
#else
    for (uint32_t b = 0; b < 16u; b++) to[b] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u)));
#endif
}
TSP_HD uint32_t piece_count(const uint8_t* run, uint32_t bytes)       // the 16-byte lines of the address space that [run, run + bytes) touches
{
    if (!bytes) return 0u;
    const uintptr_t a = (uintptr_t)run;
    return (uint32_t)((((a + bytes + 15u) & ~(uintptr_t)15) - (a & ~(uintptr_t)15)) / 16u);
}
// Piece q of a stream's run: `run` = dst + dst_offset, `bytes` delivered, `base` = src + src_offset, run_end / src_at the stream's own
// rows, np of them.  Loads: only words that hold a byte some packet delivers.  Stores: only inside [run, run + bytes).
TSP_HD void gather_piece(const uint8_t* base, uint8_t* run, uint32_t bytes, const uint32_t* run_end, const uint32_t* src_at, uint32_t np, uint32_t q)
{
    const uintptr_t a0 = (uintptr_t)run, line = (a0 & ~(uintptr_t)15) + 16u * (uintptr_t)q;
    const uintptr_t lo = line > a0 ? line : a0, hi = line + 16u < a0 + bytes ? line + 16u : a0 + bytes;
    if (lo >= hi) return;
    const uint32_t r0 = (uint32_t)(lo - a0), r1 = (uint32_t)(hi - a0);
    uint32_t a = 0, b = np;                                           // the first packet with run_end > r0
    while (a < b) {
        const uint32_t m = a + (b - a) / 2u;
        if (run_end[m] > r0) b = m; else a = m + 1u;
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    uint32_t r = r0;
    for (uint32_t k = a; r < r1 && k < np; k++) {
        const uint32_t end_k = run_end[k], begin_k = k ? run_end[k - 1u] : 0u;
        if (end_k <= r) continue;                                     // (a packet that delivers nothing)
        const uint32_t upto = end_k < r1 ? end_k : r1;
        const uint8_t* const from = base + src_at[k] + (r - begin_k);   // the source of run byte r
        const uint32_t b0 = (uint32_t)(a0 + r - line), b1 = (uint32_t)(a0 + upto - line);   // [b0, b1) of the line's 16 bytes
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t t = 0; t < 4u; t++) {
            const uint32_t x0 = b0 > 4u * t ? b0 : 4u * t, x1 = b1 < 4u * t + 4u ? b1 : 4u * t + 4u;
            if (x0 >= x1) continue;
            const uint8_t* const f = from + (x0 - b0);
            const uint32_t cnt = x1 - x0, sh = (uint32_t)((uintptr_t)f & 3u);
            const uint8_t* const al = f - sh;
            const uint32_t w_lo = word(al, f, f + cnt), w_hi = sh + cnt > 4u ? word(al + 4, f, f + cnt) : 0u;
            const uint32_t v = funnel(w_lo, w_hi, sh) & (cnt == 4u ? 0xffffffffu : ((1u << (8u * cnt)) - 1u));
            w[t] |= v << (8u * (x0 - 4u * t));
        }
        r = upto;
    }
    if (hi - lo == 16u) { store16((uint8_t*)lo, w); return; }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t x = 0; x < 16u; x++)                                // (unrolled: w stays in registers)
        if (line + x >= lo && line + x < hi) *(uint8_t*)(line + x) = (uint8_t)(w[x >> 2] >> (8u * (x & 3u)));
}

// ---- one stream from end to end, serially: the plain route's lane and the CPU driver.  pk, run_end, src_at: packets() rows each.
TSP_HD uint32_t packets(const Stream& s) { return s.src_bytes / kPacket; }
TSP_HD void demux(const Stream& s, const uint8_t* src, uint8_t* dst, Pes* table, Pkt* pk, uint32_t* run_end, uint32_t* src_at, Result* out)
{
    const uint8_t* const base = src + s.src_offset;
    const uint32_t np = packets(s);
    Tab t = {kNone, kNone, kNone, s.pmt_pid, s.audio_pid, 0u};
    for (uint32_t i = 0; i < np; i++) {
        pk[i] = classify(s, base, i);
        if (t.corrupt == kNone && kind_of(pk[i]) == kCorruptField) t.corrupt = i;
    }
    Result r = {};
    r.trailing_bytes = (uint8_t)(s.src_bytes % kPacket);
    r.packets = np;
    for (uint32_t i = 0; i < np && i < t.corrupt; i++) {
        const uint32_t kind = kind_of(pk[i]);
        r.bad_sync += kind == kBadSync; r.tei_packets += kind == kTei; r.scrambled_packets += kind == kScrambled;
        if (t.pat == kNone && pat_here(s, pk[i])) { t.pat = i; t.pmt_pid = found_pid(pk[i]); }
    }
    for (uint32_t i = 0; i < np && t.pmt == kNone; i++) {
        if (!pmt_candidate(s, t, pk[i], i)) continue;
        const Pkt c = with_section(pk[i], base, (uint64_t)i * kPacket, 2u);
        if (section_ok(c)) { t.pmt = i; t.audio_pid = found_pid(c); t.first = i + 1u; }
    }
    Seg st = seg_start(s);
    uint32_t n_rec = 0, deliv = 0;
    int last_cc = -1;
    for (uint32_t i = 0; i < np; i++) {
        src_at[i] = 0;
        run_end[i] = deliv;
        if (!is_audio(t, pk[i], i)) continue;
        const Elem e = audio_elem(base, i, pk[i]);
        const bool first = r.audio_packets == 0u;
        const bool jump = paybit_of(pk[i]) && last_cc >= 0 && cc_of(pk[i]) != (((uint32_t)last_cc + 1u) & 15u);
        if (paybit_of(pk[i])) last_cc = (int)cc_of(pk[i]);
        if (e.start) {
            if (st.bits & kSegRec) record_tail(s, table, n_rec - 1u, st, true);
            r.bad_pes_starts += !e.good;
        }
        const uint32_t d = delivers(st, e);
        if (makes_record(s, e, first)) record_head(s, table, n_rec++, deliv, i, e);
        st = combine(st, seg_of(s, e, first, jump));
        r.cc_jumps += jump;
        src_at[i] = i * kPacket + off_of(pk[i]) + e.skip;
        deliv += d;
        run_end[i] = deliv;
        r.dropped_bytes += e.c - d;
        r.audio_packets++;
    }
    if (st.bits & kSegRec) record_tail(s, table, n_rec - 1u, st, false);
    r.status = (uint8_t)status_of(s, t);
    r.pmt_pid = (uint16_t)t.pmt_pid; r.audio_pid = (uint16_t)t.audio_pid;
    r.pat_packet = t.pat; r.pmt_packet = t.pmt; r.corrupt_packet = t.corrupt;
    r.pes_packets = n_rec; r.bytes_delivered = deliv;
    r.pes_open_bytes = open_bytes_at_end(s, st, r.audio_packets);
    *out = r;
    uint8_t* const run = dst + s.dst_offset;
    const uint32_t pieces = piece_count(run, deliv);
    for (uint32_t q = 0; q < pieces; q++) gather_piece(base, run, deliv, run_end, src_at, np, q);
}

}  // namespace tspkt

// ---- ADTS: A1-A3 of include/ohgpu_ts.h
namespace adts {

namespace fb = fieldbytes;

enum { kOk = 0, kNotAdts = 1 };
enum { kRecognise = 1, kKnownFlags = 1 };
enum { kInterrupted = 1 };
constexpr uint32_t kLastStart = 1001, kRecogniseFrames = 5, kRecogniseBytes = 10, kMinBytes = 7;

struct Stream {               // 32 bytes = ohgpu_adts_stream_desc
    uint64_t src_offset;
    uint32_t src_bytes, flags, frame_first, frame_capacity;
    uint32_t reserved[2];
};
struct Result {               // 64 bytes = ohgpu_adts_stream_result
    uint32_t status, frames, bytes_consumed, first_frame_offset, interruptions, skipped_bytes, mean_payload_bytes;
    uint8_t  profile, sf_index, channel_config, reserved;
    uint32_t reserved2[8];
};
struct Frame {                // 32 bytes = ohgpu_adts_frame
    uint64_t offset;
    uint32_t bytes, flags;
    uint8_t  header_bytes, profile, sf_index, channel_config;
    uint32_t reserved[3];
};
static_assert(sizeof(Stream) == 32 && sizeof(Result) == 64 && sizeof(Frame) == 32, "ADTS layouts");

struct Hdr { uint32_t bytes, header_bytes, profile, sf_index, channel_config; };
// A1: the header at p of the n bytes at base
TSP_HD bool header_at(const uint8_t* base, uint32_t n, uint64_t p, Hdr* h)
{
    if (p + kMinBytes > n) return false;
    const uint32_t w = fb::be32(base, p), x = fb::be32(base, p + 3);  // bytes 0..3 and 3..6
    if ((w >> 20) != 0xfffu || (w & 0x00060000u) != 0u) return false;
    h->header_bytes = (w & 0x00010000u) ? 7u : 9u;
    h->profile = (w >> 14) & 3u;
    h->sf_index = (w >> 10) & 15u;
    if (h->sf_index > 12u) return false;
    h->channel_config = (w >> 6) & 7u;
    h->bytes = ((w & 3u) << 11) | (((x >> 16) & 0xffu) << 3) | ((x >> 13) & 7u);
    if (h->bytes < h->header_bytes) return false;
    return (x & 3u) == 0u;
}
// A3 from one start position
TSP_HD bool five_from(const uint8_t* base, uint32_t n, uint32_t p, uint32_t* payload)
{
    uint64_t j = p;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < kRecogniseFrames; k++) {
        Hdr h;
        if (j + kRecogniseBytes > n || !header_at(base, n, j, &h)) return false;
        sum += h.bytes - h.header_bytes;
        j += h.bytes;
    }
    *payload = sum;
    return true;
}
TSP_HD void put_frame(const Stream& s, Frame* table, uint32_t k, uint32_t p, const Hdr& h, bool interrupted)
{
    if (k >= s.frame_capacity) return;
    Frame f = {};
    f.offset = p; f.bytes = h.bytes; f.flags = interrupted ? (uint32_t)kInterrupted : 0u;
    f.header_bytes = (uint8_t)h.header_bytes; f.profile = (uint8_t)h.profile; f.sf_index = (uint8_t)h.sf_index; f.channel_config = (uint8_t)h.channel_config;
    table[s.frame_first + k] = f;
}
TSP_HD void set_first(Result* r, uint32_t p, const Hdr& h)
{
    r->first_frame_offset = p; r->profile = (uint8_t)h.profile; r->sf_index = (uint8_t)h.sf_index; r->channel_config = (uint8_t)h.channel_config;
}
// A2 from `start`, serially: next(p) = the first position >= p with a valid header, or n - 6 where there is none (n >= 7 there).
// writes: this caller puts the records into the table (a wave walks the chain in step; one of its lanes writes).
template <typename Next>
TSP_HD void chain_from(const Stream& s, const uint8_t* base, uint32_t start, Frame* table, Next&& next, Result* r, bool writes = true)
{
    const uint32_t n = s.src_bytes;
    uint32_t p = start;
    bool interrupted = false;
    while ((uint64_t)p + kMinBytes <= n) {
        Hdr h;
        if (header_at(base, n, p, &h)) {
            if ((uint64_t)p + h.bytes > n) break;
            if (!r->frames && !(s.flags & kRecognise)) set_first(r, p, h);
            if (writes) put_frame(s, table, r->frames, p, h, interrupted);
            r->frames++;
            r->interruptions += interrupted;
            interrupted = false;
            p += h.bytes;
        } else {
            const uint32_t q = next(p + 1u);
            r->skipped_bytes += q - p;
            p = q;
            interrupted = true;
        }
    }
    r->bytes_consumed = p;
}
TSP_HD void walk(const Stream& s, const uint8_t* src, Frame* table, Result* out)
{
    const uint8_t* const base = src + s.src_offset;
    const uint32_t n = s.src_bytes;
    Result r = {};
    uint32_t start = 0;
    if (s.flags & kRecognise) {
        uint32_t payload = 0;
        while (start <= kLastStart && !five_from(base, n, start, &payload)) start++;
        if (start > kLastStart) { r.status = kNotAdts; *out = r; return; }
        Hdr h = {};
        header_at(base, n, start, &h);
        set_first(&r, start, h);
        r.mean_payload_bytes = payload / kRecogniseFrames;
    }
    auto next = [&](uint32_t p) {
        Hdr h;
        while ((uint64_t)p + kMinBytes <= n && !header_at(base, n, p, &h)) p++;
        return p;
    };
    chain_from(s, base, start, table, next, &r);
    *out = r;
}

// Host only: the ID3v2 tags at the head of a buffer
inline uint64_t id3v2_skip(const uint8_t* p, uint64_t n)
{
    uint64_t at = 0;
    while (n - at >= 10u) {
        const uint8_t* t = p + at;
        if (t[0] != 'I' || t[1] != 'D' || t[2] != '3' || t[3] == 0xff || t[4] == 0xff || ((t[6] | t[7] | t[8] | t[9]) & 0x80u)) break;
        at += 10u + (((uint64_t)t[6] << 21) | ((uint64_t)t[7] << 14) | ((uint64_t)t[8] << 7) | t[9]) + ((t[5] & 0x10u) ? 10u : 0u);
        if (at > n) break;
    }
    return at;
}

}  // namespace adts
