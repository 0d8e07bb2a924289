// cbcs_core.h -- the second protected fragmented MPEG-4 family (ohgpu_cbcs_*): schemes `cenc` and `cbcs`, tenc versions 0
// and 1 (the constant IV, the crypt:skip pattern), and a senc with subsample entries.  It stands on csrc/cenc_core.h and shares with it,
// without a copy, the walk and its protection policy (cenc::ProtectionT, here under the rules Parts), the forward cipher, read_iv and the
// counter block, the block loads and stores and the rows' places; the inverse cipher and both key schedules are csrc/raop_aes_core.h's.
// Written from FIPS-197 and the rules of include/ohgpu_cbcs.h.  Everything is __host__ __device__: csrc/cbcs_kernel.hip runs this text
// on the device, tests/cpp/cbcs_core_driver.cpp runs the same text on the CPU under the sanitizers, csrc/api_cbcs.hip runs the walk for
// ohgpu_cbcs_head.
//
//   the chain   a senc entry's place depends on the counts in front of it, so the entries of a traf are followed one after the other --
//               by the walk's own lane, at the traf's end, where they have to be followed anyway to hold them to the box and to the
//               samples' sizes.  On its way it writes a SubRow an entry (the entry's place in its sample, its clear and protected
//               bytes, the protected bytes of the sample in front of it -- the keystream offset --, the sample's work units in front
//               of it) and a SampleRec a sample (its first SubRow, their count, its IV's place, its units and cipher blocks).  Nothing
//               of either depends on where the sample lies, which only the expansion knows.  A sample without entries (no senc under a
//               constant IV, a senc without the flag, a count of 0) has no SubRow: it is one protected part.
//   capacity    the first sample whose entries do not fit what is left of subsample_capacity ends the rows served: rows_cap, which
//               stands where packet_capacity stands for the carries, the expansion and finish().
//   work units  a 16-byte piece of a part.  A clear part of C bytes has ceil(C / 16); a `cbcs` protected part of B bytes ceil(B / 16)
//               (whole blocks, then the tail); a `cenc` protected part is cut at the keystream's block edges: with o = the keystream
//               offset mod 16 it has ceil((o + B) / 16) pieces, the first of 16 - o bytes, and every piece pays for one keystream block.
//   a lane      unit_lane(): one unit of one sample.  cbcs_lane() computes the place of the encrypted block in front of its own from the
//               pattern, reads both, runs the inverse cipher and xors; ctr_part_lane() makes the piece's keystream block.  Whole
//               16-byte pieces are read as the aligned dwords that hold them and written by one 16-byte store at the destination's own
//               address; shorter ones go byte by byte.  No byte outside the sample's two ranges is written, and none is read outside
//               the aligned dwords that hold its source range.
#pragma once

#include "cenc_core.h"
#include "frag_units.h"

#define CBCS_HD MP4B_HD

namespace cbcs {

using mp4box::be16;
using mp4box::be32;
using mp4box::fourcc;
using mp4box::Box;
using mp4box::read_box;
using mp4box::Row;
using mp4frag::kInvalid;
using mp4frag::kNoKey;
using mp4frag::kNone;
using mp4frag::kOk;
using mp4frag::kUnsupported;
using mp4frag::Rec;
using mp4frag::RunRec;

constexpr uint32_t kSchemeCenc = 0x63656e63u, kSchemeCbcs = 0x63626373u, kLaneUnits = 64;
constexpr uint32_t kKeyWords = 2u * raopcore::kRoundKeyWords;       // a stream's schedules: the cipher's, then the inverse cipher's
enum Kind : uint32_t { kCopy = 0, kCtr = 1, kCbc = 2 };              // how a stream's protected parts are served

struct Stream {               // 120 bytes = ohgpu_cbcs_stream_desc
    cenc::Stream c;
    uint32_t sub_first, sub_capacity;
};
struct More {                 // 24 bytes: what ohgpu_cbcs_stream_result has behind ohgpu_cenc_stream_result's fields
    uint8_t  crypt, skip, civ_size, pad;
    uint32_t subsamples;
    uint8_t  civ[16];
};
struct Result { cenc::Result c; More m; };           // 232 bytes = ohgpu_cbcs_stream_result
struct SubRow {               // one senc entry (device scratch)
    uint32_t at;              // its clear part's first byte, from the sample's
    uint32_t clear, prot;
    uint32_t ks;              // the sample's protected bytes in front of it
    uint32_t unit_first;      // the sample's work units in front of it
};
struct SampleRec {            // one sample of a protected track (device scratch)
    uint32_t sub_first, n_sub;    // its entries, in the stream's share of the subsample table; none: one protected part
    uint32_t iv_pos;              // its IV, or the constant one, from the stream's first byte
    uint32_t units, blocks;       // of its entries (n_sub != 0)
};
static_assert(sizeof(Stream) == 120 && sizeof(More) == 24 && sizeof(Result) == 232 && sizeof(SubRow) == 20 && sizeof(SampleRec) == 20, "cbcs layouts");

// ---- the part arithmetic
CBCS_HD uint32_t pieces(uint32_t bytes) { return bytes / 16u + (bytes % 16u ? 1u : 0u); }
CBCS_HD bool patterned(uint32_t crypt, uint32_t skip) { return crypt != 0u && skip != 0u; }
// is whole block b of a `cbcs` part encrypted?
CBCS_HD bool encrypted(uint32_t b, uint32_t crypt, uint32_t skip) { return !patterned(crypt, skip) || b % (crypt + skip) < crypt; }
// the encrypted ones among a part's first `blocks` whole blocks
CBCS_HD uint32_t encrypted_of(uint32_t blocks, uint32_t crypt, uint32_t skip)
{
    if (!patterned(crypt, skip)) return blocks;
    const uint32_t period = crypt + skip, rest = blocks % period;
    return blocks / period * crypt + (rest < crypt ? rest : crypt);
}
CBCS_HD uint32_t prot_units(uint32_t kind, uint32_t prot, uint32_t ks) { return kind == kCtr ? (prot ? (uint32_t)(((uint64_t)(ks % 16u) + prot + 15u) / 16u) : 0u) : pieces(prot); }
CBCS_HD uint32_t prot_blocks(uint32_t kind, uint32_t prot, uint32_t ks, uint32_t crypt, uint32_t skip)
{
    return kind == kCtr ? prot_units(kind, prot, ks) : kind == kCbc ? encrypted_of(prot / 16u, crypt, skip) : 0u;
}
// a sample without entries: one part of the stream's kind (a clear track's: one clear part)
CBCS_HD SubRow whole_sample(uint32_t kind, uint32_t size)
{
    SubRow e = {};
    if (kind == kCopy) e.clear = size; else e.prot = size;
    return e;
}

// ---- the rules of cenc::ProtectionT: the schm, the tenc, and the chain of a traf's senc
struct Parts {
    // what the caller gives: the stream's share of the subsample table, its sample records (a row a packet row) and their counts
    SubRow*    subs;
    SampleRec* recs;
    uint32_t   sub_capacity, packet_capacity;
    // the tenc
    uint8_t  crypt, skip, civ_size;
    uint32_t civ_pos;
    // the chain
    uint32_t sub_used, rows_cap;          // entries written; the first sample whose entries found no room (kNone: none)
    bool     full;

    template <class G>
    MP4B_HD uint32_t kind_of(const G& g) const { return !g.is_protected ? (uint32_t)kCopy : g.scheme == kSchemeCbcs ? (uint32_t)kCbc : (uint32_t)kCtr; }

    template <class W, class G>
    MP4B_HD uint32_t judge_entry(W& w, G& g, uint64_t schm_at, uint64_t tenc_pay, uint64_t tenc_len)
    {
        const uint8_t* const p = w.p;
        crypt = skip = civ_size = 0; civ_pos = 0;
        if (g.scheme != kSchemeCenc && g.scheme != kSchemeCbcs) return w.fail(kUnsupported, schm_at);
        if (tenc_len < 24u) return w.fail(kInvalid, g.tenc_at);
        if (p[tenc_pay] > 1u) return w.fail(kUnsupported, g.tenc_at);
        const uint32_t pattern = p[tenc_pay] == 1u ? p[tenc_pay + 5] : 0u, prot = p[tenc_pay + 6], ivs = p[tenc_pay + 7];
        if (prot > 1u) return w.fail(kInvalid, g.tenc_at);
        g.is_protected = (uint8_t)prot; g.iv_size = 0;
        if (!prot) return kOk;
        uint32_t civ = 0;
        if (ivs == 0u) {
            if (tenc_len < 25u || tenc_len - 25u < p[tenc_pay + 24]) return w.fail(kInvalid, g.tenc_at);
            civ = p[tenc_pay + 24];
            if (civ != 8u && civ != 16u) return w.fail(kUnsupported, g.tenc_at);
        }
        if (g.scheme == kSchemeCenc) {
            if (pattern != 0u || (ivs != 8u && ivs != 16u)) return w.fail(kUnsupported, g.tenc_at);       // (a pattern under counter mode is `cens`)
        } else {
            if (ivs != 0u && ivs != 8u && ivs != 16u) return w.fail(kUnsupported, g.tenc_at);
            if ((pattern >> 4) == 0u && (pattern & 15u) != 0u) return w.fail(kUnsupported, g.tenc_at);
        }
        crypt = (uint8_t)(pattern >> 4); skip = (uint8_t)(pattern & 15u);
        g.iv_size = (uint8_t)ivs; civ_size = (uint8_t)civ; civ_pos = (uint32_t)(tenc_pay + 25u);
        return kOk;
    }

    // The end of a protected track's traf: its runs are [run0, w.n_runs), `n` samples in all, the stream's samples [w.samples - n, w.samples).
    template <class W, class G>
    MP4B_HD uint32_t judge_traf(W& w, G& g, uint64_t traf, uint32_t run0, uint32_t n)
    {
        const uint8_t* const p = w.p;
        const uint32_t kind = kind_of(g), first = (uint32_t)(w.samples - n);
        bool entries = false;
        uint64_t pos = 0, end = 0;
        if (!g.have_senc) {
            if (!n) return kOk;
            if (g.iv_size) return w.fail(kUnsupported, traf);             // (its IVs may lie in saiz / saio, which are not read)
        } else {
            if (g.senc_len < 8u) return w.fail(kInvalid, g.senc_at);
            const uint32_t head = be32(p, g.senc_pay), count = be32(p, g.senc_pay + 4);
            if ((head >> 24) != 0u || (head & 1u)) return w.fail(kUnsupported, g.senc_at);
            if (count != n) return w.fail(kInvalid, g.senc_at);
            entries = (head & 2u) != 0u;
            pos = g.senc_pay + 8u; end = g.senc_pay + g.senc_len;
        }
        // the traf's truns again, for the samples' sizes: the walk held them to the traf and keeps a record only of the runs within
        // run_capacity, and the parts of EVERY sample must sum to its size
        Box tb;
        (void)read_box(p, traf, w.n, false, &tb);
        uint64_t child = traf + tb.header;
        const uint64_t traf_stop = traf + tb.size;
        RunRec run = {};
        uint32_t begun = 0, in_run = 0;
        for (uint32_t i = 0; i < n; i++) {
            MP4B_STEP(1);
            while (in_run == run.samples) {                               // the next trun that has samples (there is one: n is their sum)
                Box c;
                if (read_box(p, child, traf_stop, false, &c) != 1) return w.fail(kInvalid, traf);
                const uint64_t q = child + c.header;
                child += c.size;
                if (c.type != fourcc('t', 'r', 'u', 'n')) continue;
                const uint32_t fl = be32(p, q) & 0xffffffu, count = be32(p, q + 4);
                if (!count) continue;
                RunRec r = {};
                r.size_at = kNone;
                if (fl & 0x100u) r.stride += 4u;
                if (fl & 0x200u) { r.size_at = r.stride; r.stride += 4u; }
                if (fl & 0x400u) r.stride += 4u;
                if (fl & 0x800u) r.stride += 4u;
                r.entries_pos = (uint32_t)(q + 8u + ((fl & 1u) ? 4u : 0u) + ((fl & 4u) ? 4u : 0u));
                r.samples = count; r.def_size = w.traf_def_size;
                run = r; begun++; in_run = 0;
            }
            const bool known = run0 + begun - 1u < w.run_capacity;        // a run with a record: its samples can be served
            const uint32_t s = first + i;
            uint32_t iv_at = civ_pos, count = 0;
            if (g.have_senc) {
                if (g.iv_size) {
                    if (end - pos < g.iv_size) return w.fail(kInvalid, g.senc_at);
                    iv_at = (uint32_t)pos; pos += g.iv_size;
                }
                if (entries) {
                    if (end - pos < 2u) return w.fail(kInvalid, g.senc_at);
                    count = be16(p, pos); pos += 2u;
                    if ((end - pos) / 6u < count) return w.fail(kInvalid, g.senc_at);
                }
            }
            const bool room = !full && count <= sub_capacity - sub_used;
            if (!room && !full) { full = true; rows_cap = s; }
            const bool keep = known && room && s < packet_capacity;
            uint64_t total = 0;
            uint32_t ks = 0, units = 0, blocks = 0;
            for (uint32_t e = 0; e < count; e++, pos += 6u) {
                MP4B_STEP(1);
                SubRow row;
                row.at = (uint32_t)total; row.clear = be16(p, pos); row.prot = be32(p, pos + 2); row.ks = ks; row.unit_first = units;
                if (keep) subs[sub_used + e] = row;
                units += pieces(row.clear) + prot_units(kind, row.prot, ks); blocks += prot_blocks(kind, row.prot, ks, crypt, skip);
                ks += row.prot; total += (uint64_t)row.clear + row.prot;
            }
            if (count && total != mp4frag::entry_size(p, run, in_run)) return w.fail(kInvalid, g.senc_at);
            if (keep) {
                SampleRec rec;
                rec.sub_first = sub_used; rec.n_sub = count; rec.iv_pos = iv_at; rec.units = units; rec.blocks = blocks;
                recs[s] = rec;
                sub_used += count;
            }
            in_run++;
        }
        return kOk;
    }
};
using Protection = cenc::ProtectionT<Parts>;

// One stream: mp4frag::walk_into under Protection; what the protection boxes gave; the rows the later phases serve (*rows_cap).
// subs: the stream's share of the subsample table; samples: its sample records (neither is touched by a head_only walk).
CBCS_HD void walk(const Stream& s, const uint8_t* base, bool head_only, SubRow* subs, SampleRec* samples, mp4frag::Result* out, cenc::Extra* x, More* more, Rec* rec,
                  RunRec* runs, uint32_t* rows_cap)
{
    mp4frag::WalkT<Protection> w = {};
    Protection& g = w.prot;
    g.key_flags = s.c.key_flags; g.want_kid = s.c.kid;
    g.subs = subs; g.recs = samples; g.sub_capacity = s.sub_capacity; g.packet_capacity = s.c.s.packet_capacity; g.rows_cap = kNone;
    mp4frag::walk_into(w, s.c.s, base, head_only, out, rec, runs);
    cenc::Extra e = {};
    More m = {};
    if (out->status == kOk || out->status == kNoKey) {
        e.entry = g.entry_type ? g.entry_type : w.codec; e.scheme = g.scheme; e.is_protected = g.is_protected; e.iv_size = g.iv_size;
        for (int k = 0; k < 16; k++) e.kid[k] = g.kid[k];
        m.crypt = g.crypt; m.skip = g.skip; m.civ_size = g.civ_size; m.subsamples = g.sub_used;
        for (uint32_t k = 0; k < g.civ_size; k++) m.civ[k] = base[g.civ_pos + k];
    }
    *x = e; *more = m;
    *rows_cap = g.rows_cap < s.c.s.packet_capacity ? g.rows_cap : s.c.s.packet_capacity;
}
CBCS_HD uint32_t kind_of(const cenc::Extra& x) { return !x.is_protected ? (uint32_t)kCopy : x.scheme == kSchemeCbcs ? (uint32_t)kCbc : (uint32_t)kCtr; }

// ---- a unit on its way
struct SampleIv { cenc::Iv ctr; uint32_t cbc[4]; };          // the counter's reading, and the CBC IV's (8 bytes: the first half, the rest zero)
CBCS_HD SampleIv read_sample_iv(const uint8_t* p, uint64_t at, uint32_t bytes)
{
    SampleIv v;
    v.ctr = cenc::read_iv(p, at, bytes);
    v.cbc[0] = v.ctr.w0; v.cbc[1] = v.ctr.w1;
    v.cbc[2] = bytes == 16u ? fieldbytes::le32(p, at + 8) : 0u; v.cbc[3] = bytes == 16u ? fieldbytes::le32(p, at + 12) : 0u;
    return v;
}
struct Tables { const uint32_t* te0; const uint32_t* td0; const uint8_t* isbox; };

CBCS_HD void copy_piece(const uint8_t* in, uint8_t* out, uint32_t n)
{
    if (n == 16u) {
        uint32_t c[4];
        cenc::load_block(in, c);
        cenc::store_block(out, c);
        return;
    }
    for (uint32_t k = 0; k < n; k++) out[k] = in[k];
}

// Piece b of a `cbcs` protected part of `prot` bytes at `in` (16 b < prot).  rk: the inverse cipher's schedule.
CBCS_HD void cbcs_lane(const uint8_t* in, uint8_t* out, uint32_t prot, uint32_t b, uint32_t crypt, uint32_t skip, const uint32_t* rk, const uint32_t iv[4], const Tables& t)
{
    const uint64_t at = 16ull * b;
    const uint32_t n = prot - at < 16u ? (uint32_t)(prot - at) : 16u;
    if (n < 16u || !encrypted(b, crypt, skip)) { copy_piece(in + at, out + at, n); return; }
    // the encrypted block in front of it: block b is the k-th encrypted one, k = (b / period) crypt + b % period
    uint32_t c[4], prev[4], clear[4];
    bool chained = b != 0u;
    uint64_t prev_at = at - 16u;
    if (patterned(crypt, skip)) {
        const uint32_t period = crypt + skip, k = b / period * crypt + b % period;
        chained = k != 0u;
        if (chained) prev_at = 16ull * ((k - 1u) / crypt * period + (k - 1u) % crypt);
    }
    cenc::load_block(in + at, c);
    if (chained) cenc::load_block(in + prev_at, prev);
    else for (int k = 0; k < 4; k++) prev[k] = iv[k];
    raopcore::decrypt_block(rk, c, clear, t.td0, t.isbox);
    for (int k = 0; k < 4; k++) clear[k] ^= prev[k];
    cenc::store_block(out + at, clear);
}

// Piece v of a `cenc` protected part of `prot` bytes at `in` whose first byte uses keystream byte `ks` of the sample.  w: the cipher's schedule.
CBCS_HD void ctr_part_lane(const uint8_t* in, uint8_t* out, uint32_t prot, uint32_t ks, uint32_t v, const uint32_t* w, const cenc::Iv& iv, const uint32_t* te0)
{
    const uint32_t first = ks % 16u;
    const uint64_t a = v ? 16ull * v - first : 0u, edge = 16ull * (v + 1u) - first, b = edge < prot ? edge : prot;
    const uint32_t n = (uint32_t)(b - a), off = v ? 0u : first;
    uint32_t c[4], stream[4];
    cenc::counter_block(iv, (uint64_t)(ks / 16u) + v, c);
    cenc::encrypt_block(w, c, stream, te0);
    if (n == 16u) {
        cenc::load_block(in + a, c);
        for (int k = 0; k < 4; k++) c[k] ^= stream[k];
        cenc::store_block(out + a, c);
        return;
    }
    for (uint32_t k = 0; k < n; k++) out[a + k] = (uint8_t)(in[a + k] ^ (stream[(off + k) / 4u] >> (8u * ((off + k) % 4u))));
}

// Unit v of entry e of a sample that lies at `in` and goes to `out`.  keys: the stream's two schedules.
CBCS_HD void unit_lane(const uint8_t* in, uint8_t* out, const SubRow& e, uint32_t v, uint32_t kind, uint32_t crypt, uint32_t skip, const uint32_t* keys, const SampleIv& iv,
                       const Tables& t)
{
    const uint32_t clear_units = pieces(e.clear);
    if (v < clear_units) {
        const uint32_t at = 16u * v, n = e.clear - at < 16u ? e.clear - at : 16u;
        copy_piece(in + e.at + at, out + e.at + at, n);
        return;
    }
    const uint64_t part = (uint64_t)e.at + e.clear;
    if (kind == kCbc) cbcs_lane(in + part, out + part, e.prot, v - clear_units, crypt, skip, keys + raopcore::kRoundKeyWords, iv.cbc, t);
    else ctr_part_lane(in + part, out + part, e.prot, e.ks, v - clear_units, keys, iv.ctr, t.te0);
}

// The units and the cipher blocks of gathered row `row` of `size` bytes.
CBCS_HD void sample_work(uint32_t kind, const More& m, const SampleRec* samples, uint32_t row, uint32_t size, uint32_t* units, uint32_t* blocks)
{
    if (kind != kCopy && samples[row].n_sub) { *units = samples[row].units; *blocks = samples[row].blocks; return; }
    *units = pieces(size);                                    // (one part, from keystream offset 0)
    *blocks = prot_blocks(kind, size, 0u, m.crypt, m.skip);
}

// The plain route, after mp4frag::finish(): the public rows, the count of cipher blocks, and every gathered sample on its way, one
// unit after the other.  cs: the descriptor; src_rows: the expansion's rows; subs, samples: the walk's, the stream's own.
CBCS_HD void gather_serial(const Stream& cs, const uint8_t* src, uint8_t* dst, const Rec& rec, const RunRec* runs, const Row* src_rows, const mp4frag::Result& r,
                           const uint32_t* keys, const Tables& t, const SubRow* subs, const SampleRec* samples, const More& m, Row* rows, cenc::Extra* x)
{
    const mp4frag::Stream& s = cs.c.s;
    const uint32_t kind = kind_of(*x), iv_bytes = x->iv_size ? x->iv_size : m.civ_size;
    uint64_t at = s.dst_offset, blocks = 0;
    for (uint32_t row = 0; row < rec.rows; row++) {
        MP4B_STEP(2);
        Row out;
        out.src_offset = s.dst_offset; out.bytes = 0; out.reserved = 0;
        if (cenc::gathered_row(s, r, row)) {
            const uint32_t size = src_rows[row].bytes;
            out.src_offset = at; out.bytes = size;
            uint32_t units, mine;
            sample_work(kind, m, samples, row, size, &units, &mine);
            SampleIv iv = {};
            if (kind != kCopy) iv = read_sample_iv(src + s.src_offset, samples[row].iv_pos, iv_bytes);
            const uint32_t n_sub = kind != kCopy ? samples[row].n_sub : 0u;
            const SubRow whole = whole_sample(kind, size);
            for (uint32_t e = 0; e < (n_sub ? n_sub : 1u); e++) {
                const SubRow& sub = n_sub ? subs[samples[row].sub_first + e] : whole;
                const uint32_t n = pieces(sub.clear) + prot_units(kind, sub.prot, sub.ks);
                for (uint32_t v = 0; v < n; v++) unit_lane(src + src_rows[row].src_offset, dst + at, sub, v, kind, m.crypt, m.skip, keys, iv, t);
            }
            at += size; blocks += mine;
        }
        rows[row] = out;
    }
    x->blocks = blocks;
}

// The entry of a sample that holds its unit u (n_sub != 0): the last whose unit_first is <= u.
CBCS_HD uint32_t entry_of(const SubRow* subs, uint32_t n_sub, uint32_t u)
{
    return fragu::last_le(0u, n_sub, u, [subs](uint32_t k) { MP4B_STEP(3); return subs[k].unit_first; });
}

}  // namespace cbcs
