// cenc_core.h -- Common Encryption (`cenc`: AES-128 in counter mode) in front of the FLAC and Apple Lossless decoders:
// what stands between the bytes of a protected fragmented MPEG-4 stream and the clear, contiguous run of its samples.  The walk, the
// totals, the carries, the expansion and finish() are csrc/mp4_frag_core.h's, run with the policy below in place of mp4frag::Clear; the
// AES tables' field arithmetic and the key schedule are csrc/raop_aes_core.h's.  Written from FIPS-197 and the rules of
// include/ohgpu_cenc.h.  Everything is __host__ __device__: csrc/cenc_kernel.hip runs this text on the device, tests/cpp/cenc_core_driver.cpp runs
// the same text on the CPU under the sanitizers, csrc/api_cenc.hip runs the walk for ohgpu_cenc_head.
//
//   cipher      the forward cipher: AddRoundKey(w[0]); nine rounds of SubBytes, ShiftRows, MixColumns, AddRoundKey(w[r]); then SubBytes,
//               ShiftRows, AddRoundKey(w[10]).  A column is one 32-bit word read little-endian, as in raop_aes_core.h.  A round's first
//               three steps are four table reads a column: Te0[x] = MixColumns of the column (Sbox[x], 0, 0, 0) = (2s, s, s, 3s); the
//               tables of rows 1..3 are Te0 rotated left by 8, 16 and 24 bits, so only Te0 is kept, and its second byte IS the S-box,
//               which the last round takes from it.
//   counter     block j of a sample: bytes 0..7 the IV's, bytes 8..15 the big-endian (L + j) mod 2^64, L the IV's second half (0 for an
//               8-byte IV).  The low half wraps and carries nowhere.
//   protection  Protection below: `enca` > sinf > frma, schm, schi > tenc in moov; senc, sbgp, sgpd in a traf.  What a traf's boxes say
//               is judged at the traf's end, since senc may stand anywhere among its siblings: a seig grouping first, then the senc.
//   the rows    the public packet rows point into the destination arena; gather_serial() has the rule, and the count of keystream blocks.
//   a lane      crypt_lane(): block j of one sample, from any source address to any destination address.  A whole block is read as the
//               aligned dwords that hold it, funnelled, and written by one 16-byte store at the destination's own address; the last,
//               partial block goes byte by byte.  No byte outside the sample's two ranges is written, and none is read outside the
//               aligned dwords that hold its source range.
#pragma once

#include <stddef.h>

#include "mp4_frag_core.h"
#include "raop_aes_core.h"

#define CENC_HD MP4B_HD

namespace cenc {

using mp4box::be32;
using mp4box::be64;
using mp4box::Box;
using mp4box::fourcc;
using mp4box::read_box;
using mp4box::Row;
using mp4frag::kInvalid;
using mp4frag::kNoKey;
using mp4frag::kNone;
using mp4frag::kOk;
using mp4frag::kUnsupported;
using mp4frag::Rec;
using mp4frag::RunRec;

constexpr uint32_t kHaveKey = 1, kScheduleWords = raopcore::kRoundKeyWords, kLaneBlocks = 64;

struct Stream {               // 112 bytes = ohgpu_cenc_stream_desc
    mp4frag::Stream s;
    uint32_t key_flags, reserved[3];
    uint8_t  kid[16], key[16];
};
struct Extra {                // 40 bytes: what ohgpu_cenc_stream_result has behind ohgpu_mp4f_stream_result's fields
    uint32_t entry, scheme;
    uint8_t  is_protected, iv_size, pad[2];
    uint32_t reserved;
    uint8_t  kid[16];
    uint64_t blocks;
};
struct Result { mp4frag::Result r; Extra x; };       // 208 bytes = ohgpu_cenc_stream_result
struct RowRec {               // what the decrypt-gather keeps of one sample row (device scratch)
    uint64_t block_first;     // the keystream blocks of the tile's rows in front of it
    uint32_t iv_pos, pad;     // its IV, from the stream's first byte
};
static_assert(sizeof(Stream) == 112 && sizeof(Extra) == 40 && sizeof(Result) == 208 && sizeof(RowRec) == 16, "protected MPEG-4 layouts");

// ---- the cipher
struct Forward { uint32_t te0[256]; };
constexpr Forward make_forward()
{
    const raopcore::Tables t = raopcore::make_tables();
    Forward f = {};
    for (int x = 0; x < 256; x++) {
        const uint8_t s = t.sbox[x];
        f.te0[x] = (uint32_t)raopcore::gf_mul(s, 2) | ((uint32_t)s << 8) | ((uint32_t)s << 16) | ((uint32_t)raopcore::gf_mul(s, 3) << 24);
    }
    return f;
}

CENC_HD uint32_t rotl32(uint32_t v, uint32_t n) { return (v << n) | (v >> (32u - n)); }
// SubBytes + ShiftRows + MixColumns of one output column: row r comes from column (c + r) mod 4, here a, b, c, d in that order
CENC_HD uint32_t round_column(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const uint32_t* te0)
{
    return te0[a & 0xffu] ^ rotl32(te0[(b >> 8) & 0xffu], 8) ^ rotl32(te0[(c >> 16) & 0xffu], 16) ^ rotl32(te0[d >> 24], 24);
}
CENC_HD uint32_t last_column(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const uint32_t* te0)
{
    return ((te0[a & 0xffu] >> 8) & 0xffu) | (te0[(b >> 8) & 0xffu] & 0xff00u) | ((te0[(c >> 16) & 0xffu] & 0xff00u) << 8) | ((te0[d >> 24] & 0xff00u) << 16);
}
// w: the cipher's schedule (raopcore::expand_encrypt_key)
CENC_HD void encrypt_block(const uint32_t* w, const uint32_t in[4], uint32_t out[4], const uint32_t* te0)
{
    uint32_t s0 = in[0] ^ w[0], s1 = in[1] ^ w[1], s2 = in[2] ^ w[2], s3 = in[3] ^ w[3];
    for (int r = 1; r < 10; r++) {
        const uint32_t t0 = round_column(s0, s1, s2, s3, te0) ^ w[4 * r];
        const uint32_t t1 = round_column(s1, s2, s3, s0, te0) ^ w[4 * r + 1];
        const uint32_t t2 = round_column(s2, s3, s0, s1, te0) ^ w[4 * r + 2];
        const uint32_t t3 = round_column(s3, s0, s1, s2, te0) ^ w[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    out[0] = last_column(s0, s1, s2, s3, te0) ^ w[40];
    out[1] = last_column(s1, s2, s3, s0, te0) ^ w[41];
    out[2] = last_column(s2, s3, s0, s1, te0) ^ w[42];
    out[3] = last_column(s3, s0, s1, s2, te0) ^ w[43];
}

// ---- the counter
struct Iv { uint32_t w0, w1; uint64_t low; };        // bytes 0..7 as two little-endian words; L
CENC_HD Iv read_iv(const uint8_t* p, uint64_t at, uint32_t iv_size)
{
    Iv v;
    v.w0 = fieldbytes::le32(p, at); v.w1 = fieldbytes::le32(p, at + 4);
    v.low = iv_size == 16u ? be64(p, at + 8) : 0u;
    return v;
}
CENC_HD void counter_block(const Iv& v, uint64_t j, uint32_t c[4])
{
    const uint64_t low = v.low + j;                   // modulo 2^64: no carry into the IV's first half
    c[0] = v.w0; c[1] = v.w1;
    c[2] = __builtin_bswap32((uint32_t)(low >> 32)); c[3] = __builtin_bswap32((uint32_t)low);
}

// ---- a block on its way
#if defined(__HIP_DEVICE_COMPILE__) || defined(OHGPU_ALIGNED_READS)
CENC_HD void load_block(const uint8_t* a, uint32_t c[4])
{
    const uint32_t shift = (uint32_t)((uintptr_t)a & 3u) * 8u;
    const uint32_t* w = (const uint32_t*)((uintptr_t)a & ~(uintptr_t)3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
    if (!shift) { c[0] = w0; c[1] = w1; c[2] = w2; c[3] = w3; return; }
    const uint32_t w4 = w[4];                         // (it holds the block's last bytes)
    c[0] = (w0 >> shift) | (w1 << (32u - shift)); c[1] = (w1 >> shift) | (w2 << (32u - shift));
    c[2] = (w2 >> shift) | (w3 << (32u - shift)); c[3] = (w3 >> shift) | (w4 << (32u - shift));
}
#else
CENC_HD void load_block(const uint8_t* a, uint32_t c[4]) { __builtin_memcpy(c, a, 16); }
#endif
CENC_HD void store_block(uint8_t* a, const uint32_t c[4]) { __builtin_memcpy(a, c, 16); }     // at the destination's own address

// Block j of a sample of `size` bytes (16 j < size) that lies at `in` and goes to `out`.  w: the stream's schedule, or null for a
// clear track, whose bytes are moved as they are.
CENC_HD void crypt_lane(const uint8_t* in, uint8_t* out, uint32_t size, uint32_t j, const uint32_t* w, const Iv& iv, const uint32_t* te0)
{
    uint32_t ks[4] = {0u, 0u, 0u, 0u};
    if (w) {
        uint32_t c[4];
        counter_block(iv, j, c);
        encrypt_block(w, c, ks, te0);
    }
    const uint64_t at = 16ull * j;
    const uint32_t n = size - at < 16u ? (uint32_t)(size - at) : 16u;
    if (n == 16u) {
        uint32_t c[4];
        load_block(in + at, c);
        for (int k = 0; k < 4; k++) c[k] ^= ks[k];
        store_block(out + at, c);
        return;
    }
    for (uint32_t k = 0; k < 4u; k++)                 // the keystream's leading bytes
        for (uint32_t b = 0; b < 4u; b++)
            if (4u * k + b < n) out[at + 4u * k + b] = (uint8_t)(in[at + 4u * k + b] ^ (ks[k] >> (8u * b)));
}

// ---- the protection boxes: the policy of mp4frag::WalkT.  What differs between the families that read them -- which schemes and
// which `tenc` are served, and what a traf's `senc` must hold -- is the Rules': Whole, below, is this family's (`cenc`, whole samples,
// an IV a sample); csrc/cbcs_core.h has the rules of ohgpu_cbcs_*.  Everything else is shared text.
template <class Rules>
struct ProtectionT : Rules {
    static constexpr bool kAdmits = true;
    // what the caller gives: the descriptor's key_flags and kid; head_only walks ask for no key
    uint32_t key_flags;
    const uint8_t* want_kid;
    // the trak in hand (the last one read is the taken one)
    uint32_t entry_type, scheme;          // `enca` and its scheme type; 0 and 0 for a plain entry
    uint8_t  is_protected, iv_size, kid[16];
    uint64_t tenc_at;
    // the traf in hand
    bool     have_senc, have_seig;
    uint64_t senc_at, senc_pay, senc_len, seig_at;

    MP4B_HD void trak_begin()
    {
        entry_type = scheme = 0; is_protected = iv_size = 0; tenc_at = 0;
        for (int k = 0; k < 16; k++) kid[k] = 0;
    }

    // the header of the child box at pos of [pos, end), counted: false with the walk's err_at set
    template <class W>
    MP4B_HD bool child(W& w, uint64_t pos, uint64_t end, uint32_t* seen, Box* k)
    {
        MP4B_STEP(0);
        if (++*seen <= mp4box::kMaxBoxes && read_box(w.p, pos, end, false, k) == 1 && k->size <= end - pos) return true;
        (void)w.fail(kInvalid, pos);
        return false;
    }

    // The `enca` entry at `entry`: its payload [q, entry_end).  Every child is walked and counted before anything is judged.
    template <class W>
    MP4B_HD uint32_t entry(W& w, uint64_t entry, uint64_t q, uint64_t entry_end, bool* parsed)
    {
        const uint8_t* const p = w.p;
        entry_type = fourcc('e', 'n', 'c', 'a');
        if (entry_end - q < 28u) return w.fail(kInvalid, entry);
        w.channels = mp4box::be16(p, q + 16); w.bits = mp4box::be16(p, q + 18); w.rate = mp4box::be16(p, q + 24);
        uint32_t seen = 1;                // (the entry itself)
        bool have_sinf = false, have_frma = false, have_schm = false, have_tenc = false, have_dfla = false, have_alac = false;
        uint64_t frma_at = 0, frma_pay = 0, frma_len = 0, schm_at = 0, schm_pay = 0, schm_len = 0, tenc_pay = 0, tenc_len = 0, dfla_at = 0, alac_at = 0;
        Box dfla = {}, alac = {};
        for (uint64_t c = q + 28u; entry_end - c >= 8u;) {
            Box k;
            if (!child(w, c, entry_end, &seen, &k)) return kInvalid;
            const uint64_t end = c + k.size;
            if (k.type == fourcc('s', 'i', 'n', 'f') && !have_sinf) {
                have_sinf = true;
                bool have_schi = false;
                for (uint64_t c2 = c + k.header; end - c2 >= 8u;) {
                    Box k2;
                    if (!child(w, c2, end, &seen, &k2)) return kInvalid;
                    const uint64_t pay2 = c2 + k2.header, len2 = k2.size - k2.header;
                    if (k2.type == fourcc('f', 'r', 'm', 'a') && !have_frma) { have_frma = true; frma_at = c2; frma_pay = pay2; frma_len = len2; }
                    else if (k2.type == fourcc('s', 'c', 'h', 'm') && !have_schm) { have_schm = true; schm_at = c2; schm_pay = pay2; schm_len = len2; }
                    else if (k2.type == fourcc('s', 'c', 'h', 'i') && !have_schi) {
                        have_schi = true;
                        for (uint64_t c3 = pay2; pay2 + len2 - c3 >= 8u;) {
                            Box k3;
                            if (!child(w, c3, pay2 + len2, &seen, &k3)) return kInvalid;
                            if (k3.type == fourcc('t', 'e', 'n', 'c') && !have_tenc) { have_tenc = true; tenc_at = c3; tenc_pay = c3 + k3.header; tenc_len = k3.size - k3.header; }
                            c3 += k3.size;
                        }
                    }
                    c2 += k2.size;
                }
            } else if (k.type == fourcc('d', 'f', 'L', 'a') && !have_dfla) { have_dfla = true; dfla_at = c; dfla = k; }
            else if (k.type == fourcc('a', 'l', 'a', 'c') && !have_alac) { have_alac = true; alac_at = c; alac = k; }
            c = end;
        }
        if (!have_sinf || !have_frma || !have_schm || !have_tenc) return w.fail(kInvalid, entry);
        if (frma_len < 4u) return w.fail(kInvalid, frma_at);
        if (schm_len < 12u) return w.fail(kInvalid, schm_at);
        scheme = be32(p, schm_pay + 4);
        const uint32_t judged = Rules::judge_entry(w, *this, schm_at, tenc_pay, tenc_len);      // the scheme and the tenc: is_protected, iv_size
        if (judged != kOk) return judged;
        for (uint32_t k = 0; k < 16u; k++) kid[k] = p[tenc_pay + 8u + k];
        // the original format's own children, with the clear entry's rules
        w.codec = be32(p, frma_pay);
        if (w.codec == fourcc('a', 'l', 'a', 'c')) {
            if (!have_alac) return w.fail(kUnsupported, entry);
            mp4box::Walk b;
            b.p = p; b.n = w.n; b.visited = 0; b.err_at = 0;
            mp4box::Track fresh = {};
            b.tr = fresh;
            const uint32_t st = b.alac_box(alac_at, alac);
            if (st != kOk) return w.fail(st, b.err_at);
            w.cfg = b.tr.cfg; w.limit = b.tr.t.packet_limit;
            *parsed = true;
            return kOk;
        }
        if (w.codec != fourcc('f', 'L', 'a', 'C') || !(w.mask & mp4frag::kCodecFlac)) return kOk;
        if (!have_dfla) return w.fail(kUnsupported, entry);
        *parsed = true;
        return w.dfla(dfla_at, dfla_at + dfla.header, dfla.size - dfla.header);
    }

    template <class W>
    MP4B_HD uint32_t after_moov(W& w)
    {
        if (!is_protected) return kOk;
        bool mine = (key_flags & kHaveKey) != 0u;
        for (uint32_t k = 0; k < 16u && mine; k++) mine = want_kid[k] == kid[k];
        return mine ? (uint32_t)kOk : w.fail(kNoKey, tenc_at);
    }

    MP4B_HD void traf_begin() { have_senc = have_seig = false; }
    template <class W>
    MP4B_HD void traf_box(W& w, uint32_t type, uint64_t at, uint64_t q, uint64_t m)
    {
        if (type == fourcc('s', 'e', 'n', 'c') && !have_senc) { have_senc = true; senc_at = at; senc_pay = q; senc_len = m; }
        const bool group = type == fourcc('s', 'b', 'g', 'p') || type == fourcc('s', 'g', 'p', 'd');
        if (group && !have_seig && m >= 8u && be32(w.p, q + 4) == fourcc('s', 'e', 'i', 'g')) { have_seig = true; seig_at = at; }
    }
    // The end of a traf of the taken track: its runs are [run0, w.n_runs), `n` samples in all.
    template <class W>
    MP4B_HD uint32_t traf_end(W& w, uint64_t traf, uint32_t run0, uint32_t n)
    {
        if (have_seig) return w.fail(kUnsupported, seig_at);
        if (!is_protected) return kOk;
        return Rules::judge_traf(w, *this, traf, run0, n);
    }
};

// This family's rules: scheme `cenc`, tenc version 0, an IV of 8 or 16 bytes a sample, a senc of IVs alone.
struct Whole {
    template <class W, class G>
    MP4B_HD uint32_t judge_entry(W& w, G& g, uint64_t schm_at, uint64_t tenc_pay, uint64_t tenc_len)
    {
        const uint8_t* const p = w.p;
        if (g.scheme != fourcc('c', 'e', 'n', 'c')) return w.fail(kUnsupported, schm_at);
        if (tenc_len < 24u) return w.fail(kInvalid, g.tenc_at);
        if (p[tenc_pay] != 0u) return w.fail(kUnsupported, g.tenc_at);
        const uint32_t prot = p[tenc_pay + 6], ivs = p[tenc_pay + 7];
        if (prot > 1u) return w.fail(kInvalid, g.tenc_at);
        if (prot == 1u && ivs != 8u && ivs != 16u) return w.fail(kUnsupported, g.tenc_at);
        g.is_protected = (uint8_t)prot; g.iv_size = (uint8_t)(prot ? ivs : 0u);
        return kOk;
    }
    // the end of a protected track's traf that has no seig grouping
    template <class W, class G>
    MP4B_HD uint32_t judge_traf(W& w, G& g, uint64_t traf, uint32_t run0, uint32_t n)
    {
        if (!g.have_senc) return n ? w.fail(kUnsupported, traf) : (uint32_t)kOk;
        if (g.senc_len < 8u) return w.fail(kInvalid, g.senc_at);
        const uint32_t head = be32(w.p, g.senc_pay), count = be32(w.p, g.senc_pay + 4);
        if ((head >> 24) != 0u || (head & 3u)) return w.fail(kUnsupported, g.senc_at);
        if (count > (g.senc_len - 8u) / g.iv_size || count != n) return w.fail(kInvalid, g.senc_at);
        uint64_t before = 0;
        for (uint32_t k = run0; k < w.n_runs && k < w.run_capacity; k++) {
            MP4B_STEP(1);
            w.runs[k].iv_pos = (uint32_t)(g.senc_pay + 8u + before * g.iv_size);
            before += w.runs[k].samples;
        }
        return kOk;
    }
};
using Protection = ProtectionT<Whole>;

// One stream: mp4frag::walk_into under Protection, and what the protection boxes gave.
CENC_HD void walk(const Stream& s, const uint8_t* base, bool head_only, mp4frag::Result* out, Extra* x, Rec* rec, RunRec* runs)
{
    mp4frag::WalkT<Protection> w = {};
    w.prot.key_flags = s.key_flags; w.prot.want_kid = s.kid;
    mp4frag::walk_into(w, s.s, base, head_only, out, rec, runs);
    Extra e = {};
    if (out->status == kOk || out->status == kNoKey) {
        const Protection& g = w.prot;
        e.entry = g.entry_type ? g.entry_type : w.codec; e.scheme = g.scheme; e.is_protected = g.is_protected; e.iv_size = g.iv_size;
        for (int k = 0; k < 16; k++) e.kid[k] = g.kid[k];
    }
    *x = e;
}

// ---- the rows
CENC_HD bool gathered_row(const mp4frag::Stream& s, const mp4frag::Result& r, uint32_t row) { return r.bytes_gathered != 0u && row >= s.gather_first_row && row < r.samples_available; }
CENC_HD uint32_t blocks_of(uint32_t bytes) { return bytes / 16u + (bytes % 16u ? 1u : 0u); }
// The place in the destination arena of gathered row `row`, which lies in run `k`: the gather's own arithmetic (mp4frag::piece_of).
CENC_HD uint64_t row_place(const mp4frag::Stream& s, const Rec& rec, const RunRec* runs, uint32_t k, const Row& src)
{
    const int64_t in_run = (int64_t)(src.src_offset - s.src_offset) - runs[k].place;
    return s.dst_offset + (runs[k].gathered - runs[rec.gather_run].gathered) + (uint64_t)(in_run - rec.gather_skip);
}

// The plain route, after mp4frag::finish(): the public rows, the count of keystream blocks, and every gathered sample on its way, one
// block after the other.  src_rows: the expansion's rows (places in the source arena); `src` and `dst`: the arenas' first bytes;
// w: the stream's schedule.
CENC_HD void gather_serial(const Stream& cs, const uint8_t* src, uint8_t* dst, const Rec& rec, const RunRec* runs, const Row* src_rows, const mp4frag::Result& r,
                           const uint32_t* w, const uint32_t* te0, Row* rows, Extra* x)
{
    const mp4frag::Stream& s = cs.s;
    const bool prot = x->is_protected != 0u;
    uint64_t at = s.dst_offset, blocks = 0;
    uint32_t k = 0;
    for (uint32_t row = 0; row < rec.rows; row++) {
        MP4B_STEP(2);
        Row out;
        out.src_offset = s.dst_offset; out.bytes = 0; out.reserved = 0;
        if (gathered_row(s, r, row)) {
            while (row >= runs[k].first_sample + runs[k].samples) k++;
            const uint32_t size = src_rows[row].bytes, n = blocks_of(size);
            out.src_offset = at; out.bytes = size;
            Iv iv = {};
            if (prot) iv = read_iv(src + s.src_offset, runs[k].iv_pos + (uint64_t)(row - runs[k].first_sample) * x->iv_size, x->iv_size);
            for (uint32_t j = 0; j < n; j++) crypt_lane(src + src_rows[row].src_offset, dst + at, size, j, prot ? w : nullptr, iv, te0);
            at += size; blocks += n;
        }
        rows[row] = out;
    }
    x->blocks = prot ? blocks : 0u;
}

}  // namespace cenc
