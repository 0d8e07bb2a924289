// raop_aes_core.h -- what stands between a RAOP (AirPlay) datagram and the Apple Lossless decoder: AES-128 in CBC mode, decryption
// only, under RAOP's packet rule.  Written from FIPS-197; the tables are computed here, at compile time, from the
// field's arithmetic.  Everything is __host__ __device__: csrc/raop_decrypt_kernel.hip runs this text on the device,
// tests/cpp/raop_core_driver.cpp runs the same text on the CPU under the sanitizers.
// (csrc/cenc_core.h builds its forward table from this file's S-box and field arithmetic and takes expand_encrypt_key as it is.)
//
// Reading of the standard:
//   field      GF(2^8) modulo x^8 + x^4 + x^3 + x + 1; the S-box is the field inverse (0 -> 0) through the affine map
//              b ^ rotl(b,1) ^ rotl(b,2) ^ rotl(b,3) ^ rotl(b,4) ^ 0x63, the inverse S-box its inverse.
//   state      four columns; a column is one 32-bit word read LITTLE-endian from the block, so that row r of the column is byte r of
//              the word and a block is four dword loads with no byte swap.
//   cipher     the equivalent inverse cipher (FIPS-197 5.3.5): AddRoundKey(dk[0]); nine rounds of InvSubBytes, InvShiftRows,
//              InvMixColumns, AddRoundKey(dk[r]); then InvSubBytes, InvShiftRows, AddRoundKey(dk[10]).  dk[r] is the encryption
//              schedule's key 10 - r, with InvMixColumns applied to dk[1..9].  A round's first three steps are four table reads a
//              column: Td0[x] = InvMixColumns of the column (InvSbox[x], 0, 0, 0); the tables of rows 1..3 are Td0 rotated left
//              by 8, 16 and 24 bits, so only Td0 is kept.
//   RAOP       (RaopAudioDecryptor::Decrypt, OpenHome/Av/Raop/ProtocolRaop.cpp:1477-1502) every packet starts again from the
//              session's IV: plaintext block j = D(C_j) ^ (j == 0 ? IV : C_{j-1}); the bytes % 16 tail is copied as sent; a packet
//              shorter than 16 bytes is all tail; a packet of 0 bytes writes nothing.
//
// Work is cut into pieces: up to 64 consecutive blocks of one packet, a lane per block; the piece that holds a packet's last block
// (or, for a packet with no whole block, its only piece) also copies the tail, a byte per lane.  Every load and store of a piece
// lies inside [src_offset, src_offset + bytes) and [dst_offset, dst_offset + bytes) of its packet.
#pragma once

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define RAOP_HD __host__ __device__ inline
#else
#define RAOP_HD inline
#endif

namespace raopcore {

enum { kBlock = 16, kPieceBlocks = 64, kRoundKeyWords = 44, kKeyWords = 48 };   // a stream's record: 44 words of schedule, 4 of IV

struct Tables {
    uint32_t td0[256];
    uint8_t  isbox[256];
    uint8_t  sbox[256];
};

constexpr uint8_t gf_mul(uint8_t a, uint8_t b)
{
    uint8_t p = 0;
    for (int k = 0; k < 8; k++) {
        if (b & 1) p = (uint8_t)(p ^ a);
        const bool high = (a & 0x80) != 0;
        a = (uint8_t)(a << 1);
        if (high) a = (uint8_t)(a ^ 0x1b);
        b = (uint8_t)(b >> 1);
    }
    return p;
}

constexpr uint8_t rotl8(uint8_t v, int n) { return (uint8_t)((v << n) | (v >> (8 - n))); }

constexpr Tables make_tables()
{
    Tables t = {};
    // the field's inverses through powers of the generator x + 1: 3^k for k = 0..254 visits every non-zero element, and the inverse of
    // 3^k is 3^(255 - k); 0 maps to 0
    uint8_t power[255] = {}, inverse[256] = {};
    int log[256] = {};
    uint8_t g = 1;
    for (int k = 0; k < 255; k++) { power[k] = g; log[g] = k; g = gf_mul(g, 3); }
    for (int x = 1; x < 256; x++) inverse[x] = power[(255 - log[x]) % 255];
    for (int x = 0; x < 256; x++) {
        const uint8_t b = inverse[x];
        const uint8_t s = (uint8_t)(b ^ rotl8(b, 1) ^ rotl8(b, 2) ^ rotl8(b, 3) ^ rotl8(b, 4) ^ 0x63);
        t.sbox[x] = s;
        t.isbox[s] = (uint8_t)x;
    }
    for (int x = 0; x < 256; x++) {
        const uint8_t s = t.isbox[x];
        t.td0[x] = (uint32_t)gf_mul(s, 0x0e) | ((uint32_t)gf_mul(s, 0x09) << 8) | ((uint32_t)gf_mul(s, 0x0d) << 16) | ((uint32_t)gf_mul(s, 0x0b) << 24);
    }
    return t;
}

RAOP_HD uint32_t rotl32(uint32_t v, uint32_t n) { return (v << n) | (v >> (32u - n)); }

// InvSubBytes + InvShiftRows + InvMixColumns of one output column: row r comes from column (c - r) mod 4, here a, b, c, d in that order
RAOP_HD uint32_t inv_round_column(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const uint32_t* td0)
{
    return td0[a & 0xffu] ^ rotl32(td0[(b >> 8) & 0xffu], 8) ^ rotl32(td0[(c >> 16) & 0xffu], 16) ^ rotl32(td0[d >> 24], 24);
}

RAOP_HD uint32_t inv_last_column(uint32_t a, uint32_t b, uint32_t c, uint32_t d, const uint8_t* isbox)
{
    return (uint32_t)isbox[a & 0xffu] | ((uint32_t)isbox[(b >> 8) & 0xffu] << 8) | ((uint32_t)isbox[(c >> 16) & 0xffu] << 16) | ((uint32_t)isbox[d >> 24] << 24);
}

// rk: the equivalent inverse cipher's schedule (expand_decrypt_key).  c and p may not overlap.
RAOP_HD void decrypt_block(const uint32_t rk[44], const uint32_t c[4], uint32_t p[4], const uint32_t* td0, const uint8_t* isbox)
{
    uint32_t s0 = c[0] ^ rk[0], s1 = c[1] ^ rk[1], s2 = c[2] ^ rk[2], s3 = c[3] ^ rk[3];
    for (int r = 1; r < 10; r++) {
        const uint32_t t0 = inv_round_column(s0, s3, s2, s1, td0) ^ rk[4 * r];
        const uint32_t t1 = inv_round_column(s1, s0, s3, s2, td0) ^ rk[4 * r + 1];
        const uint32_t t2 = inv_round_column(s2, s1, s0, s3, td0) ^ rk[4 * r + 2];
        const uint32_t t3 = inv_round_column(s3, s2, s1, s0, td0) ^ rk[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    p[0] = inv_last_column(s0, s3, s2, s1, isbox) ^ rk[40];
    p[1] = inv_last_column(s1, s0, s3, s2, isbox) ^ rk[41];
    p[2] = inv_last_column(s2, s1, s0, s3, isbox) ^ rk[42];
    p[3] = inv_last_column(s3, s2, s1, s0, isbox) ^ rk[43];
}

// FIPS-197 5.2's expansion of the 16 key bytes as sent: the 11 round keys of the cipher itself (words little-endian, so RotWord is a
// rotation right by 8 and Rcon lands in the low byte).  csrc/cenc_core.h's counter mode takes this schedule as it is.
inline void expand_encrypt_key(const uint8_t key[16], uint32_t w[44], const Tables& t)
{
    for (int i = 0; i < 4; i++) w[i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) | ((uint32_t)key[4 * i + 3] << 24);
    uint8_t rcon = 1;
    for (int i = 4; i < 44; i++) {
        uint32_t v = w[i - 1];
        if (i % 4 == 0) {
            v = (v >> 8) | (v << 24);
            v = (uint32_t)t.sbox[v & 0xffu] | ((uint32_t)t.sbox[(v >> 8) & 0xffu] << 8) | ((uint32_t)t.sbox[(v >> 16) & 0xffu] << 16) | ((uint32_t)t.sbox[v >> 24] << 24);
            v ^= rcon;
            rcon = gf_mul(rcon, 2);
        }
        w[i] = w[i - 4] ^ v;
    }
}

// The 11 round keys of the equivalent inverse cipher: the expansion above, the keys taken in reverse, InvMixColumns on keys 1..9.
inline void expand_decrypt_key(const uint8_t key[16], uint32_t rk[44], const Tables& t)
{
    uint32_t w[44];
    expand_encrypt_key(key, w, t);
    for (int r = 0; r <= 10; r++)
        for (int c = 0; c < 4; c++) {
            const uint32_t v = w[4 * (10 - r) + c];
            // InvMixColumns(v) by the round's own table: Td0[Sbox[b]] is InvMixColumns of (b, 0, 0, 0)
            rk[4 * r + c] = r == 0 || r == 10 ? v
                          : t.td0[t.sbox[v & 0xffu]] ^ rotl32(t.td0[t.sbox[(v >> 8) & 0xffu]], 8) ^ rotl32(t.td0[t.sbox[(v >> 16) & 0xffu]], 16) ^ rotl32(t.td0[t.sbox[v >> 24]], 24);
        }
    for (uint32_t& v : w) *(volatile uint32_t*)&v = 0;
}

inline void load_iv(const uint8_t iv[16], uint32_t out[4])
{
    for (int i = 0; i < 4; i++) out[i] = (uint32_t)iv[4 * i] | ((uint32_t)iv[4 * i + 1] << 8) | ((uint32_t)iv[4 * i + 2] << 16) | ((uint32_t)iv[4 * i + 3] << 24);
}

// ---- the work table ----
struct Job {                     // one packet: where its bytes lie and where its plaintext goes
    uint64_t src_offset;         // multiple of 4, in the source arena
    uint64_t dst_offset;         // multiple of 4, in the arena `to_arena` names
    uint32_t bytes, key;         // key: the stream's record, kKeyWords words each
    uint32_t to_arena;           // 0: the batch's plaintext scratch; 1: the caller's destination arena
    uint32_t reserved;
};

struct Piece {                   // up to kPieceBlocks consecutive blocks of one packet: 32 bytes
    uint64_t src_offset, dst_offset;     // the PACKET's
    uint32_t key;
    uint32_t first_block, n_blocks;      // blocks [first_block, first_block + n_blocks), n_blocks 0..64
    uint16_t tail;                       // bytes behind block first_block + n_blocks that are copied as sent (the packet's last piece only)
    uint16_t to_arena;
};

struct StreamIn {                // what the plan needs of a stream descriptor
    uint32_t first_packet, n_packets;
    uint64_t dst_offset;
    uint32_t plaintext;          // OHGPU_RAOP_OUT_PLAINTEXT: the source layout moved to dst_offset; else: the scratch, every packet at a 16-byte boundary
    uint32_t reserved;
};
struct PacketIn { uint64_t src_offset; uint32_t bytes, reserved; };      // ohgpu_alac_packet

// A job per packet of the table, in the table's order; returns the bytes of plaintext scratch the decoding streams take.
inline uint64_t plan_jobs(const StreamIn* streams, size_t n, const PacketIn* packets, std::vector<Job>* jobs)
{
    uint64_t scratch = 0;
    for (size_t i = 0; i < n; i++) {
        const StreamIn& s = streams[i];
        for (uint32_t k = 0; k < s.n_packets; k++) {
            const PacketIn& p = packets[s.first_packet + k];
            Job j;
            j.src_offset = p.src_offset; j.bytes = p.bytes; j.key = (uint32_t)i; j.reserved = 0;
            j.to_arena = s.plaintext ? 1u : 0u;
            if (s.plaintext) j.dst_offset = s.dst_offset + (p.src_offset - packets[s.first_packet].src_offset);
            else { j.dst_offset = scratch; scratch += ((uint64_t)p.bytes + kBlock - 1) / kBlock * kBlock; }
            jobs->push_back(j);
        }
    }
    return scratch;
}

inline void plan_pieces(const Job* jobs, size_t n, std::vector<Piece>* out)
{
    for (size_t i = 0; i < n; i++) {
        const Job& j = jobs[i];
        const uint32_t blocks = j.bytes / kBlock, tail = j.bytes % kBlock;
        if (j.bytes == 0) continue;
        for (uint32_t b = 0; b == 0 || b < blocks; b += kPieceBlocks) {
            Piece p;
            p.src_offset = j.src_offset; p.dst_offset = j.dst_offset; p.key = j.key;
            p.first_block = b;
            p.n_blocks = blocks - b < (uint32_t)kPieceBlocks ? blocks - b : (uint32_t)kPieceBlocks;
            p.tail = (uint16_t)(b + p.n_blocks == blocks ? tail : 0u);
            p.to_arena = (uint16_t)j.to_arena;
            out->push_back(p);
        }
    }
}

RAOP_HD uint32_t load32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
    return v;
}

RAOP_HD void store32(uint8_t* p, uint32_t v) { __builtin_memcpy(__builtin_assume_aligned(p, 4), &v, 4); }

// One lane of a piece.  keys: the stream's record (44 words of schedule, then the IV); src and dst are 4-byte aligned arena bases.
RAOP_HD void piece_lane(const Piece& pc, uint32_t lane, const uint32_t* keys, const uint8_t* src, uint8_t* dst, const uint32_t* td0, const uint8_t* isbox)
{
    const uint8_t* in = src + pc.src_offset;
    uint8_t* out = dst + pc.dst_offset;
    if (lane < pc.n_blocks) {
        const uint64_t at = (uint64_t)(pc.first_block + lane) * kBlock;
        uint32_t c[4], prev[4], p[4];
        for (int k = 0; k < 4; k++) {
            c[k] = load32(in + at + 4 * k);
            prev[k] = at ? load32(in + at - kBlock + 4 * k) : keys[kRoundKeyWords + k];
        }
        decrypt_block(keys, c, p, td0, isbox);
        for (int k = 0; k < 4; k++) store32(out + at + 4 * k, p[k] ^ prev[k]);
    }
    if (lane < pc.tail) {
        const uint64_t at = (uint64_t)(pc.first_block + pc.n_blocks) * kBlock + lane;
        out[at] = in[at];
    }
}

}  // namespace raopcore
