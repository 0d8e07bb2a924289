// dsd_line_kernel.hip -- DSD on the device: the three codec-side packers, the playable pass-through and DSD silence.
//   DSF  CodecDsdDsf::Process      (Codec/DsdDsf.cpp:169-247): pairs of 4096-byte planes, left then right, bits LSB first
//   DFF  CodecDsdDff::TransferToOutputBuffer (Codec/DsdDff.cpp:305-327): bytes L R L R, MSB first
//   Raw  CodecDsdRaw / DsdFiller   (Codec/DsdRaw.cpp:119-134, DsdFiller.cpp:73-99): bytes L L R R, padding only
//   MsgPlayableDsd::ReadBlock (Pipeline/Msg.cpp:2834-2839) and MsgPlayableSilenceDsd::ReadBlock (:2916-2932)
// The pipeline format is a run of chunks of 4 + P bytes, [P/2 x 00] L L [P/2 x 00] R R; W * 4 bytes make a sample block, and what
// lies between a descriptor's last chunk and the end of its last block is 0x69.
//
// A descriptor is cut on the host into PIECES of up to 2048 chunks, one 32-byte record each, and a wave takes a piece.  On the wide
// path a lane takes eight chunks: sixteen source bytes per channel (one 16-byte load of each DSF plane, or two consecutive ones of
// a DFF / Raw stream), v_bfrev_b32 on each dword for DSF, then ONE v_perm_b32 per output dword -- its selector, a compile-time
// constant, interleaves the channels, inserts the padding and undoes the byte order the bit reversal turned round -- and two, three
// or four 16-byte stores (P = 0, 2, 4).  Nothing goes through LDS.  What is not a whole lane (the last 1..7 chunks of a descriptor),
// every piece of a descriptor whose offsets are not 16-byte aligned or whose padding is wider than 4, and the edges of the 0x69
// fill are written byte by byte by the same wave.
#include <hip/hip_runtime.h>

#include <vector>

#include "dsd_perm.h"
#include "ohgpu_internal.h"

namespace ohgpu {

constexpr uint32_t kDsdWaves = 4;
constexpr uint32_t kDsdPieceChunks = 2048;                             // chunks per piece: four passes of a wave's 64 lanes x 8 chunks
constexpr uint32_t kDsdLaneChunks = 8;
constexpr uint32_t kDsdSilenceWord = 0x01010101u * OHGPU_DSD_SILENCE_BYTE;
enum { kPieceWide = 1, kPieceSilence = 2 };

// (where byte t of a lane's output comes from, and the one v_perm_b32 per output dword -- dsd_src_of, dsd_perm, dsd_out_dword,
// dsd_store_vec: csrc/dsd_perm.h, shared with csrc/dsd_file_kernel.hip)

// The whole lanes of a piece: lane unit g = chunks [j0 + 8 g, + 8) of the descriptor.
template <int KIND, int P>
__device__ __forceinline__ void dsd_wide_body(const uint8_t* __restrict__ sp, uint8_t* __restrict__ dp, const uint32_t j0,
                                              const uint32_t units, const uint32_t lane)
{
    for (uint32_t g = lane; g < units; g += 64) {
        const uint64_t j = (uint64_t)j0 + (uint64_t)g * kDsdLaneChunks;
        const uint8_t *a, *b;
        if constexpr (KIND == OHGPU_DSD_DSF) {
            a = sp + (j >> 11) * 8192 + (j & 2047) * 2;                 // 8 | 2048: a lane never straddles a plane
            b = a + 4096;
        } else {
            a = sp + j * 4;
            b = a + 16;
        }
        const dv4 x = __builtin_nontemporal_load((const dv4*)a), y = __builtin_nontemporal_load((const dv4*)b);
        uint32_t in[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        if constexpr (KIND == OHGPU_DSD_DSF) {
#pragma unroll
            for (int k = 0; k < 8; k++) in[k] = __builtin_bitreverse32(in[k]);
        }
        uint8_t* out = dp + j * (4 + P);
        dsd_store_vec<KIND, P, 0>(in, out);
        dsd_store_vec<KIND, P, 1>(in, out);
        if constexpr (P >= 2) dsd_store_vec<KIND, P, 2>(in, out);
        if constexpr (P >= 4) dsd_store_vec<KIND, P, 3>(in, out);
    }
}

// `len` bytes of 0x69 at p: 16-byte stores between the first and the last 16-byte boundary inside it, bytes at its edges.
__device__ __forceinline__ void dsd_fill(uint8_t* p, const uint32_t len, const uint32_t lane)
{
    uint32_t head = (uint32_t)(-(intptr_t)p) & 15u;
    if (head > len) head = len;
    const uint32_t vecs = (len - head) >> 4, tail0 = head + (vecs << 4);
    const dv4 v = {kDsdSilenceWord, kDsdSilenceWord, kDsdSilenceWord, kDsdSilenceWord};
    for (uint32_t k = lane; k < vecs; k += 64) __builtin_nontemporal_store(v, (dv4*)(p + head + (size_t)k * 16));
    if (lane < head) p[lane] = (uint8_t)OHGPU_DSD_SILENCE_BYTE;
    if (lane < len - tail0) p[tail0 + lane] = (uint8_t)OHGPU_DSD_SILENCE_BYTE;
}

__global__ __launch_bounds__(kDsdWaves * 64) void dsd_line_kernel(const DsdPiece* __restrict__ pieces, const uint32_t n_pieces,
                                                                 const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                 const uint32_t arenas_aligned)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t piece = blockIdx.x * kDsdWaves + wave; piece < n_pieces; piece += gridDim.x * kDsdWaves) {
        const DsdPiece pc = pieces[piece];
        const uint32_t P = pc.pad, cs = 4u + P, kind = pc.kind, j0 = pc.j0, n = pc.n;
        const uint8_t* sp = src + pc.src_off;
        uint8_t* dp = dst + pc.dst_off;
        uint32_t done = 0;                                              // chunks of the piece the wide path has written
        if ((pc.flags & kPieceWide) && arenas_aligned) {
            if (kind == OHGPU_DSD_PASS) {                               // the piece's bytes as they are, sixteen to a lane
                const uint64_t first = (uint64_t)j0 * cs;               // (a multiple of 16: j0 is one of 2048, cs is even)
                const uint32_t vecs = (n * cs) >> 4;
                for (uint32_t k = lane; k < vecs; k += 64)
                    __builtin_nontemporal_store(__builtin_nontemporal_load((const dv4*)(sp + first + (size_t)k * 16)), (dv4*)(dp + first + (size_t)k * 16));
                const uint32_t rest = n * cs - (vecs << 4);
                if (lane < rest) dp[first + (vecs << 4) + lane] = sp[first + (vecs << 4) + lane];
                done = n;
            } else {
                const uint32_t units = n / kDsdLaneChunks;
                done = units * kDsdLaneChunks;
                switch (kind * 8 + P) {                                 // (the planner marks a packer's piece wide only for P = 0, 2, 4)
                case OHGPU_DSD_DSF * 8 + 0: dsd_wide_body<OHGPU_DSD_DSF, 0>(sp, dp, j0, units, lane); break;
                case OHGPU_DSD_DSF * 8 + 2: dsd_wide_body<OHGPU_DSD_DSF, 2>(sp, dp, j0, units, lane); break;
                case OHGPU_DSD_DSF * 8 + 4: dsd_wide_body<OHGPU_DSD_DSF, 4>(sp, dp, j0, units, lane); break;
                case OHGPU_DSD_DFF * 8 + 0: dsd_wide_body<OHGPU_DSD_DFF, 0>(sp, dp, j0, units, lane); break;
                case OHGPU_DSD_DFF * 8 + 2: dsd_wide_body<OHGPU_DSD_DFF, 2>(sp, dp, j0, units, lane); break;
                case OHGPU_DSD_DFF * 8 + 4: dsd_wide_body<OHGPU_DSD_DFF, 4>(sp, dp, j0, units, lane); break;
                case OHGPU_DSD_RAW * 8 + 0: dsd_wide_body<OHGPU_DSD_RAW, 0>(sp, dp, j0, units, lane); break;
                case OHGPU_DSD_RAW * 8 + 2: dsd_wide_body<OHGPU_DSD_RAW, 2>(sp, dp, j0, units, lane); break;
                case OHGPU_DSD_RAW * 8 + 4: dsd_wide_body<OHGPU_DSD_RAW, 4>(sp, dp, j0, units, lane); break;
                default: done = 0; break;
                }
            }
        }
        // ---- byte by byte: output bytes [done * cs, n * cs) of the piece ----
        const uint32_t b1 = n * cs;
        for (uint32_t t = done * cs + lane; t < b1; t += 64) {
            const uint32_t c = t / cs, o = t - c * cs, h = P >> 1;
            const uint64_t j = (uint64_t)j0 + c;
            uint32_t v = 0;
            if (kind == OHGPU_DSD_PASS) {
                v = sp[j * cs + o];
            } else if (o >= h && (o < h + 2 || o >= 2 * h + 2)) {
                const uint32_t ch = o < h + 2 ? 0u : 1u, i = ch ? o - 2 * h - 2 : o - h;
                if (kind == OHGPU_DSD_DSF) v = __builtin_bitreverse32(sp[(j >> 11) * 8192 + ch * 4096 + (j & 2047) * 2 + i]) >> 24;
                else if (kind == OHGPU_DSD_DFF) v = sp[j * 4 + ch + 2 * i];
                else v = sp[j * 4 + ch * 2 + i];
            }
            dp[(uint64_t)j0 * cs + t] = (uint8_t)v;
        }
        if (pc.fill) dsd_fill(dp + ((uint64_t)j0 + n) * cs, pc.fill, lane);
    }
}

// ---- the plain kernel (ohgpu_set_kernel_variant(1)): a workgroup per descriptor, a thread per chunk, then per fill byte ----
__device__ __forceinline__ uint8_t dsd_reverse8(uint8_t x)
{
    uint8_t r = 0;
    for (int k = 0; k < 8; k++) r = (uint8_t)(r | (((x >> k) & 1) << (7 - k)));
    return r;
}

__global__ __launch_bounds__(256) void dsd_kernel_v1(const ohgpu_dsd_desc* __restrict__ descs, const uint32_t n_descs,
                                                     const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    for (uint32_t d = blockIdx.x; d < n_descs; d += gridDim.x) {
        const ohgpu_dsd_desc ds = descs[d];
        const uint32_t P = ds.pad_bytes_per_chunk, cs = 4u + P, per_block = ds.sample_block_words * 4u / cs;
        const uint64_t blocks = ((uint64_t)ds.n_chunks + per_block - 1) / per_block, total = blocks * ds.sample_block_words * 4u;
        const bool silent = (ds.flags & OHGPU_DSD_FLAG_SILENCE) != 0;
        const uint8_t* sp = src + ds.src_offset;
        uint8_t* dp = dst + ds.dst_offset;
        for (uint64_t j = threadIdx.x; j < ds.n_chunks && !silent; j += blockDim.x) {
            uint8_t* o = dp + j * cs;
            if (ds.kind == OHGPU_DSD_PASS) {
                for (uint32_t k = 0; k < cs; k++) o[k] = sp[j * cs + k];
                continue;
            }
            uint8_t l0, l1, r0, r1;
            if (ds.kind == OHGPU_DSD_DSF) {
                const uint8_t* pl = sp + (j / 2048) * 8192 + (j % 2048) * 2;
                l0 = dsd_reverse8(pl[0]); l1 = dsd_reverse8(pl[1]); r0 = dsd_reverse8(pl[4096]); r1 = dsd_reverse8(pl[4097]);
            } else if (ds.kind == OHGPU_DSD_DFF) {
                l0 = sp[4 * j]; r0 = sp[4 * j + 1]; l1 = sp[4 * j + 2]; r1 = sp[4 * j + 3];
            } else {
                l0 = sp[4 * j]; l1 = sp[4 * j + 1]; r0 = sp[4 * j + 2]; r1 = sp[4 * j + 3];
            }
            for (uint32_t k = 0; k < P / 2; k++) o[k] = 0;
            o += P / 2;
            o[0] = l0; o[1] = l1;
            o += 2;
            for (uint32_t k = 0; k < P / 2; k++) o[k] = 0;
            o += P / 2;
            o[0] = r0; o[1] = r1;
        }
        for (uint64_t t = (silent ? 0 : (uint64_t)ds.n_chunks * cs) + threadIdx.x; t < total; t += blockDim.x) dp[t] = (uint8_t)OHGPU_DSD_SILENCE_BYTE;
    }
}

// ---- host side ----
void free_dsd_line(ohgpu_ctx* ctx, ohgpu_batch* b)
{
    if (b->dsd.d_pieces) ctx_dev_free(ctx, b->dsd.d_pieces);
    b->dsd = DsdPlan();
}

int plan_dsd_line(ohgpu_ctx* ctx, ohgpu_batch* b, const ohgpu_dsd_desc* descs, size_t n)
{
    b->dsd = DsdPlan();
    std::vector<DsdPiece> pieces;
    for (size_t i = 0; i < n; i++) {
        const ohgpu_dsd_desc& d = descs[i];
        if (d.n_chunks == 0) continue;
        const uint32_t P = d.pad_bytes_per_chunk, cs = 4u + P, per_block = d.sample_block_words * 4u / cs;
        const uint64_t blocks = ((uint64_t)d.n_chunks + per_block - 1) / per_block;
        const bool silent = (d.flags & OHGPU_DSD_FLAG_SILENCE) != 0;
        const bool aligned = d.dst_offset % 16 == 0 && (silent || d.src_offset % 16 == 0);
        DsdPiece pc;
        memset(&pc, 0, sizeof(pc));
        pc.src_off = silent ? 0 : d.src_offset; pc.dst_off = d.dst_offset;
        pc.kind = d.kind; pc.pad = (uint8_t)P;
        bool wide;                                                      // some of the descriptor goes out in 16-byte stores
        if (silent) {                                                   // all fill, cut where the audible pieces would be cut
            pc.flags = kPieceSilence;
            const uint64_t total = blocks * d.sample_block_words * 4u, step = (uint64_t)kDsdPieceChunks * cs;
            for (uint64_t at = 0; at < total; at += step) {
                pc.j0 = (uint32_t)(at / cs); pc.n = 0; pc.fill = (uint32_t)std::min<uint64_t>(step, total - at);
                pieces.push_back(pc);
            }
            wide = aligned && total >= 16;
        } else {
            const bool lanes = aligned && (d.kind == OHGPU_DSD_PASS || P <= 4);
            pc.flags = lanes ? kPieceWide : 0;
            for (uint64_t j0 = 0; j0 < d.n_chunks; j0 += kDsdPieceChunks) {
                pc.j0 = (uint32_t)j0; pc.n = (uint32_t)std::min<uint64_t>(kDsdPieceChunks, d.n_chunks - j0);
                pc.fill = j0 + pc.n == d.n_chunks ? (uint32_t)(blocks * d.sample_block_words * 4u - (uint64_t)d.n_chunks * cs) : 0u;
                pieces.push_back(pc);
            }
            wide = lanes && (d.kind == OHGPU_DSD_PASS ? (uint64_t)d.n_chunks * cs >= 16 : d.n_chunks >= kDsdLaneChunks);
        }
        if (wide) b->dsd.n_wide++; else b->dsd.n_generic++;
    }
    if (pieces.empty()) return OHGPU_OK;
    if (pieces.size() > 0xffffffffull) { b->dsd = DsdPlan(); return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_batch_create: too many pieces"); }
    hipError_t e = ctx_dev_alloc(ctx, &b->dsd.d_pieces, pieces.size() * sizeof(DsdPiece));
    if (e == hipSuccess) e = hipMemcpy(b->dsd.d_pieces, pieces.data(), pieces.size() * sizeof(DsdPiece), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        free_dsd_line(ctx, b);
        return set_error(hip_code(e), "piece plan upload: %s", hipGetErrorString(e));
    }
    b->dsd.n_pieces = (uint32_t)pieces.size();
    return OHGPU_OK;
}

hipError_t launch_dsd_line(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    if (b->dsd.n_pieces == 0) return hipSuccess;
    const uint32_t cus = ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256u;
    uint32_t grid = (b->dsd.n_pieces + kDsdWaves - 1) / kDsdWaves;
    if (grid > cus * 8u) grid = cus * 8u;
    const uint32_t arenas_aligned = (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0;
    hipLaunchKernelGGL(dsd_line_kernel, dim3(grid), dim3(kDsdWaves * 64), 0, s, (const DsdPiece*)b->dsd.d_pieces, b->dsd.n_pieces, src, dst, arenas_aligned);
    return hipGetLastError();
}

hipError_t launch_dsd_v1(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    const uint32_t cus = ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256u;
    const uint32_t grid = (uint32_t)std::min<size_t>(b->n, (size_t)cus * 8u);
    hipLaunchKernelGGL(dsd_kernel_v1, dim3(grid), dim3(256), 0, s, (const ohgpu_dsd_desc*)b->d_descs, (uint32_t)b->n, src, dst);
    return hipGetLastError();
}

}  // namespace ohgpu
