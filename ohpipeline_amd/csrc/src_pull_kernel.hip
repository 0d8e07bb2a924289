// src_pull_kernel.hip -- the pulled resampler: every message carries its own position and step, so a stream's ratio
// follows its clock controller message by message.  One persistent grid: each workgroup stages the filter's (P + 1) x T Q28 table in
// LDS once, then loops over the batch's tiles (up to 256 consecutive outputs of one message, cut on the host).  Per tile the input
// window is loaded coalesced and converted to the S24 domain once per subsample (kept as exact fp64 values); each lane owns one
// output frame, forms its T interpolated coefficients once and uses each for every channel.
#include <hip/hip_runtime.h>

#include "ohgpu_internal.h"
#include "pcm_device.h"

namespace ohgpu {

// LDS window of a tile, in subsamples (fp64): what keeps the T = 32 kernel at three workgroups a CU and the T = 64 one at two
// (table 257 x 33 x 4 = 33.9 KB + 16 KB; 257 x 65 x 4 = 66.8 KB + 12 KB; of 160 KiB)
uint32_t src_pull_window_cap(uint32_t T) { return T == 32 ? 2048u : 1536u; }

uint32_t src_pull_lds_bytes(uint32_t T, uint32_t phases_log2)
{
    return src_pull_window_cap(T) * 8u + ((1u << phases_log2) + 1u) * (T + 1u) * 4u;
}

constexpr uint32_t kStage = 8;                 // subsamples of a tile's window a lane loads: win_cap <= kStage * kPullTile

// A lane's share of a tile's window in the S24 domain, the depth and byte order constants: every byte load is issued before the
// first is waited for.  Frames before the stream start, and slots beyond the window, read the buffer's first frame (always there:
// a message's window lies inside its buffer) and are replaced by zeros.
template <uint32_t SB, bool LE, uint32_t CH>
__device__ __forceinline__ void load_window(int32_t (&x)[kStage], const uint8_t* __restrict__ s0, int64_t rel0, int64_t win_first,
                                            uint32_t nsub, uint32_t ch)
{
#pragma unroll
    for (uint32_t i = 0; i < kStage; i++) {
        const uint32_t q = threadIdx.x + i * kPullTile;
        const uint32_t f = CH ? q / CH : q / ch, c = q - f * ch;
        const bool real = q < nsub && win_first + (int64_t)f >= 0;
        const uint8_t* const p = real ? s0 + ((uint64_t)(rel0 + (int64_t)f) * ch + c) * SB : s0;
        const int32_t v = ((int32_t)load_be_word(p, SB, LE)) >> 8;
        x[i] = real ? v : 0;
    }
}

// CH = 0: any channel count 1..8 (read from the descriptor); CH = 2: stereo, the channel loop fixed at compile time.
template <uint32_t CH>
__global__ __launch_bounds__(kPullTile) void src_pull_kernel(const ohgpu_src_pull_msg_desc* __restrict__ descs,
                                                             const PullTile* __restrict__ tiles, uint32_t n_tiles,
                                                             const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                             const uint16_t* __restrict__ ramp_table,
                                                             const int32_t* __restrict__ table, uint32_t T, uint32_t s,
                                                             uint32_t win_cap)
{
    extern __shared__ double lds[];
    double* const win = lds;                                           // [frame][channel], S24 values as doubles
    int32_t* const tab = (int32_t*)(lds + win_cap);                    // row r at tab + r * (T + 1): the odd stride spreads the rows' banks
    const uint32_t P = 1u << s, stride = T + 1;
    const uint32_t tshift = T == 32 ? 5u : 6u;
    for (uint32_t i = threadIdx.x; i < (P + 1) * T; i += blockDim.x)
        tab[(i >> tshift) * stride + (i & (T - 1))] = table[i];
    constexpr uint32_t kAcc = CH ? CH : OHGPU_MAX_CHANNELS;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const PullTile tl = tiles[t];
        const ohgpu_src_pull_msg_desc& d = descs[tl.msg];
        const uint32_t ch = CH ? CH : d.channels, sb = d.src_bits >> 3, db = d.dst_bits >> 3;
        const bool src_le = d.src_endian == OHGPU_ENDIAN_LITTLE && sb > 1;
        __syncthreads();                                               // the table is in; the last tile's readers are done
        const uint8_t* const s0 = src + d.src_offset;
        const uint32_t nsub = tl.win_frames * ch;
        int32_t x[kStage];
        const int64_t rel0 = tl.win_first - (int64_t)d.src_frame0;
        switch (sb * 2 + (src_le ? 1 : 0)) {                           // (uniform: one branch a tile)
        case 2: case 3: load_window<1, false, CH>(x, s0, rel0, tl.win_first, nsub, ch); break;
        case 4: load_window<2, false, CH>(x, s0, rel0, tl.win_first, nsub, ch); break;
        case 5: load_window<2, true, CH>(x, s0, rel0, tl.win_first, nsub, ch); break;
        case 6: load_window<3, false, CH>(x, s0, rel0, tl.win_first, nsub, ch); break;
        case 7: load_window<3, true, CH>(x, s0, rel0, tl.win_first, nsub, ch); break;
        case 8: load_window<4, false, CH>(x, s0, rel0, tl.win_first, nsub, ch); break;
        default: load_window<4, true, CH>(x, s0, rel0, tl.win_first, nsub, ch); break;
        }
#pragma unroll
        for (uint32_t i = 0; i < kStage; i++) {
            const uint32_t q = threadIdx.x + i * kPullTile;
            if (q < nsub) win[q] = (double)x[i];                       // S24 values, exact as doubles
        }
        __syncthreads();
        if (threadIdx.x >= tl.count) continue;
        const uint32_t j = tl.j0 + threadIdx.x;
        const uint64_t u = (uint64_t)d.pos_frac + (uint64_t)j * d.step;
        const int64_t n = (int64_t)(d.pos_frame + (u >> 32));
        const uint32_t f = (uint32_t)u;
        const uint32_t p = (uint32_t)((uint64_t)f >> (32 - s));
        const int32_t wq = (int32_t)(((f >> (16 - s)) & 0xffffu) << 15);
        const int32_t* const r0 = tab + p * stride;
        const double* const xn = win + (uint32_t)(n - tl.win_first) * ch;
        double acc[kAcc];
#pragma unroll
        for (uint32_t c = 0; c < kAcc; c++) acc[c] = 0.0;
#pragma unroll 8
        for (uint32_t k = 0; k < T; k++) {
            const int32_t c0 = r0[k], c1 = r0[stride + k];
            // (C1 - C0) * w >> 16, arithmetic: the high word of (2 (C1 - C0)) * (w << 15); |C1 - C0| < 2^30 (check_src_pull_table)
            const double ck = (double)(c0 + __mulhi((c1 - c0) * 2, wq));
            const double* const xk = xn - k * ch;
#pragma unroll
            for (uint32_t c = 0; c < kAcc; c++)
                if (CH || c < ch) acc[c] = fma(ck, xk[c], acc[c]);
        }
        const bool ramp = (d.flags & OHGPU_FLAG_RAMP) != 0;
        uint32_t mult = 0;
        if (ramp) {
            const int32_t total = (int32_t)((uint32_t)d.ramp_start - (uint32_t)d.ramp_end);
            mult = ramp_table[ramp_index(d.ramp_start, total, (int32_t)j, (int32_t)d.n_frames)];
        }
        const bool dst_le = d.dst_endian == OHGPU_ENDIAN_LITTLE, zero_lsb = (d.flags & OHGPU_FLAG_ZERO_LSB32) != 0;
        uint8_t* const o = dst + d.dst_offset + (uint64_t)j * ch * db;
#pragma unroll
        for (uint32_t c = 0; c < kAcc; c++) {
            if (!CH && c >= ch) break;
            uint32_t w = ((uint32_t)src_round_s24(acc[c])) << 8;
            if (ramp) w = ramp_word(w, mult, 3, ch, c);
            store_word(o + c * db, w, db, dst_le, zero_lsb);
        }
    }
}

template <uint32_t CH>
static hipError_t launch_one(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    const ohgpu_src* f = b->src;
    const uint32_t lds = src_pull_lds_bytes(f->T, f->phases_log2);
    const void* kernel = (const void*)src_pull_kernel<CH>;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)kPullTile, (size_t)lds);
    if (e != hipSuccess) return e;
    const uint64_t want = (uint64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * (uint64_t)(per_cu > 0 ? per_cu : 1);
    const uint32_t grid = (uint32_t)(want < b->n_pull_tiles ? want : b->n_pull_tiles);
    hipLaunchKernelGGL(src_pull_kernel<CH>, dim3(grid), dim3(kPullTile), lds, s, (const ohgpu_src_pull_msg_desc*)b->d_descs,
                       (const PullTile*)b->d_pull_tiles, b->n_pull_tiles, src, dst, ctx->d_ramp_table, f->d_pull_table, f->T,
                       f->phases_log2, src_pull_window_cap(f->T));
    return hipGetLastError();
}

hipError_t launch_src_pull(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    if (b->n_pull_tiles == 0) return hipSuccess;
    return b->uniform && b->channels == 2 ? launch_one<2>(ctx, b, src, dst, s) : launch_one<0>(ctx, b, src, dst, s);
}

}  // namespace ohgpu
