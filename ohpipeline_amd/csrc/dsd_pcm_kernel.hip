// dsd_pcm_kernel.hip -- DSD -> PCM on the device (include/ohgpu.h).
//
// dsd_pcm_table_kernel, the fast route.  D is a multiple of 8, so an output's window of N bits is N / 8 whole BYTES of its channel's
// stream, and the sum over a byte's eight taps is one of 256 values: the filter becomes N / 8 tables of 256 int32 (built on the host
// when the filter is created, N / 8 KiB), an output N / 8 look-ups and adds -- no multiply, no bit is ever unpacked.  A workgroup
// brings the tables into LDS once and then loops over tiles of up to kDsdPcmTile frames of one message: the tile's bytes of both
// channels are staged into LDS byte by byte (pad bytes dropped, bytes before the stream start = 0x69), then one thread per output
// value walks its window.  Every source byte it loads lies in a chunk that ohgpu_dsd_pcm_window names for the message, which the
// creation held to the window and the arena: nothing is loaded wider than a byte, so nothing outside them is touched.
//
// dsd_pcm_kernel_v1, the plain route: dsd_pcm_core.h's convert_value, one thread per output value over the same tiles.
#include <hip/hip_runtime.h>

#include <vector>

#include "dsd_pcm_core.h"
#include "ohgpu_internal.h"
#include "pcm_device.h"

namespace ohgpu {

constexpr uint32_t kDsdPcmThreads = 2 * kDsdPcmTile;                         // one per output value of a tile
// a tile's bytes per channel: (frames - 1) * D / 8 + N / 8 <= 511 * 8 + 128
constexpr uint32_t kDsdPcmStageStride = (kDsdPcmTile - 1) * 8 + kDsdPcmTableTaps / 8 + 8;
static_assert(kDsdPcmStageStride % 4 == 0, "the second channel's stage starts on a dword");

static uint32_t dsd_pcm_lds_bytes(uint32_t N) { return N / 8 * 1024 + 2 * kDsdPcmStageStride; }

void build_dsd_pcm_tables(const int32_t* coef, uint32_t N, std::vector<int32_t>* tables)
{
    // byte b of a window holds, most significant bit first, the samples that meet coef[N - 1 - 8b - i], i = 0 .. 7
    tables->assign((size_t)N / 8 * 256, 0);
    for (uint32_t b = 0; b < N / 8; b++)
        for (uint32_t v = 0; v < 256; v++) {
            int32_t sum = 0;
            for (uint32_t i = 0; i < 8; i++) { const int32_t c = coef[N - 1 - 8 * b - i]; sum += ((v >> (7 - i)) & 1) ? c : -c; }
            (*tables)[(size_t)b * 256 + v] = sum;
        }
}

__global__ __launch_bounds__(kDsdPcmThreads) void dsd_pcm_table_kernel(const ohgpu_dsd_pcm_msg_desc* __restrict__ descs,
                                                                       const DsdPcmTile* __restrict__ tiles, uint32_t n_tiles,
                                                                       const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                       const uint16_t* __restrict__ ramp_table,
                                                                       const int32_t* __restrict__ tables, uint32_t NB, uint32_t DB)
{
    extern __shared__ int32_t lds[];
    int32_t* const tab = lds;                                              // [NB][256]
    uint8_t* const stage = (uint8_t*)(lds + NB * 256);                     // [2][kDsdPcmStageStride]
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < NB * 64; i += kDsdPcmThreads) ((int4*)tab)[i] = ((const int4*)tables)[i];
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        __syncthreads();                                                   // the tables are in; the last tile's stage has been read
        const DsdPcmTile t = tiles[tile];
        const ohgpu_dsd_pcm_msg_desc& d = descs[t.msg];
        const uint32_t P = d.pad_bytes_per_chunk, cs = 4u + P;
        const uint32_t nbytes = (t.count - 1u) * DB + NB;                  // per channel
        const int64_t byte0 = (int64_t)((d.out_frame0 + t.f0 + 1u) * DB) - (int64_t)NB;   // the tile's oldest byte of a channel's stream
        const uint8_t* const win = src + d.src_offset;
        for (uint32_t i = tid; i < 2u * nbytes; i += kDsdPcmThreads) {
            const uint32_t c = i >= nbytes, k = i - c * nbytes;
            const int64_t B = byte0 + (int64_t)k;
            uint8_t v = OHGPU_DSD_SILENCE_BYTE;
            if (B >= 0) v = win[(((uint64_t)B >> 1) - d.src_chunk0) * cs + (c ? P + 2u : P / 2u) + ((uint32_t)B & 1u)];
            stage[c * kDsdPcmStageStride + k] = v;
        }
        __syncthreads();
        const uint32_t f = tid >> 1, c = tid & 1u;
        if (f >= t.count) continue;
        const uint8_t* const w = stage + c * kDsdPcmStageStride + f * DB;
        int32_t acc = 16;
#pragma unroll 8
        for (uint32_t b = 0; b < NB; b++) acc += tab[b * 256u + w[b]];
        int32_t y = acc >> 5;
        y = y > 8388607 ? 8388607 : (y < -8388608 ? -8388608 : y);
        uint32_t word = (uint32_t)y << 8;                                  // the left-justified BE word of pcm_device.h
        if (d.flags & OHGPU_FLAG_RAMP) {
            const int32_t total = (int32_t)d.ramp_start - (int32_t)d.ramp_end;
            word = ramp_word(word, ramp_table[ramp_index(d.ramp_start, total, (int32_t)(t.f0 + f), (int32_t)d.n_frames)], 3, 2, c);
        }
        store_word(dst + d.dst_offset + ((uint64_t)(t.f0 + f) * 2u + c) * 3u, word, 3, d.dst_endian == OHGPU_ENDIAN_LITTLE, false);
    }
}

__global__ __launch_bounds__(kDsdPcmThreads) void dsd_pcm_kernel_v1(const ohgpu_dsd_pcm_msg_desc* __restrict__ descs,
                                                                    const DsdPcmTile* __restrict__ tiles, uint32_t n_tiles,
                                                                    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                    const uint16_t* __restrict__ ramp_table,
                                                                    const int32_t* __restrict__ coef, uint32_t N, uint32_t D)
{
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const DsdPcmTile t = tiles[tile];
        if ((threadIdx.x >> 1) < t.count)
            dsdpcm::convert_value(descs[t.msg], coef, N, D, src, dst, ramp_table, (uint64_t)t.f0 * 2u + threadIdx.x);
    }
}

void free_dsd_pcm(ohgpu_ctx* ctx, ohgpu_batch* b)
{
    if (b->dsdpcm.d_tiles) ctx_dev_free(ctx, b->dsdpcm.d_tiles);
    b->dsdpcm = DsdPcmPlan();
}

int plan_dsd_pcm(ohgpu_ctx* ctx, ohgpu_batch* b, const ohgpu_dsd_pcm_msg_desc* descs, size_t n)
{
    b->dsdpcm = DsdPcmPlan();
    std::vector<DsdPcmTile> tiles;
    uint32_t with_frames = 0;
    for (size_t i = 0; i < n; i++) {
        with_frames += descs[i].n_frames != 0;
        for (uint32_t f0 = 0; f0 < descs[i].n_frames; f0 += kDsdPcmTile) {
            const uint32_t left = descs[i].n_frames - f0;
            tiles.push_back(DsdPcmTile{(uint32_t)i, f0, left < kDsdPcmTile ? left : kDsdPcmTile, 0});
        }
    }
    if (tiles.size() > 0xffffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_pcm_batch_create: too many tiles");
    b->dsdpcm.fast = b->dsdpcm_filter->d_tables != nullptr && ctx->variant != 1;
    (b->dsdpcm.fast ? b->dsdpcm.n_fast : b->dsdpcm.n_plain) = with_frames;
    if (tiles.empty()) return OHGPU_OK;
    hipError_t e = ctx_dev_alloc(ctx, &b->dsdpcm.d_tiles, tiles.size() * sizeof(DsdPcmTile));
    if (e == hipSuccess) e = hipMemcpy(b->dsdpcm.d_tiles, tiles.data(), tiles.size() * sizeof(DsdPcmTile), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        free_dsd_pcm(ctx, b);
        return set_error(hip_code(e), "tile plan upload: %s", hipGetErrorString(e));
    }
    b->dsdpcm.n_tiles = (uint32_t)tiles.size();
    return OHGPU_OK;
}

hipError_t launch_dsd_pcm_table(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    const ohgpu_dsd_pcm* f = b->dsdpcm_filter;
    const uint32_t lds = dsd_pcm_lds_bytes(f->N);
    const void* kernel = (const void*)dsd_pcm_table_kernel;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)kDsdPcmThreads, (size_t)lds);
    if (e != hipSuccess) return e;
    // (a workgroup pays for its tables once: no more workgroups than the device holds at a time)
    const uint64_t want = (uint64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * (uint64_t)(per_cu > 0 ? per_cu : 1);
    const uint32_t grid = (uint32_t)(want < b->dsdpcm.n_tiles ? want : b->dsdpcm.n_tiles);
    hipLaunchKernelGGL(dsd_pcm_table_kernel, dim3(grid), dim3(kDsdPcmThreads), lds, s, (const ohgpu_dsd_pcm_msg_desc*)b->d_descs,
                       (const DsdPcmTile*)b->dsdpcm.d_tiles, b->dsdpcm.n_tiles, src, dst, ctx->d_ramp_table, f->d_tables, f->N / 8, f->D / 8);
    return hipGetLastError();
}

hipError_t launch_dsd_pcm_v1(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    const ohgpu_dsd_pcm* f = b->dsdpcm_filter;
    const uint32_t cus = ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256u;
    const uint32_t grid = b->dsdpcm.n_tiles < cus * 8u ? b->dsdpcm.n_tiles : cus * 8u;
    hipLaunchKernelGGL(dsd_pcm_kernel_v1, dim3(grid), dim3(kDsdPcmThreads), 0, s, (const ohgpu_dsd_pcm_msg_desc*)b->d_descs,
                       (const DsdPcmTile*)b->dsdpcm.d_tiles, b->dsdpcm.n_tiles, src, dst, ctx->d_ramp_table, f->d_coef, f->N, f->D);
    return hipGetLastError();
}

}  // namespace ohgpu
