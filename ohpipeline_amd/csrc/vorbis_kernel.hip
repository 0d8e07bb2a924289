// vorbis_kernel.hip -- Vorbis I packets on the device (the format text is csrc/vorbis_core.h).
// One run is four phases, all queued on the stream:
//   head       the rows zeroed; a lane per packet reads type, mode and window flags; a lane per stream sums the blocks into positions
//   entropy    a lane per OK packet, bit-serial: the floors' values unwrapped, the residue's passes added into the packet's float32 rows
//              (plain adds in the specification's order), the coupling undone
//   synthesis  a workgroup per (packet, channel): lane 0 lists the curve's segments, a lane a segment draws it by the integer line rule
//              and multiplies the row by the dB table into the LDS (and back to the row, which ohgpu_vorbis_batch_spectrum reads); the
//              IMDCT of N = n / 2 coefficients is a DCT-IV through an N / 2-point complex FFT in the LDS -- t[m] = (X[2m] + i X[N-1-2m])
//              A[m], radix 2 in place from bit-reversed order, c[k] = T[k] B[k], u[2k] = Re c[k], u[N-1-2k] = -Im c[k] -- whose N values
//              unfold into the block's n, times the window, to the block scratch.  A, B, the FFT's twiddles and the window's slopes are
//              tables the host made in double.  The LDS holds 16 KiB of complex data and 16 KiB of spectrum at n = 8192.
//   store      a lane per output sample of a packet: the previous block's second half plus this block's first, rounded and clipped,
//              to the interleaved big-endian frames or the planes
// The plain route (a batch created under ohgpu_set_kernel_variant(1)) differs in the transform alone: the DCT-IV as the direct sum over a
// cosine table of 8N points, accumulated in double.
// Rows and blocks lie packet by packet (not transposed: a lane of the entropy phase owns whole rows).  Every load of packet bytes is
// bounded by the packet's bit count, every row and block index by the block size, every destination store by samples <= max_samples -
// position, which the batch check holds inside the arena.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "api_common.h"

namespace ohgpu {

using namespace vorbiscore;

constexpr uint32_t kVbLanes = 64, kVbThreads = 256, kVbMaxHalf = 4096;

struct VorbisTabs { VorbisTab t[14]; };

__global__ __launch_bounds__(kVbLanes) void vorbis_head_kernel(const Stream* __restrict__ streams, const Packet* __restrict__ packets, uint32_t n,
                                                               const uint32_t* __restrict__ images, const uint8_t* __restrict__ src, Rec* __restrict__ recs)
{
    const uint32_t i = blockIdx.x * kVbLanes + threadIdx.x;
    if (i >= n) return;
    const Packet pk = packets[i];
    head_packet(images + streams[pk.stream].image_word, src + pk.src_offset, pk.bytes, &recs[i]);
}

__global__ __launch_bounds__(kVbLanes) void vorbis_scan_kernel(const Stream* __restrict__ streams, uint32_t n, Rec* __restrict__ recs)
{
    const uint32_t i = blockIdx.x * kVbLanes + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    scan_stream(s, recs + s.first_packet);
}

__global__ __launch_bounds__(kVbLanes) void vorbis_entropy_kernel(const Stream* __restrict__ streams, const Packet* __restrict__ packets, uint32_t n,
                                                                  const uint32_t* __restrict__ images, const uint8_t* __restrict__ src, const Rec* __restrict__ recs,
                                                                  float* __restrict__ rows, FloorOut* __restrict__ floors, uint8_t* __restrict__ cls)
{
    const uint32_t i = blockIdx.x * kVbLanes + threadIdx.x;
    if (i >= n) return;
    const Rec rec = recs[i];
    if (rec.status != kOk) return;
    const Packet pk = packets[i];
    const Stream s = streams[pk.stream];
    const uint32_t stride = s.bs1 / 2u;
    const Rows r{rows + s.row_base + (uint64_t)pk.index * s.channels * stride, stride};
    decode_packet(images + s.image_word, src + pk.src_offset, pk.bytes, rec, r, floors + (uint64_t)i * kMaxChannels, cls + s.class_base + (uint64_t)pk.index * s.class_bytes);
}

// PLAIN: the direct-form DCT-IV in place of the FFT.
template <bool PLAIN>
__global__ __launch_bounds__(kVbThreads) void vorbis_synth_kernel(const Stream* __restrict__ streams, const Packet* __restrict__ packets, const uint32_t* __restrict__ images,
                                                                   const Rec* __restrict__ recs, const FloorOut* __restrict__ floors, float* __restrict__ rows,
                                                                   float* __restrict__ blocks, const float* __restrict__ tables, VorbisTabs tabs)
{
    __shared__ float spec[kVbMaxHalf];
    __shared__ float2 buf[kVbMaxHalf / 2];
    __shared__ Segment segs[64];
    __shared__ int32_t seg_info[3];
    const uint32_t p = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const Rec rec = recs[p];
    if (rec.status != kOk) return;
    const Packet pk = packets[p];
    const Stream s = streams[pk.stream];
    if (c >= s.channels) return;
    const uint32_t n = rec.blocksize, N = n / 2u, M = N / 2u;
    float* row = rows + s.row_base + ((uint64_t)pk.index * s.channels + c) * (s.bs1 / 2u);
    float* block = blocks + s.block_base + ((uint64_t)pk.index * s.channels + c) * s.bs1;
    const FloorOut& fo = floors[(uint64_t)p * kMaxChannels + c];
    if (!fo.used) {                                                     // (uniform over the workgroup)
        for (uint32_t i = tid; i < N; i += kVbThreads) row[i] = 0.0f;
        for (uint32_t i = tid; i < n; i += kVbThreads) block[i] = 0.0f;
        return;
    }
    const uint32_t* img = images + s.image_word;
    const Mode& mode = image_mode(img, rec.mode);
    const Mapping& map = image_mapping(img, mode.mapping);
    const Floor& fl = image_floor(img, map.sub_floor[map.mux[c]]);
    if (tid == 0) {
        int32_t tx, ty;
        seg_info[0] = (int32_t)floor_segments(fl, fo, segs, &tx, &ty);
        seg_info[1] = tx; seg_info[2] = ty;
    }
    __syncthreads();
    const float* db = tables;
    if (tid < (uint32_t)seg_info[0])
        draw_segment(segs[tid], (int32_t)N, [&](int32_t x, int32_t y) { spec[x] = row[x] * db[y]; });
    for (uint32_t x = (uint32_t)seg_info[1] + tid; x < N; x += kVbThreads) spec[x] = row[x] * db[seg_info[2]];
    __syncthreads();
    for (uint32_t i = tid; i < N; i += kVbThreads) row[i] = spec[i];
    const uint32_t lg = 31u - (uint32_t)__clz((int)n);
    const VorbisTab tab = tabs.t[lg];
    if (PLAIN) {
        const float* cos8 = tables + tab.cos8;
        float* u = (float*)buf;                                         // N floats: the 16 KiB of the complex buffer
        for (uint32_t i = tid; i < N; i += kVbThreads) u[i] = dct4_direct(spec, N, cos8, i);
        __syncthreads();
        for (uint32_t i = tid; i < N; i += kVbThreads) spec[i] = u[i];
    } else {
        const float2* A = (const float2*)(tables + tab.a);
        const float2* B = (const float2*)(tables + tab.b);
        const float2* W = (const float2*)(tables + tab.w);
        const uint32_t lgM = lg - 2u;
        for (uint32_t m = tid; m < M; m += kVbThreads) {
            const float re = spec[2u * m], im = spec[N - 1u - 2u * m];
            const float2 a = A[m];
            buf[__brev(m) >> (32u - lgM)] = make_float2(re * a.x - im * a.y, re * a.y + im * a.x);
        }
        for (uint32_t h = 1; h < M; h *= 2u) {
            __syncthreads();
            const uint32_t tw = M / (2u * h);
            for (uint32_t b = tid; b < M / 2u; b += kVbThreads) {
                const uint32_t j = b & (h - 1u), i = ((b - j) << 1) + j;
                const float2 w = W[j * tw], lo = buf[i], hi = buf[i + h];
                const float2 t = make_float2(hi.x * w.x - hi.y * w.y, hi.x * w.y + hi.y * w.x);
                buf[i] = make_float2(lo.x + t.x, lo.y + t.y);
                buf[i + h] = make_float2(lo.x - t.x, lo.y - t.y);
            }
        }
        __syncthreads();
        for (uint32_t k = tid; k < M; k += kVbThreads) {
            const float2 v = buf[k], bb = B[k];
            spec[2u * k] = v.x * bb.x - v.y * bb.y;
            spec[N - 1u - 2u * k] = -(v.x * bb.y + v.y * bb.x);
        }
    }
    __syncthreads();
    const float* slope_n = tables + tab.slope;
    const float* slope_0 = tables + tabs.t[31u - (uint32_t)__clz((int)s.bs0)].slope;
    const bool is_long = mode.blockflag != 0;
    for (uint32_t i = tid; i < n; i += kVbThreads) {
        block[i] = unfold_at(spec, N, i) * window_at(i, n, s.bs0, is_long, rec.prev_flag != 0, rec.next_flag != 0, slope_n, slope_0);
    }
}

__global__ __launch_bounds__(kVbThreads) void vorbis_store_kernel(const Stream* __restrict__ streams, const Packet* __restrict__ packets, const Rec* __restrict__ recs,
                                                                   const float* __restrict__ blocks, uint8_t* __restrict__ dst)
{
    const uint32_t p = blockIdx.x, j = blockIdx.y * kVbThreads + threadIdx.x;
    const Rec rec = recs[p];
    if (rec.status != kOk || j >= rec.samples) return;
    const Packet pk = packets[p];
    const Stream s = streams[pk.stream];
    const uint32_t n = rec.blocksize, pn = rec.prev_block, ch = s.channels;
    const float* cur = blocks + s.block_base + (uint64_t)pk.index * ch * s.bs1;
    const float* prev = blocks + s.block_base + (uint64_t)rec.prev_packet * ch * s.bs1;
    const uint64_t at = rec.position + j;
    for (uint32_t c = 0; c < ch; c++) {
        const int32_t v = to_pcm16(overlap_at(prev + (uint64_t)c * s.bs1, pn, cur + (uint64_t)c * s.bs1, n, j));
        if (s.flags & kOutPlanar32) *(int32_t*)(dst + s.dst_offset + c * s.dst_plane_stride + at * 4u) = v;
        else {
            uint8_t* q = dst + s.dst_offset + (at * ch + c) * 2u;
            *(uint16_t*)q = (uint16_t)((((uint32_t)v >> 8) & 0xffu) | (((uint32_t)v & 0xffu) << 8));
        }
    }
}

// The tables of one block size, appended to `t`: A[m] = exp(-i pi (4m + 1) / (4N)), B[k] = exp(-i pi k / N), W[j] = exp(-2 pi i j / M),
// the window's rising slope, and for the plain route cos(2 pi j / (8N)).
static VorbisTab make_tables(uint32_t n, bool plain, std::vector<float>* t)
{
    const double pi = 3.14159265358979323846;
    const uint32_t N = n / 2u, M = N / 2u;
    VorbisTab tab = {};
    tab.a = (uint32_t)t->size();
    for (uint32_t m = 0; m < M; m++) { const double x = -pi * (4.0 * m + 1.0) / (4.0 * N); t->push_back((float)std::cos(x)); t->push_back((float)std::sin(x)); }
    tab.b = (uint32_t)t->size();
    for (uint32_t k = 0; k < M; k++) { const double x = -pi * k / N; t->push_back((float)std::cos(x)); t->push_back((float)std::sin(x)); }
    tab.w = (uint32_t)t->size();
    for (uint32_t j = 0; j < M / 2u; j++) { const double x = -2.0 * pi * j / M; t->push_back((float)std::cos(x)); t->push_back((float)std::sin(x)); }
    tab.slope = (uint32_t)t->size();
    t->resize(t->size() + N);
    window_slope(n, t->data() + tab.slope);
    if (plain) {
        tab.cos8 = (uint32_t)t->size();
        for (uint32_t j = 0; j < 8u * N; j++) t->push_back((float)std::cos(2.0 * pi * j / (8.0 * N)));
    }
    return tab;
}

int vorbis_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const void* images, uint64_t images_bytes)
{
    VorbisState& v = *b->vorbis;
    OHGPU_TRY(state_events(v, 5));
    if (v.packets.empty()) return OHGPU_OK;
    std::vector<float> tables(256);
    db_table(tables.data());
    uint64_t rows = 0, blocks = 0, cls = 0;
    for (Stream& s : v.streams) {
        s.row_base = rows; s.block_base = blocks; s.class_base = cls;
        rows += (uint64_t)s.n_packets * s.channels * (s.bs1 / 2u);
        blocks += (uint64_t)s.n_packets * s.channels * s.bs1;
        cls += (uint64_t)s.n_packets * s.class_bytes;
        if (!s.n_packets) continue;
        v.max_channels = std::max(v.max_channels, s.channels);
        v.max_block = std::max(v.max_block, s.bs1);
        for (uint32_t n : {s.bs0, s.bs1}) {
            const uint32_t lg = ilog(n) - 1u;
            if (!v.tabs[lg].slope) v.tabs[lg] = make_tables(n, v.plain, &tables);
        }
    }
    v.rows_bytes = (size_t)rows * sizeof(float);
    OHGPU_TRY(dev_array(ctx, v, &v.d_images, (size_t)(images_bytes / 4u), (const uint32_t*)images));
    OHGPU_TRY(dev_array(ctx, v, &v.d_streams, v.streams.size(), v.streams.data()));
    OHGPU_TRY(dev_array(ctx, v, &v.d_packets, v.packets.size(), v.packets.data()));
    OHGPU_TRY(dev_array<Rec>(ctx, v, &v.d_recs, v.packets.size()));
    OHGPU_TRY(dev_array<FloorOut>(ctx, v, &v.d_floors, v.packets.size() * kMaxChannels));
    OHGPU_TRY(dev_array<float>(ctx, v, &v.d_rows, (size_t)rows));
    OHGPU_TRY(dev_array<float>(ctx, v, &v.d_blocks, (size_t)blocks));
    OHGPU_TRY(dev_array<uint8_t>(ctx, v, &v.d_cls, (size_t)cls));
    OHGPU_TRY(dev_array(ctx, v, &v.d_tables, tables.size(), tables.data()));
    return OHGPU_OK;
}

int vorbis_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    VorbisState& v = *b->vorbis;
    OHGPU_TRY(run_begin(v, s));
    const uint32_t np = (uint32_t)v.packets.size(), ns = (uint32_t)v.streams.size();
    const Stream* streams = (const Stream*)v.d_streams;
    const Packet* packets = (const Packet*)v.d_packets;
    const uint32_t* images = (const uint32_t*)v.d_images;
    Rec* recs = (Rec*)v.d_recs;
    FloorOut* floors = (FloorOut*)v.d_floors;
    float* rows = (float*)v.d_rows;
    float* blocks = (float*)v.d_blocks;
    VorbisTabs tabs;
    memcpy(tabs.t, v.tabs, sizeof(tabs.t));
    const uint32_t packet_blocks = (np + kVbLanes - 1) / kVbLanes;
    OHGPU_HIP_TRY(hipEventRecord(v.ev[0], s));
    if (np) {
        OHGPU_HIP_TRY(hipMemsetAsync(rows, 0, v.rows_bytes, s));
        hipLaunchKernelGGL(vorbis_head_kernel, dim3(packet_blocks), dim3(kVbLanes), 0, s, streams, packets, np, images, src, recs);
        OHGPU_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(vorbis_scan_kernel, dim3((ns + kVbLanes - 1) / kVbLanes), dim3(kVbLanes), 0, s, streams, ns, recs);
        OHGPU_HIP_TRY(hipGetLastError());
    }
    OHGPU_HIP_TRY(hipEventRecord(v.ev[1], s));
    if (np) {
        hipLaunchKernelGGL(vorbis_entropy_kernel, dim3(packet_blocks), dim3(kVbLanes), 0, s, streams, packets, np, images, src, (const Rec*)recs, rows, floors, (uint8_t*)v.d_cls);
        OHGPU_HIP_TRY(hipGetLastError());
    }
    OHGPU_HIP_TRY(hipEventRecord(v.ev[2], s));
    if (np) {
        if (v.plain) hipLaunchKernelGGL(vorbis_synth_kernel<true>, dim3(np, v.max_channels), dim3(kVbThreads), 0, s, streams, packets, images, (const Rec*)recs, (const FloorOut*)floors, rows, blocks, (const float*)v.d_tables, tabs);
        else hipLaunchKernelGGL(vorbis_synth_kernel<false>, dim3(np, v.max_channels), dim3(kVbThreads), 0, s, streams, packets, images, (const Rec*)recs, (const FloorOut*)floors, rows, blocks, (const float*)v.d_tables, tabs);
        OHGPU_HIP_TRY(hipGetLastError());
    }
    OHGPU_HIP_TRY(hipEventRecord(v.ev[3], s));
    if (np) {
        hipLaunchKernelGGL(vorbis_store_kernel, dim3(np, (v.max_block / 2u + kVbThreads - 1) / kVbThreads), dim3(kVbThreads), 0, s, streams, packets, (const Rec*)recs, (const float*)blocks, dst);
        OHGPU_HIP_TRY(hipGetLastError());
    }
    return run_end(v, s);
}

}  // namespace ohgpu
