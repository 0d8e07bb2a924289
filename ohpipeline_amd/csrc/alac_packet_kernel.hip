// alac_packet_kernel.hip -- Apple Lossless packets on the device (the format text is csrc/alac_packet_core.h).
// One run is three phases, all queued on the stream:
//   entropy  a lane per packet, bit-serial: every element parsed, the residuals (or an escaped element's samples) to the packet's
//            rows of scratch, one record per channel beside them, the packet's status and sample count
//   predict  a lane per row, compressed channels of OK packets: the predictor recurrence in place
//   store    a workgroup per (group of rows, 64 samples): the tile goes through the LDS, so that it is read a row per lane and
//            written a sample per lane -- consecutive lanes to consecutive samples; the pair matrix, the shifted-off low bytes
//            (read straight from the packet: the entropy phase only noted where they begin) and the output form on the way
// Scratch is transposed: rows in groups of 64, sample i of row r of a group at word (group_base + i) * 64 + r, so that the 64 lanes of
// a wave of the predict phase, which run in lockstep, touch ONE 256-byte run per sample, and the entropy phase nearly so.  A packet's
// rows never straddle a group and a group holds rows of one frame length (alaccore::plan_rows).
// The plain route (a batch created under ohgpu_set_kernel_variant(1)) is one thread per packet doing everything, over the same groups
// laid out row by row.  Every load is bounded by the packet's bytes (alaccore::peek32), every row store by the frame length (a larger
// sample count fails the packet) and every destination store by the batch check's span of n_packets * frame_length samples.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "api_common.h"

namespace ohgpu {

using namespace alaccore;

constexpr uint32_t kAlacLanes = 64;
constexpr uint32_t kTile = 64;              // samples per store tile (and rows: kGroupRows)

__global__ __launch_bounds__(kAlacLanes) void alac_entropy_kernel(const Stream* __restrict__ streams, const Packet* __restrict__ packets, uint32_t n,
                                                                  const uint8_t* __restrict__ src, Chan* __restrict__ chans, int32_t* __restrict__ scratch,
                                                                  const uint64_t* __restrict__ group_base, PacketOut* __restrict__ outs)
{
    const uint32_t i = blockIdx.x * kAlacLanes + threadIdx.x;
    if (i >= n) return;
    const Packet pk = packets[i];
    const Stream s = streams[pk.stream];
    const TransposedRows rows{scratch, group_base, pk.row0};
    uint32_t samples = 0;
    const int st = parse_packet(src + pk.src_offset, pk.bytes, s, chans + pk.row0, rows, &samples);
    PacketOut o;
    o.status = (uint32_t)st;
    o.samples = st == kStatusOk ? samples : 0u;
    outs[i] = o;
}

__global__ __launch_bounds__(kAlacLanes) void alac_predict_kernel(const uint32_t* __restrict__ row_packet, uint32_t n_rows, const PacketOut* __restrict__ outs,
                                                                  const Chan* __restrict__ chans, int32_t* __restrict__ scratch, const uint64_t* __restrict__ group_base)
{
    const uint32_t r = blockIdx.x * kAlacLanes + threadIdx.x;
    if (r >= n_rows) return;
    const uint32_t p = row_packet[r];
    if (p == ~0u) return;
    const PacketOut o = outs[p];
    if (o.status != kStatusOk) return;
    predict_row(chans[r], transposed_row(scratch, group_base, r), o.samples);
}

__global__ __launch_bounds__(256) void alac_store_kernel(const Stream* __restrict__ streams, const Packet* __restrict__ packets, const uint32_t* __restrict__ row_packet,
                                                         const PacketOut* __restrict__ outs, const Chan* __restrict__ chans, const int32_t* __restrict__ scratch,
                                                         const uint64_t* __restrict__ group_base, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    __shared__ int32_t tile[kTile][kGroupRows + 1];
    const uint32_t g = blockIdx.x, i0 = blockIdx.y * kTile;
    const uint64_t base = group_base[g];
    const uint32_t length = (uint32_t)(group_base[g + 1] - base);           // the group's frame length
    if (i0 >= length) return;
    const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
    for (uint32_t k = wave; k < kTile; k += 4) tile[k][lane] = i0 + k < length ? scratch[(base + i0 + k) * kGroupRows + lane] : 0;
    __syncthreads();
    const uint32_t i = i0 + lane;
    for (uint32_t r = wave; r < kGroupRows; r += 4) {
        const uint32_t row = g * kGroupRows + r, p = row_packet[row];
        if (p == ~0u) continue;
        const PacketOut o = outs[p];
        if (o.status != kStatusOk || i >= o.samples) continue;
        const Packet pk = packets[p];
        const Stream s = streams[pk.stream];
        const Chan& ch = chans[row];
        const uint32_t partner = ch.place == 1 ? r + 1u : ch.place == 2 ? r - 1u : r;
        store_sample(s, dst, (uint64_t)pk.index * s.frame_length + i, row - pk.row0,
                     finish_sample(ch, tile[lane][r], tile[lane][partner], src + pk.src_offset, pk.bytes, i));
    }
}

// The plain route: one thread per packet does everything, straight from the bytes (its rows of scratch are its work space).
__global__ __launch_bounds__(kAlacLanes) void alac_plain_kernel(const Stream* __restrict__ streams, const Packet* __restrict__ packets, uint32_t n,
                                                                const uint8_t* __restrict__ src, Chan* __restrict__ chans, int32_t* __restrict__ scratch,
                                                                const uint64_t* __restrict__ group_base, uint8_t* __restrict__ dst, PacketOut* __restrict__ outs)
{
    const uint32_t i = blockIdx.x * kAlacLanes + threadIdx.x;
    if (i >= n) return;
    const Packet pk = packets[i];
    const Stream s = streams[pk.stream];
    const PlainRows rows{scratch, group_base, pk.row0};
    PacketOut o;
    decode_packet(src + pk.src_offset, pk, s, chans + pk.row0, rows, dst, &o);
    outs[i] = o;
}

int alac_plan(ohgpu_ctx* ctx, ohgpu_batch* b)
{
    AlacState& a = *b->alac;
    std::vector<uint64_t> group_base;
    std::vector<uint32_t> row_packet;
    plan_rows(a.streams.data(), a.packets.data(), a.packets.size(), &group_base, &row_packet);
    a.n_rows = (uint32_t)row_packet.size();
    a.n_groups = (uint32_t)group_base.size() - 1u;
    for (const Stream& s : a.streams) if (s.n_packets) a.max_frame_length = std::max(a.max_frame_length, s.frame_length);
    OHGPU_TRY(state_events(a, 4));
    if (a.packets.empty()) return OHGPU_OK;
    const size_t np = a.packets.size();
    OHGPU_TRY(dev_array(ctx, a, &a.d_streams, a.streams.size(), a.streams.data()));
    OHGPU_TRY(dev_array(ctx, a, &a.d_packets, np, a.packets.data()));
    OHGPU_TRY(dev_array<PacketOut>(ctx, a, &a.d_outs, np));
    OHGPU_TRY(dev_array<Chan>(ctx, a, &a.d_chans, a.n_rows));
    OHGPU_TRY(dev_array(ctx, a, &a.d_rowpacket, row_packet.size(), row_packet.data()));
    OHGPU_TRY(dev_array(ctx, a, &a.d_groupbase, group_base.size(), group_base.data()));
    a.rows_bytes = (size_t)group_base.back() * kGroupRows * sizeof(int32_t);
    OHGPU_TRY(dev_array<uint8_t>(ctx, a, &a.d_rows, a.rows_bytes));
    return OHGPU_OK;
}

int alac_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    AlacState& a = *b->alac;
    OHGPU_TRY(run_begin(a, s));
    const uint32_t np = (uint32_t)a.packets.size();
    const Stream* streams = (const Stream*)a.d_streams;
    const Packet* packets = (const Packet*)a.d_packets;
    PacketOut* outs = (PacketOut*)a.d_outs;
    Chan* chans = (Chan*)a.d_chans;
    int32_t* rows = (int32_t*)a.d_rows;
    const uint64_t* group_base = (const uint64_t*)a.d_groupbase;
    const uint32_t* row_packet = (const uint32_t*)a.d_rowpacket;
    const uint32_t packet_blocks = (np + kAlacLanes - 1) / kAlacLanes;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(a.ev[0], s));
    if (np && a.plain) {
        hipLaunchKernelGGL(alac_plain_kernel, dim3(packet_blocks), dim3(kAlacLanes), 0, s, streams, packets, np, src, chans, rows, group_base, dst, outs);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    } else if (np) {
        hipLaunchKernelGGL(alac_entropy_kernel, dim3(packet_blocks), dim3(kAlacLanes), 0, s, streams, packets, np, src, chans, rows, group_base, outs);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(a.ev[1], s));
    if (np && !a.plain) {
        hipLaunchKernelGGL(alac_predict_kernel, dim3((a.n_rows + kAlacLanes - 1) / kAlacLanes), dim3(kAlacLanes), 0, s, row_packet, a.n_rows,
                           (const PacketOut*)outs, (const Chan*)chans, rows, group_base);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(a.ev[2], s));
    if (np && !a.plain) {
        hipLaunchKernelGGL(alac_store_kernel, dim3(a.n_groups, (a.max_frame_length + kTile - 1) / kTile), dim3(256), 0, s, streams, packets, row_packet,
                           (const PacketOut*)outs, (const Chan*)chans, (const int32_t*)rows, group_base, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(a, s);
}

int alac_results(ohgpu_ctx* ctx, const ohgpu_batch* b, ohgpu_alac_packet_result* out)
{
    AlacState& a = *b->alac;
    if (a.packets.empty()) return OHGPU_OK;
    return fetch_after_run("ohgpu_alac_batch_results", a, out, a.d_outs, a.packets.size() * sizeof(PacketOut));
}

}  // namespace ohgpu
