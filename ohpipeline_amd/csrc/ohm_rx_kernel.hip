// ohm_rx_kernel.hip -- the Songcast receiver on the device (the text of all three phases is csrc/ohm_rx_core.h).
//   parse      a lane per datagram, one launch sized to the table: fourteen aligned dword loads, a record of 104 bytes out.
//   sequence   a lane per stream, one launch sized to the stream table: the frame sequencer over the stream's records in arrival
//              order; its window is four named 64-bit words chosen by selects and walked by bit scans, so the whole state machine
//              stays in registers (no scratch memory: the build's resource report says 0 bytes a lane for all three kernels); its
//              ring of 256 datagram indices is a workspace of the batch.  Latency-bound
//              by construction (one lane walks a stream); it is there so that the gather needs no host in front of it.
//   gather     the wide one.  A wave per datagram, the launch capped at kGatherGroupsPerCu workgroups a CU, every wave going round
//              the table in strides of the launch's waves.  The record and the datagram's place are read through a wave-uniform
//              index (scalar loads); a record that is not OUTPUT costs those two loads.  Whole 16-byte destination lines are one
//              store each, from five aligned source dwords through a byte funnel (a 64-bit shift); edges go byte by byte, never as a
//              read-modify-write of a dword: neighbouring datagrams of a stream abut inside one dword.
// Every load lies inside a datagram that ohgpu_ohm_rx_batch_check placed inside the source arena, every store inside the stream's
// run, which the same check sized from the table alone (the sum of max(bytes - 58, 0) bounds any parse's audio).
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

using namespace ohmrx;

constexpr uint32_t kRxThreads = 256, kRxWaves = kRxThreads / 64;
constexpr uint32_t kGatherGroupsPerCu = 8;

__global__ __launch_bounds__(kRxThreads) void ohm_rx_parse_kernel(const Datagram* __restrict__ grams, uint32_t n, const uint8_t* __restrict__ src, Record* __restrict__ recs)
{
    const uint32_t k = blockIdx.x * kRxThreads + threadIdx.x;
    if (k >= n) return;
    const Datagram g = grams[k];
    parse(src + g.src_offset, g.bytes, &recs[k]);
}

__global__ __launch_bounds__(64) void ohm_rx_sequence_kernel(const Stream* __restrict__ streams, uint32_t n, Record* __restrict__ recs, uint32_t* __restrict__ rings,
                                                             StreamResult* __restrict__ results)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    sequence(s, recs + s.first_datagram, rings + (size_t)i * kRing, &results[i]);
}

__global__ __launch_bounds__(kRxThreads) void ohm_rx_gather_kernel(const Datagram* __restrict__ grams, const Record* __restrict__ recs, uint32_t n,
                                                                   const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u);      // (the same in every lane: says so to the compiler)
    const uint32_t stride = gridDim.x * kRxWaves;
    for (uint32_t k = blockIdx.x * kRxWaves + wave; k < n; k += stride) {
        const Record& r = recs[k];
        if (r.disposition != kOutput || r.audio_bytes == 0) continue;
        gather_lane(src + grams[k].src_offset + r.audio_offset, dst + r.dst_offset, r.audio_bytes, threadIdx.x % 64u, 64u);
    }
}

uint32_t ohm_rx_gather_blocks(uint32_t n_datagrams, uint32_t cus)
{
    const uint32_t want = (n_datagrams + kRxWaves - 1) / kRxWaves, cap = cus * kGatherGroupsPerCu;
    return want < cap ? want : cap;
}

int ohm_rx_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Stream* streams, const Datagram* datagrams)
{
    OhmRxState& r = *b->ohmrx;
    OHGPU_TRY(state_events(r, 4));
    OHGPU_TRY(dev_array(ctx, r, &r.d_streams, r.n_streams, streams));
    OHGPU_TRY(dev_array<StreamResult>(ctx, r, &r.d_results, r.n_streams));
    OHGPU_TRY(dev_array<uint32_t>(ctx, r, &r.d_rings, r.n_streams * kRing));
    OHGPU_TRY(dev_array(ctx, r, &r.d_datagrams, r.n_datagrams, datagrams));
    OHGPU_TRY(dev_array<Record>(ctx, r, &r.d_records, r.n_datagrams));
    return OHGPU_OK;
}

int ohm_rx_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    OhmRxState& r = *b->ohmrx;
    OHGPU_TRY(run_begin(r, s));      // (the records serve one run at a time)
    const uint32_t ng = (uint32_t)r.n_datagrams, ns = (uint32_t)r.n_streams;
    const uint32_t cus = ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256u;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(r.ev[0], s));
    if (ng) {
        hipLaunchKernelGGL(ohm_rx_parse_kernel, dim3((ng + kRxThreads - 1) / kRxThreads), dim3(kRxThreads), 0, s, (const Datagram*)r.d_datagrams, ng, src, (Record*)r.d_records);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(r.ev[1], s));
    if (ns) {
        hipLaunchKernelGGL(ohm_rx_sequence_kernel, dim3((ns + 63u) / 64u), dim3(64), 0, s, (const Stream*)r.d_streams, ns, (Record*)r.d_records, (uint32_t*)r.d_rings,
                           (StreamResult*)r.d_results);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(r.ev[2], s));
    if (ng) {
        hipLaunchKernelGGL(ohm_rx_gather_kernel, dim3(ohm_rx_gather_blocks(ng, cus)), dim3(kRxThreads), 0, s, (const Datagram*)r.d_datagrams, (const Record*)r.d_records, ng, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(r, s);
}

}  // namespace ohgpu
