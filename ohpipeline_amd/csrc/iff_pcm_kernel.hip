// iff_pcm_kernel.hip -- WAV, AIFF and AIFC files on the device (the formats' text is csrc/iff_chunk_core.h).
//   walk     a lane per stream: the chunks, the format, where the audio lies, the result record and the record of the conversion
//            (source position, output bytes, sample widths, byte order, mode).  Serial by nature, like the MPEG-4 walk.
//   convert  a workgroup per kIffGroupPieces pieces of one stream's destination run (the list of workgroups is made at create from
//            dst_bytes_capacity, which bounds any walk's run).  A workgroup reads the walk's record through a uniform index and leaves
//            at once when its first piece lies behind the run's last.  A piece is whole 16-byte lines of the destination: one store a
//            line from the aligned 16-byte source lines that hold its samples, through the funnel, a byte permute per output dword and the
//            funnel again (registers only: no LDS, no scratch).  A stream's first workgroup also moves the head and the tail of the
//            run byte by byte -- never as a read-modify-write of a dword: neighbouring runs may abut inside one.
//   plain    (kernel variant 1) one launch, a lane per stream: the walk and the byte-wise conversion.
// Every load lies inside the dwords that lie whole inside a stream's range, which ohgpu_iff_batch_check placed inside the source arena
// (the walk's field reads: the aligned dwords that hold the range, the contract of ohgpu_mp4_batch_run); every store lies inside
// [dst_offset, + dst_bytes_capacity), which the same check placed inside the destination arena and apart from every other stream's.
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

using namespace iffchunk;

constexpr uint32_t kIffThreads = 256;

__global__ __launch_bounds__(64) void iff_walk_kernel(const Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, Result* __restrict__ results,
                                                      Rec* __restrict__ recs)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    walk(s, src + s.src_offset, &results[i], &recs[i]);
}

__global__ __launch_bounds__(64) void iff_plain_kernel(const Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       Result* __restrict__ results, Rec* __restrict__ recs)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    Result r;
    Rec c;
    walk(s, src + s.src_offset, &r, &c);
    if (c.out_bytes) convert_bytes(c, src + s.src_offset + c.src_pos, dst + c.dst_pos, 0, c.out_bytes, 0, 1);
    results[i] = r;
    recs[i] = c;
}

__global__ __launch_bounds__(kIffThreads) void iff_convert_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs, const IffGroup* __restrict__ groups,
                                                                  const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const IffGroup g = groups[blockIdx.x];
    const Rec c = recs[g.stream];
    if (c.out_bytes == 0u) return;
    const uint8_t* const run = src + streams[g.stream].src_offset + c.src_pos;
    uint8_t* const to = dst + c.dst_pos;
    const Cut k = cut(c, (uintptr_t)run, (uintptr_t)to);
    const uint32_t first = g.group * kIffGroupPieces;
    if (first && first >= k.pieces) return;
    const uint32_t last = k.pieces - first < kIffGroupPieces ? k.pieces : first + kIffGroupPieces;
    if (first < k.pieces) convert_pieces_of(c, k, run, to, first, last, threadIdx.x, kIffThreads);
    if (first == 0u) {
        convert_bytes(c, run, to, 0, k.head, threadIdx.x, kIffThreads);
        convert_bytes(c, run, to, k.tail_from, c.out_bytes, threadIdx.x, kIffThreads);
    }
}

int iff_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Stream* streams)
{
    IffState& g = *b->iff;
    OHGPU_TRY(state_events(g, 3));
    if (!g.n_streams) return OHGPU_OK;
    std::vector<IffGroup> groups;
    for (size_t i = 0; i < g.n_streams; i++) g.writes = g.writes || streams[i].dst_bytes_capacity != 0u;
    if (!g.plain)
        for (size_t i = 0; i < g.n_streams; i++) {
            // a run has no more than dst_bytes_capacity / 16 pieces; its first workgroup is there for the edges of a run without pieces
            const uint64_t pieces = streams[i].dst_bytes_capacity / 16u, whole = (pieces + kIffGroupPieces - 1u) / kIffGroupPieces;
            const uint64_t want = streams[i].dst_bytes_capacity == 0u ? 0u : whole ? whole : 1u;
            for (uint64_t k = 0; k < want; k++) groups.push_back(IffGroup{(uint32_t)i, (uint32_t)k});
            if (groups.size() > 0x7fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_iff_batch_create: the destination ranges are more than one batch takes");
        }
    g.n_groups = (uint32_t)groups.size();
    OHGPU_TRY(dev_array(ctx, g, &g.d_streams, g.n_streams, streams));
    OHGPU_TRY(dev_array<Result>(ctx, g, &g.d_results, g.n_streams));
    OHGPU_TRY(dev_array<Rec>(ctx, g, &g.d_recs, g.n_streams));
    OHGPU_TRY(dev_array(ctx, g, &g.d_groups, g.n_groups, groups.data()));
    return OHGPU_OK;
}

void iff_free(ohgpu_ctx* ctx, ohgpu_batch* b)
{
    if (!b->iff) return;
    state_release(ctx, *b->iff);
    delete b->iff;
    b->iff = nullptr;
}

int iff_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    IffState& g = *b->iff;
    OHGPU_TRY(run_begin(g, s));      // (the records serve one run at a time)
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u;
    const Stream* const streams = (const Stream*)g.d_streams;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    if (g.plain) {
        hipLaunchKernelGGL(iff_plain_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, dst, (Result*)g.d_results, (Rec*)g.d_recs);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
        return run_end(g, s);
    }
    hipLaunchKernelGGL(iff_walk_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, (Result*)g.d_results, (Rec*)g.d_recs);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
    if (g.n_groups) {
        hipLaunchKernelGGL(iff_convert_kernel, dim3(g.n_groups), dim3(kIffThreads), 0, s, streams, (const Rec*)g.d_recs, (const IffGroup*)g.d_groups, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(g, s);
}

}  // namespace ohgpu
