// dsd_file_kernel.hip -- DSF and DFF files on the device (the formats' text is csrc/dsd_file_core.h).
//   walk     a lane per stream: the chunks, the format, where the audio lies, the result record and the record of the conversion
//            (kind, audio position, first chunk, chunk count, where the 0x69 fill begins and ends).  Serial by nature, like the PCM
//            file walk.
//   convert  a workgroup of kDsdFileGroupPieces waves per stream and kDsdFileGroupPieces pieces of its room (the list of workgroups is
//            made at create from dst_bytes_capacity, which bounds any walk's run).  A wave takes a piece of dsdfile::kPieceChunks
//            chunks, reads the walk's record through a uniform index and leaves at once when its piece lies behind the run.  A lane
//            takes eight chunks: the aligned 16-byte lines that cover sixteen bytes of each DSF plane, or 32 consecutive DFF bytes,
//            joined by v_alignbyte_b32 under the stream's one phase, v_bfrev_b32 for DSF, one v_perm_b32 per output dword through
//            csrc/dsd_perm.h's selectors, and two, three or four 16-byte non-temporal stores (registers only: no LDS, no scratch).
//            What is not a whole lane, a unit whose lines do not lie whole inside the stream, P above 4 and the 0x69 fill go byte by
//            byte -- never as a read-modify-write of a dword.
//   plain    (kernel variant 1) one launch, a lane per stream: the walk and the byte-wise conversion.
// Every load lies inside the dwords that lie whole inside a stream's range, which ohgpu_dsd_file_batch_check placed inside the source
// arena (the walk's field reads: the aligned dwords that hold the range, the contract of ohgpu_iff_batch_run); every store lies inside
// [dst_offset, + dst_bytes_capacity), which the same check placed inside the destination arena and apart from every other stream's.
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

using namespace dsdfile;

__global__ __launch_bounds__(64) void dsd_file_walk_kernel(const Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, Result* __restrict__ results,
                                                           Rec* __restrict__ recs)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    walk(s, src + s.src_offset, &results[i], &recs[i]);
}

__global__ __launch_bounds__(64) void dsd_file_plain_kernel(const Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            Result* __restrict__ results, Rec* __restrict__ recs)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    Result r;
    Rec c;
    walk(s, src + s.src_offset, &r, &c);
    if (c.n) {
        convert_bytes(c, src + s.src_offset + c.data_offset, dst + c.dst_pos, 0, c.fill_from, 0, 1);
        fill_bytes(dst + c.dst_pos, c.fill_from, c.fill_to, 0, 1);
    }
    results[i] = r;
    recs[i] = c;
}

__global__ __launch_bounds__(kDsdFileGroupPieces * 64) void dsd_file_convert_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs,
                                                                                   const DsdFileGroup* __restrict__ groups, const uint8_t* __restrict__ src,
                                                                                   uint8_t* __restrict__ dst)
{
    const DsdFileGroup g = groups[blockIdx.x];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const Rec c = recs[g.stream];
    const uint32_t piece = g.group * kDsdFileGroupPieces + wave;
    if ((uint64_t)piece * kPieceChunks >= c.n) return;                  // (a run of no chunks has no fill either)
    const Stream s = streams[g.stream];
    const uint8_t* const base = src + s.src_offset;
    uint8_t* const to = dst + c.dst_pos;
    convert_piece(c, base + c.data_offset, base + s.src_bytes, to, piece, ((uintptr_t)to & 15u) == 0u, lane, 64u);
}

int dsd_file_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Stream* streams)
{
    DsdFileState& g = *b->dsdfile;
    OHGPU_TRY(state_events(g, 3));
    if (!g.n_streams) return OHGPU_OK;
    std::vector<DsdFileGroup> groups;
    for (size_t i = 0; i < g.n_streams; i++) {
        // a run has no more than room_pieces pieces, whatever the walk finds
        const uint64_t pieces = room_pieces(streams[i]), want = (pieces + kDsdFileGroupPieces - 1u) / kDsdFileGroupPieces;
        g.writes = g.writes || pieces != 0u;
        if (g.plain) continue;
        if (groups.size() + want > 0x7fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_batch_create: the destination ranges are more than one batch takes");
        for (uint64_t k = 0; k < want; k++) groups.push_back(DsdFileGroup{(uint32_t)i, (uint32_t)k});
    }
    g.n_groups = (uint32_t)groups.size();
    OHGPU_TRY(dev_array(ctx, g, &g.d_streams, g.n_streams, streams));
    OHGPU_TRY(dev_array<Result>(ctx, g, &g.d_results, g.n_streams));
    OHGPU_TRY(dev_array<Rec>(ctx, g, &g.d_recs, g.n_streams));
    OHGPU_TRY(dev_array(ctx, g, &g.d_groups, g.n_groups, groups.data()));
    return OHGPU_OK;
}

void dsd_file_free(ohgpu_ctx* ctx, ohgpu_batch* b)
{
    if (!b->dsdfile) return;
    state_release(ctx, *b->dsdfile);
    delete b->dsdfile;
    b->dsdfile = nullptr;
}

int dsd_file_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    DsdFileState& g = *b->dsdfile;
    OHGPU_TRY(run_begin(g, s));      // (the records serve one run at a time)
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u;
    const Stream* const streams = (const Stream*)g.d_streams;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    if (g.plain) {
        hipLaunchKernelGGL(dsd_file_plain_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, dst, (Result*)g.d_results, (Rec*)g.d_recs);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
        return run_end(g, s);
    }
    hipLaunchKernelGGL(dsd_file_walk_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, (Result*)g.d_results, (Rec*)g.d_recs);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
    if (g.n_groups) {
        hipLaunchKernelGGL(dsd_file_convert_kernel, dim3(g.n_groups), dim3(kDsdFileGroupPieces * 64), 0, s, streams, (const Rec*)g.d_recs, (const DsdFileGroup*)g.d_groups, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(g, s);
}

}  // namespace ohgpu
