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

#include "api_file.h"

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
                                                                                   const PieceGroup* __restrict__ groups, const uint8_t* __restrict__ src,
                                                                                   uint8_t* __restrict__ dst)
{
    const PieceGroup g = groups[blockIdx.x];
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
    // a run has no more than room_pieces pieces, whatever the walk finds
    return file_plan(ctx, *b->file, "ohgpu_dsd_file_batch_create", streams, sizeof(Result), sizeof(Rec),
                     [](const Stream& st) -> uint64_t { return (room_pieces(st) + kDsdFileGroupPieces - 1u) / kDsdFileGroupPieces; });
}

int dsd_file_run(ohgpu_ctx*, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    return file_run(*b->file, src, dst, s, dsd_file_plain_kernel, dsd_file_walk_kernel, dsd_file_convert_kernel, kDsdFileGroupPieces * 64u);
}

}  // namespace ohgpu
