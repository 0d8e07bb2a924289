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

#include "api_file.h"

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

__global__ __launch_bounds__(kIffThreads) void iff_convert_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs, const PieceGroup* __restrict__ groups,
                                                                  const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const PieceGroup g = groups[blockIdx.x];
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
    return file_plan(ctx, *b->file, "ohgpu_iff_batch_create", streams, sizeof(Result), sizeof(Rec), [](const Stream& st) -> uint64_t {
        // a run has no more than dst_bytes_capacity / 16 pieces; its first workgroup is there for the edges of a run without pieces
        const uint64_t pieces = st.dst_bytes_capacity / 16u, whole = (pieces + kIffGroupPieces - 1u) / kIffGroupPieces;
        return st.dst_bytes_capacity == 0u ? 0u : whole ? whole : 1u;
    });
}

int iff_run(ohgpu_ctx*, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    return file_run(*b->file, src, dst, s, iff_plain_kernel, iff_walk_kernel, iff_convert_kernel, kIffThreads);
}

}  // namespace ohgpu
