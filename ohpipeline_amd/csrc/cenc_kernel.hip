// cenc_kernel.hip -- protected fragmented MPEG-4 on the device (the text is csrc/cenc_core.h over csrc/mp4_frag_core.h).
//   walk            a lane per stream: mp4frag's walk under cenc::Protection -- the result's head, what the protection boxes gave, the
//                   stream's record and a record a run, which also says where the run's first IV lies.
//   run sums, carries, expand, finish
//                   csrc/mp4_frag_kernel.hip's own launches (mp4f_tables), on this batch's tables: the expansion's packet rows are places
//                   in the SOURCE arena and stay the batch's own.
//   decrypt-gather  three launches where the sibling's gather stands:
//       rows        a workgroup per tile of the expansion: the public packet row of every sample (its place in the destination arena is
//                   the gather's own arithmetic, no scan), its IV's place, and the exclusive prefix of ceil(size / 16) over the tile's
//                   gathered rows; the tile's sum.
//       tiles       a lane per stream, serial over its tiles: the sums become the blocks in front of each tile; the stream's blocks.
//       crypt       persistent, a wave per chunk of 64 consecutive keystream blocks of one stream, a lane a block.  The chunk slots are
//                   laid out at create from the capacities (a stream has at most dst_capacity / 16 + packet_capacity blocks); a wave
//                   that meets a slot behind its stream's last block steps to the next stream's first slot.  The stream is the same for
//                   the whole wave, so its schedule is read through a wave-uniform index and stays in scalar registers; a lane finds
//                   its sample by two searches (the stream's tiles, the tile's rows) and then runs cenc::crypt_lane: the counter block,
//                   ten rounds on Te0 in the LDS (1 KB a workgroup; the reads are data-dependent, so bank conflicts are part of the
//                   cost), the block's bytes through aligned dwords and the funnel, one 16-byte store at the destination's own address,
//                   or bytes for a sample's last partial block.  A clear stream's blocks take the same way with no keystream.
//   plain           (kernel variant 1) one launch, a lane per stream: all of it in the serial text the CPU driver runs, the cipher
//                   included, with Te0 read from constant memory.
// Loads: the walk's are mp4_frag_kernel.hip's; an IV lies inside a senc that the walk held to its box; a sample is read only when
// emit() found it inside the stream, in the aligned dwords that hold it.  Stores: the stream's rows and run slots, its own records, or
// [dst_offset, + bytes_gathered <= dst_capacity).
// The scan, the tiles' prefix, the persistent loop and its searches, the plan of the slots and the run around the launches are
// csrc/protected_shell.h's (over csrc/frag_units.h), shared with csrc/cbcs_kernel.hip: this file has the kernels' own parts.
#include "protected_shell.h"

namespace ohgpu {

constexpr cenc::Forward kCencHostForward = cenc::make_forward();
__constant__ const cenc::Forward kCencForward = kCencHostForward;

__global__ __launch_bounds__(64) void cenc_walk_kernel(const cenc::Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, Result* __restrict__ results,
                                                       cenc::Extra* __restrict__ extras, Rec* __restrict__ recs, RunRec* __restrict__ runrecs)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const cenc::Stream s = streams[i];
    cenc::walk(s, src + s.s.src_offset, false, &results[i], &extras[i], &recs[i], runrecs + s.s.run_first);
}

__global__ __launch_bounds__(kProtThreads) void cenc_rows_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs, const RunRec* __restrict__ runrecs,
                                                                 const Mp4fTile* __restrict__ tiles, const Result* __restrict__ results, const cenc::Extra* __restrict__ extras,
                                                                 const Row* __restrict__ src_rows, Row* __restrict__ rows, cenc::RowRec* __restrict__ rowrecs,
                                                                 uint64_t* __restrict__ tile_blocks)
{
    __shared__ uint64_t part[kProtWaves];
    const Mp4fTile tile = tiles[blockIdx.x];
    const Rec rec = recs[tile.stream];
    if (tile.s0 >= rec.rows) return;                                  // (uniform over the workgroup)
    const Stream st = streams[tile.stream];
    const Result& res = results[tile.stream];
    const RunRec* const runs = runrecs + st.run_first;
    const bool prot = extras[tile.stream].is_protected != 0u;
    const uint32_t iv_size = extras[tile.stream].iv_size;
    const uint32_t first = tile.s0 + threadIdx.x * kProtPerThread;
    uint32_t n[kProtPerThread], iv_pos[kProtPerThread];
    for (uint32_t k = 0; k < kProtPerThread; k++) {
        const uint32_t s = first + k;
        n[k] = iv_pos[k] = 0;
        if (s >= rec.rows) continue;
        Row from;
        uint32_t k_run;
        if (public_row(st, rec, res, runs, src_rows, rows, s, &from, &k_run)) {
            n[k] = cenc::blocks_of(from.bytes);
            if (prot) iv_pos[k] = runs[k_run].iv_pos + (s - runs[k_run].first_sample) * iv_size;
        }
    }
    uint64_t before, total;
    tile_exclusive_scan(n, part, &before, &total);
    for (uint32_t k = 0; k < kProtPerThread; k++) {
        const uint32_t s = first + k;
        if (s < rec.rows) {
            cenc::RowRec r;
            r.block_first = before; r.iv_pos = iv_pos[k]; r.pad = 0;
            rowrecs[st.packet_first + s] = r;
        }
        before += n[k];
    }
    if (threadIdx.x == kProtThreads - 1u) tile_blocks[blockIdx.x] = total;
}

__global__ __launch_bounds__(64) void cenc_tiles_kernel(uint32_t n, const Rec* __restrict__ recs, const uint32_t* __restrict__ tile_first, uint64_t* __restrict__ tile_blocks,
                                                        uint64_t* __restrict__ nblocks, cenc::Extra* __restrict__ extras)
{
    tiles_body(n, recs, tile_first, tile_blocks, nblocks, extras, [=](uint32_t i, uint64_t blocks) { return extras[i].is_protected ? blocks : 0u; });
}

__global__ __launch_bounds__(kProtThreads) void cenc_crypt_kernel(const Stream* __restrict__ streams, uint32_t n_streams, const Rec* __restrict__ recs,
                                                                  const cenc::Extra* __restrict__ extras, const uint32_t* __restrict__ tile_first,
                                                                  const uint64_t* __restrict__ tile_blocks, const uint64_t* __restrict__ chunk_first, uint64_t n_chunks,
                                                                  const uint64_t* __restrict__ nblocks, const uint32_t* __restrict__ keys, const Row* __restrict__ src_rows,
                                                                  const Row* __restrict__ rows, const cenc::RowRec* __restrict__ rowrecs, const uint8_t* __restrict__ src,
                                                                  uint8_t* __restrict__ dst)
{
    __shared__ uint32_t te0[256];
    te0[threadIdx.x] = kCencForward.te0[threadIdx.x];
    __syncthreads();
    const uint32_t* const table = te0;
    unit_loop(streams, n_streams, recs, tile_first, tile_blocks, chunk_first, n_chunks, nblocks, [=](uint32_t r) { return rowrecs[r].block_first; },
        [=](uint32_t i, const Stream& st, uint32_t r, uint32_t j) {
            const Row from = src_rows[r], to = rows[r];
            const bool prot = extras[i].is_protected != 0u;
            cenc::Iv iv = {};
            if (prot) iv = cenc::read_iv(src + st.src_offset, rowrecs[r].iv_pos, extras[i].iv_size);
            cenc::crypt_lane(src + from.src_offset, dst + to.src_offset, from.bytes, j, prot ? keys + (size_t)i * cenc::kScheduleWords : nullptr, iv, table);
        });
}

__global__ __launch_bounds__(64) void cenc_plain_kernel(const cenc::Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        Result* __restrict__ results, cenc::Extra* __restrict__ extras, Rec* __restrict__ recs, RunRec* __restrict__ runrecs,
                                                        Run* __restrict__ runs, Row* __restrict__ src_rows, Row* __restrict__ rows, Sample* __restrict__ samples,
                                                        const uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const cenc::Stream cs = streams[i];
    const Stream& s = cs.s;
    const uint8_t* const base = src + s.src_offset;
    RunRec* const my = runrecs + s.run_first;
    Result r;
    Rec rec;
    cenc::Extra x;
    cenc::walk(cs, base, false, &r, &x, &rec, my);
    for (uint32_t k = 0; k < rec.runs_written; k++)
        if (needs_sums(my[k])) totals_serial(base, my[k], my[k].samples, &my[k].bytes, &my[k].frames);
    carries(s, &rec, my, runs + s.run_first, &r);
    expand_serial(s, base, rec, my, src_rows + s.packet_first, samples + s.packet_first, &r);
    finish(s, &rec, my, src_rows + s.packet_first, &r);
    cenc::gather_serial(cs, src, dst, rec, my, src_rows + s.packet_first, r, keys + (size_t)i * cenc::kScheduleWords, kCencForward.te0, rows + s.packet_first, &x);
    results[i] = r;
    extras[i] = x;
    recs[i] = rec;
}

int cenc_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const cenc::Stream* streams)
{
    CencState& g = *b->cenc;
    const size_t n = g.n_streams;
    std::vector<Stream> plain(n);
    std::vector<cenc::Stream> stripped(streams, streams + n);          // the device's copy has no key: the schedules are all it gets
    for (size_t i = 0; i < n; i++) {
        plain[i] = streams[i].s;
        for (uint8_t& k : stripped[i].key) k = 0;
    }
    return protected_plan<cenc::RowRec>(ctx, g, plain, stripped, "ohgpu_cenc_batch_create", [](size_t) { return 0u; });
}

int cenc_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    CencState& g = *b->cenc;
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u;
    const cenc::Stream* const cstreams = (const cenc::Stream*)g.d_cstreams;
    Result* const results = (Result*)g.d_results;
    cenc::Extra* const extras = (cenc::Extra*)g.d_extras;
    Rec* const recs = (Rec*)g.d_recs;
    RunRec* const runrecs = (RunRec*)g.d_runrecs;
    const uint32_t* const keys = (const uint32_t*)g.d_keys;
    return protected_run(g, src, s,
        [&] {
            hipLaunchKernelGGL(cenc_plain_kernel, dim3(lane_blocks), dim3(64), 0, s, cstreams, ns, src, dst, results, extras, recs, runrecs, (Run*)g.d_runs, (Row*)g.d_packets,
                               (Row*)g.d_rows, (Sample*)g.d_samples, keys);
        },
        [&] { hipLaunchKernelGGL(cenc_walk_kernel, dim3(lane_blocks), dim3(64), 0, s, cstreams, ns, src, results, extras, recs, runrecs); },
        [&]() -> int {
            if (!g.n_tiles) return OHGPU_OK;
            hipLaunchKernelGGL(cenc_rows_kernel, dim3(g.n_tiles), dim3(kProtThreads), 0, s, (const Stream*)g.d_streams, (const Rec*)recs, (const RunRec*)runrecs,
                               (const Mp4fTile*)g.d_tiles, (const Result*)results, (const cenc::Extra*)extras, (const Row*)g.d_packets, (Row*)g.d_rows,
                               (cenc::RowRec*)g.d_row_first, (uint64_t*)g.d_tile_units);
            OHGPU_HIP_TRY_ALLOC(hipGetLastError());
            hipLaunchKernelGGL(cenc_tiles_kernel, dim3(lane_blocks), dim3(64), 0, s, ns, (const Rec*)recs, (const uint32_t*)g.d_tile_first, (uint64_t*)g.d_tile_units,
                               (uint64_t*)g.d_nunits, extras);
            OHGPU_HIP_TRY_ALLOC(hipGetLastError());
            if (!g.crypt_blocks) return OHGPU_OK;
            hipLaunchKernelGGL(cenc_crypt_kernel, dim3(g.crypt_blocks), dim3(kProtThreads), 0, s, (const Stream*)g.d_streams, ns, (const Rec*)recs, (const cenc::Extra*)extras,
                               (const uint32_t*)g.d_tile_first, (const uint64_t*)g.d_tile_units, (const uint64_t*)g.d_chunk_first, g.n_chunks, (const uint64_t*)g.d_nunits, keys,
                               (const Row*)g.d_packets, (const Row*)g.d_rows, (const cenc::RowRec*)g.d_row_first, src, dst);
            OHGPU_HIP_TRY_ALLOC(hipGetLastError());
            return OHGPU_OK;
        });
}

}  // namespace ohgpu
