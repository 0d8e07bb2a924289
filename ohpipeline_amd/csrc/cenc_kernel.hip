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
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

using namespace mp4frag;

constexpr uint32_t kCencThreads = 256, kCencWaves = kCencThreads / 64, kCencPerThread = kTile / kCencThreads;
constexpr uint32_t kCencGroupsPerCu = 8;
static_assert(kTile % kCencThreads == 0 && kCencThreads == 256, "a tile is a whole number of samples a thread; a thread stages one word of Te0");

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

__global__ __launch_bounds__(kCencThreads) void cenc_rows_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs, const RunRec* __restrict__ runrecs,
                                                                 const Mp4fTile* __restrict__ tiles, const Result* __restrict__ results, const cenc::Extra* __restrict__ extras,
                                                                 const Row* __restrict__ src_rows, Row* __restrict__ rows, cenc::RowRec* __restrict__ rowrecs,
                                                                 uint64_t* __restrict__ tile_blocks)
{
    __shared__ uint64_t part[kCencWaves];
    const Mp4fTile tile = tiles[blockIdx.x];
    const Rec rec = recs[tile.stream];
    if (tile.s0 >= rec.rows) return;                                  // (uniform over the workgroup)
    const Stream st = streams[tile.stream];
    const Result& res = results[tile.stream];
    const RunRec* const runs = runrecs + st.run_first;
    const bool prot = extras[tile.stream].is_protected != 0u;
    const uint32_t iv_size = extras[tile.stream].iv_size;
    const uint32_t tid = threadIdx.x, lane = tid % 64u, wave = tid / 64u, first = tile.s0 + tid * kCencPerThread;
    uint32_t n[kCencPerThread], iv_pos[kCencPerThread];
    uint64_t mine = 0;
    for (uint32_t k = 0; k < kCencPerThread; k++) {
        const uint32_t s = first + k;
        n[k] = iv_pos[k] = 0;
        if (s >= rec.rows) continue;
        Row out;
        out.src_offset = st.dst_offset; out.bytes = 0; out.reserved = 0;
        if (cenc::gathered_row(st, res, s)) {
            const uint32_t k_run = run_of(runs, rec.runs_written, s);
            const Row from = src_rows[st.packet_first + s];
            out.src_offset = cenc::row_place(st, rec, runs, k_run, from); out.bytes = from.bytes;
            n[k] = cenc::blocks_of(from.bytes);
            if (prot) iv_pos[k] = runs[k_run].iv_pos + (s - runs[k_run].first_sample) * iv_size;
        }
        uint4 v;
        __builtin_memcpy(&v, &out, 16);
        *reinterpret_cast<uint4*>(&rows[st.packet_first + s]) = v;
        mine += n[k];
    }
    uint64_t incl = mine;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63u) part[wave] = incl;
    __syncthreads();
    uint64_t before = incl - mine;
    for (uint32_t w = 0; w < wave; w++) before += part[w];
    for (uint32_t k = 0; k < kCencPerThread; k++) {
        const uint32_t s = first + k;
        if (s < rec.rows) {
            cenc::RowRec r;
            r.block_first = before; r.iv_pos = iv_pos[k]; r.pad = 0;
            rowrecs[st.packet_first + s] = r;
        }
        before += n[k];
    }
    if (tid == kCencThreads - 1u) tile_blocks[blockIdx.x] = before;
}

__global__ __launch_bounds__(64) void cenc_tiles_kernel(uint32_t n, const Rec* __restrict__ recs, const uint32_t* __restrict__ tile_first, uint64_t* __restrict__ tile_blocks,
                                                        uint64_t* __restrict__ nblocks, cenc::Extra* __restrict__ extras)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t t0 = tile_first[i], used = (recs[i].rows + kTile - 1u) / kTile;        // (rows <= packet_capacity: the stream has that many tiles)
    uint64_t acc = 0;
    for (uint32_t t = t0; t < t0 + used; t++) {
        const uint64_t v = tile_blocks[t];
        tile_blocks[t] = acc;
        acc += v;
    }
    nblocks[i] = acc;
    extras[i].blocks = extras[i].is_protected ? acc : 0u;
}

__global__ __launch_bounds__(kCencThreads) void cenc_crypt_kernel(const Stream* __restrict__ streams, uint32_t n_streams, const Rec* __restrict__ recs,
                                                                  const cenc::Extra* __restrict__ extras, const uint32_t* __restrict__ tile_first,
                                                                  const uint64_t* __restrict__ tile_blocks, const uint64_t* __restrict__ chunk_first, uint64_t n_chunks,
                                                                  const uint64_t* __restrict__ nblocks, const uint32_t* __restrict__ keys, const Row* __restrict__ src_rows,
                                                                  const Row* __restrict__ rows, const cenc::RowRec* __restrict__ rowrecs, const uint8_t* __restrict__ src,
                                                                  uint8_t* __restrict__ dst)
{
    __shared__ uint32_t te0[256];
    te0[threadIdx.x] = kCencForward.te0[threadIdx.x];
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
    const uint64_t stride = (uint64_t)gridDim.x * kCencWaves;
    for (uint64_t g = (uint64_t)blockIdx.x * kCencWaves + wave; g < n_chunks;) {
        uint32_t lo = 0, hi = n_streams;                              // the stream the slot lies in: the last whose first slot is <= g
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (chunk_first[mid] <= g) lo = mid; else hi = mid;
        }
        const uint32_t i = __builtin_amdgcn_readfirstlane(lo);
        const uint64_t total = nblocks[i], b0 = (g - chunk_first[i]) * cenc::kLaneBlocks;
        if (b0 >= total) {                                            // behind the stream's last block: on to the next stream's slots
            g += (chunk_first[i + 1u] - g + stride - 1u) / stride * stride;
            continue;
        }
        g += stride;
        const uint64_t b = b0 + lane;
        if (b >= total) continue;
        const Stream& st = streams[i];
        const uint32_t t0 = tile_first[i], used = (recs[i].rows + kTile - 1u) / kTile;
        uint32_t ta = 0, tb = used;                                   // the tile: the last whose first block is <= b
        while (tb - ta > 1u) {
            const uint32_t mid = ta + (tb - ta) / 2u;
            if (tile_blocks[t0 + mid] <= b) ta = mid; else tb = mid;
        }
        const uint64_t in_tile = b - tile_blocks[t0 + ta];
        const uint32_t s0 = ta * kTile, s1 = s0 + kTile < recs[i].rows ? s0 + kTile : recs[i].rows;
        const cenc::RowRec* const rr = rowrecs + st.packet_first;
        uint32_t ra = s0, rb = s1;                                    // the row: the last of the tile whose first block is <= in_tile
        while (rb - ra > 1u) {
            const uint32_t mid = ra + (rb - ra) / 2u;
            if (rr[mid].block_first <= in_tile) ra = mid; else rb = mid;
        }
        const uint32_t j = (uint32_t)(in_tile - rr[ra].block_first);
        const Row from = src_rows[st.packet_first + ra], to = rows[st.packet_first + ra];
        const bool prot = extras[i].is_protected != 0u;
        cenc::Iv iv = {};
        if (prot) iv = cenc::read_iv(src + st.src_offset, rr[ra].iv_pos, extras[i].iv_size);
        cenc::crypt_lane(src + from.src_offset, dst + to.src_offset, from.bytes, j, prot ? keys + (size_t)i * cenc::kScheduleWords : nullptr, iv, te0);
    }
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
    OHGPU_TRY(mp4f_plan(ctx, g, plain.data(), "ohgpu_cenc_batch_create"));
    if (!n) return OHGPU_OK;
    g.tile_first.assign(n + 1, 0);
    std::vector<uint64_t> chunk_first(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        const Stream& s = plain[i];
        g.tile_first[i + 1] = g.tile_first[i] + (g.plain ? 0u : (uint32_t)(((uint64_t)s.packet_capacity + kTile - 1u) / kTile));
        // sum of ceil(size / 16) over rows that fit the room: at most dst_capacity / 16 + packet_capacity
        const uint64_t blocks = s.packet_capacity && s.dst_capacity ? s.dst_capacity / 16u + s.packet_capacity : 0u;
        chunk_first[i + 1] = chunk_first[i] + (g.plain ? 0u : (blocks + cenc::kLaneBlocks - 1u) / cenc::kLaneBlocks);
    }
    g.n_chunks = chunk_first[n];
    const uint64_t want = (g.n_chunks + kCencWaves - 1u) / kCencWaves, cap = (uint64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * kCencGroupsPerCu;
    g.crypt_blocks = (uint32_t)(want < cap ? want : cap);
    g.keys_bytes = g.keys.size() * sizeof(uint32_t);
    OHGPU_TRY(dev_array(ctx, g, &g.d_cstreams, n, stripped.data()));
    OHGPU_TRY(dev_array(ctx, g, &g.d_keys, g.keys.size(), g.keys.data()));
    OHGPU_TRY(dev_array<cenc::Extra>(ctx, g, &g.d_extras, n));
    OHGPU_TRY(dev_array<Row>(ctx, g, &g.d_rows, g.n_packets));
    OHGPU_TRY(dev_array<cenc::RowRec>(ctx, g, &g.d_rowrecs, g.n_packets));
    OHGPU_TRY(dev_array(ctx, g, &g.d_tile_first, n + 1, g.tile_first.data()));
    OHGPU_TRY(dev_array<uint64_t>(ctx, g, &g.d_tile_blocks, g.n_tiles));
    OHGPU_TRY(dev_array(ctx, g, &g.d_chunk_first, n + 1, chunk_first.data()));
    OHGPU_TRY(dev_array<uint64_t>(ctx, g, &g.d_nblocks, n));
    return OHGPU_OK;
}

void cenc_free(ohgpu_ctx* ctx, ohgpu_batch* b)
{
    if (b->cenc) {
        CencState& g = *b->cenc;
        (void)hipDeviceSynchronize();
        // the schedules do not outlive the batch: the device block is cleared before it goes back to the cache, the host copy too
        if (g.d_keys) (void)hipMemset(g.d_keys, 0, g.keys_bytes);
        for (uint32_t& w : g.keys) *(volatile uint32_t*)&w = 0;
    }
    state_free(ctx, b->cenc);
}

int cenc_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    CencState& g = *b->cenc;
    OHGPU_TRY(run_begin(g, s));      // (the tables serve one run at a time)
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u;
    const cenc::Stream* const cstreams = (const cenc::Stream*)g.d_cstreams;
    Result* const results = (Result*)g.d_results;
    cenc::Extra* const extras = (cenc::Extra*)g.d_extras;
    Rec* const recs = (Rec*)g.d_recs;
    RunRec* const runrecs = (RunRec*)g.d_runrecs;
    const uint32_t* const keys = (const uint32_t*)g.d_keys;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    OHGPU_TRY(mp4f_fill(g, s));                                       // (no row of the run before stands in a table: csrc/mp4_frag_kernel.hip)
    if (g.n_packets) OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_rows, 0xa5, g.n_packets * sizeof(Row), s));
    if (g.plain) {
        hipLaunchKernelGGL(cenc_plain_kernel, dim3(lane_blocks), dim3(64), 0, s, cstreams, ns, src, dst, results, extras, recs, runrecs, (Run*)g.d_runs, (Row*)g.d_packets,
                           (Row*)g.d_rows, (Sample*)g.d_samples, keys);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        for (int k = 1; k < 6; k++) OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[k], s));
        return run_end(g, s);
    }
    hipLaunchKernelGGL(cenc_walk_kernel, dim3(lane_blocks), dim3(64), 0, s, cstreams, ns, src, results, extras, recs, runrecs);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_TRY(mp4f_tables(g, src, s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(cenc_rows_kernel, dim3(g.n_tiles), dim3(kCencThreads), 0, s, (const Stream*)g.d_streams, (const Rec*)recs, (const RunRec*)runrecs,
                           (const Mp4fTile*)g.d_tiles, (const Result*)results, (const cenc::Extra*)extras, (const Row*)g.d_packets, (Row*)g.d_rows,
                           (cenc::RowRec*)g.d_rowrecs, (uint64_t*)g.d_tile_blocks);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        hipLaunchKernelGGL(cenc_tiles_kernel, dim3(lane_blocks), dim3(64), 0, s, ns, (const Rec*)recs, (const uint32_t*)g.d_tile_first, (uint64_t*)g.d_tile_blocks,
                           (uint64_t*)g.d_nblocks, extras);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    if (g.n_tiles && g.crypt_blocks) {
        hipLaunchKernelGGL(cenc_crypt_kernel, dim3(g.crypt_blocks), dim3(kCencThreads), 0, s, (const Stream*)g.d_streams, ns, (const Rec*)recs, (const cenc::Extra*)extras,
                           (const uint32_t*)g.d_tile_first, (const uint64_t*)g.d_tile_blocks, (const uint64_t*)g.d_chunk_first, g.n_chunks, (const uint64_t*)g.d_nblocks, keys,
                           (const Row*)g.d_packets, (const Row*)g.d_rows, (const cenc::RowRec*)g.d_rowrecs, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(g, s);
}

}  // namespace ohgpu
