// mp4_table_kernel.hip -- the MPEG-4 container on the device (the format's text is csrc/mp4_box_core.h).
//   walk     a lane per stream: the boxes, the taken trak's tables held to their rules, the result record and the record of where the
//            tables lie.  Serial by nature, like the Ogg chain.
//   sums     a workgroup per tile of kMp4Tile samples of one stream (the tile list is made at create, from packet_capacity): the sum of
//            the tile's stsz entries in 64 bits.  A table lies at any address: an entry is read as the aligned dwords that hold it.
//   carries  a wave per stream, four exclusive scans in turns of 64: the stream's tile sums, its stsc runs (S_k), its stts runs' samples
//            and frames.
//   expand   a workgroup per tile: the sizes' in-tile scan in LDS plus the tile's carry, the two searches, the chunk's offset, the range
//            and limit checks, one 16-byte store a lane into each table, the refusals counted and the lowest kept by atomics on the
//            result.  A chunk that began in an earlier tile is reached through the global prefix -- that tile's carry plus a sum over
//            its sizes, made once a workgroup -- never through another workgroup's LDS.  A last launch of a lane per stream turns
//            first_bad_sample into samples_available; it is timed with this phase.
//   plain    (kernel variant 1) one launch, a lane per stream: walk and expand_serial, the text the CPU driver runs.
// No workgroup waits for another inside a launch and no launch is persistent: the order of the phases is the launch boundary.
// Every load lies inside the aligned dwords that hold a stream's range, which ohgpu_mp4_batch_check placed inside the source arena (no
// dword load is misaligned; src_base is as hipMalloc gives it): the walk accepts a table only
// when its box lies inside the stream, and a row is expanded only from entries inside its table.  Every store lies inside the
// stream's rows [packet_first, + min(N, packet_capacity)), its carries (sized at create from packet_capacity) or its own records.
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

using namespace mp4box;
constexpr uint32_t kTile = kMp4Tile;

constexpr uint32_t kMp4Threads = 256, kMp4Waves = kMp4Threads / 64, kMp4PerThread = kTile / kMp4Threads;
static_assert(kTile % kMp4Threads == 0, "a tile is a whole number of samples a thread");

__global__ __launch_bounds__(64) void mp4_walk_kernel(const Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, Result* __restrict__ results,
                                                      Tables* __restrict__ tables)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    walk(s, src + s.src_offset, &results[i], &tables[i]);
}

__global__ __launch_bounds__(64) void mp4_plain_kernel(const Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, Result* __restrict__ results,
                                                       Tables* __restrict__ tables, Row* __restrict__ rows, Sample* __restrict__ samples)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    Result r;
    Tables t;
    walk(s, src + s.src_offset, &r, &t);
    if (r.status == kOk) expand_serial(s, src + s.src_offset, t, rows + s.packet_first, samples + s.packet_first, &r);
    results[i] = r;
    tables[i] = t;
}

// the sum over the workgroup; `part` has a word a wave
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* part)
{
    for (int o = 32; o; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
    __syncthreads();                                                  // (part's last readers are done)
    if (threadIdx.x % 64u == 0) part[threadIdx.x / 64u] = v;
    __syncthreads();
    uint64_t sum = 0;
    for (uint32_t w = 0; w < kMp4Waves; w++) sum += part[w];
    return sum;
}

__global__ __launch_bounds__(kMp4Threads) void mp4_sums_kernel(const Stream* __restrict__ streams, const Tables* __restrict__ tables, const Mp4Tile* __restrict__ tiles,
                                                               const uint8_t* __restrict__ src, uint64_t* __restrict__ tile_carry)
{
    __shared__ uint64_t part[kMp4Waves];
    const Mp4Tile tile = tiles[blockIdx.x];
    const Tables t = tables[tile.stream];
    const uint8_t* const base = src + streams[tile.stream].src_offset;
    uint64_t mine = 0;
    for (uint32_t k = 0; k < kMp4PerThread; k++) {
        const uint32_t s = tile.s0 + k * kMp4Threads + threadIdx.x;
        if (s < t.rows) mine += size_at(base, t, s);
    }
    const uint64_t sum = block_sum(mine, part);
    if (threadIdx.x == 0) tile_carry[blockIdx.x] = sum;
}

// out[i] = the sum of value(j), j < i, for i < n: a wave, 64 entries a turn
template <typename Value>
__device__ __forceinline__ void wave_exclusive_scan(uint32_t n, uint32_t lane, uint64_t* out, Value value)
{
    uint64_t carry = 0;
    for (uint32_t at = 0; at < n; at += 64u) {
        const uint32_t i = at + lane;
        const uint64_t v = i < n ? value(i) : 0u;
        uint64_t incl = v;
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, o);
            if (lane >= o) incl += up;
        }
        if (i < n) out[i] = carry + incl - v;
        carry += (uint64_t)__shfl((unsigned long long)incl, 63);
    }
}

__global__ __launch_bounds__(64) void mp4_carries_kernel(const Stream* __restrict__ streams, const Tables* __restrict__ tables, const Mp4Plan* __restrict__ plan,
                                                         const uint8_t* __restrict__ src, uint64_t* __restrict__ tile_carry, uint64_t* __restrict__ stsc_carry,
                                                         uint64_t* __restrict__ stts_carry, uint32_t n_stts)
{
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const Tables t = tables[i];
    if (!t.rows) return;
    const Mp4Plan pl = plan[i];
    const uint8_t* const base = src + streams[i].src_offset;
    uint64_t* const tiles = tile_carry + pl.tile_first;
    const uint32_t used_tiles = (t.rows + kTile - 1u) / kTile;       // (<= pl.n_tiles: rows <= packet_capacity)
    // the tile's own sum is read by its lane before any lane of the turn writes (the scan's shuffles lie between)
    wave_exclusive_scan(used_tiles, lane, tiles, [&](uint32_t k) { return tiles[k]; });
    wave_exclusive_scan(t.stsc_used, lane, stsc_carry + pl.stsc_first, [&](uint32_t k) { return stsc_run_samples(base, t, k); });
    wave_exclusive_scan(t.stts_used, lane, stts_carry + pl.stts_first, [&](uint32_t m) { return (uint64_t)stts_count(base, t, m); });
    wave_exclusive_scan(t.stts_used, lane, stts_carry + n_stts + pl.stts_first, [&](uint32_t m) { return (uint64_t)stts_count(base, t, m) * stts_delta(base, t, m); });
}

__global__ __launch_bounds__(kMp4Threads) void mp4_expand_kernel(const Stream* __restrict__ streams, const Tables* __restrict__ tables, const Mp4Plan* __restrict__ plan,
                                                                 const Mp4Tile* __restrict__ tiles, const uint8_t* __restrict__ src, const uint64_t* __restrict__ tile_carry,
                                                                 const uint64_t* __restrict__ stsc_carry, const uint64_t* __restrict__ stts_carry, uint32_t n_stts,
                                                                 Row* __restrict__ rows, Sample* __restrict__ samples, Result* __restrict__ results)
{
    __shared__ uint64_t prefix[kTile];                                // the sizes in front of each of the tile's samples, from the tile's start
    __shared__ uint64_t part[kMp4Waves];
    __shared__ uint32_t head_sample, refused, first_bad;
    const Mp4Tile tile = tiles[blockIdx.x];
    const Tables t = tables[tile.stream];
    if (tile.s0 >= t.rows) return;
    const Stream st = streams[tile.stream];
    const Mp4Plan pl = plan[tile.stream];
    const uint8_t* const base = src + st.src_offset;
    const uint64_t* const my_stsc = stsc_carry + pl.stsc_first;
    const uint64_t* const my_stts = stts_carry + pl.stts_first;
    const uint32_t s0 = tile.s0, tid = threadIdx.x;

    // the in-tile scan: a thread takes kMp4PerThread neighbours, the threads' totals are scanned a wave at a time
    uint32_t size[kMp4PerThread];
    uint64_t mine = 0;
    for (uint32_t k = 0; k < kMp4PerThread; k++) {
        const uint32_t s = s0 + tid * kMp4PerThread + k;
        size[k] = s < t.rows ? size_at(base, t, s) : 0u;
        mine += size[k];
    }
    uint64_t incl = mine;
    const uint32_t lane = tid % 64u, wave = tid / 64u;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63u) part[wave] = incl;
    if (tid == 0) {
        refused = 0; first_bad = kNone;
        // the chunk the tile's first sample lies in began at head_sample: in this tile, or in an earlier one
        const uint32_t k = last_at_most(my_stsc, t.stsc_used, s0);
        head_sample = s0 - (uint32_t)((s0 - my_stsc[k]) % stsc_spc(base, t, k));
    }
    __syncthreads();
    uint64_t before = incl - mine;
    for (uint32_t w = 0; w < wave; w++) before += part[w];
    for (uint32_t k = 0; k < kMp4PerThread; k++) {
        prefix[tid * kMp4PerThread + k] = before;
        before += size[k];
    }
    const uint32_t head = head_sample;
    // the global prefix at the head: its tile's carry and that tile's sizes in front of it
    uint64_t head_prefix = 0;
    if (head < s0) {                                                  // (uniform over the workgroup)
        const uint32_t head_tile = head / kTile;
        uint64_t some = 0;
        for (uint32_t s = head_tile * kTile + tid; s < head; s += kMp4Threads) some += size_at(base, t, s);
        head_prefix = tile_carry[pl.tile_first + head_tile] + block_sum(some, part);
    }
    __syncthreads();
    const uint64_t my_carry = tile_carry[blockIdx.x];
    auto global_prefix = [&](uint32_t s) { return s >= s0 ? my_carry + prefix[s - s0] : head_prefix; };   // (below s0 only the head is asked for)
    for (uint32_t k = 0; k < kMp4PerThread; k++) {
        const uint32_t s = s0 + k * kMp4Threads + tid;
        if (s >= t.rows) break;
        Row row;
        Sample sample;
        if (row_for(st, base, t, s, my_stsc, my_stts, my_stts + n_stts, global_prefix, &row, &sample)) {
            atomicAdd(&refused, 1u);
            atomicMin(&first_bad, s);
        }
        static_assert(sizeof(Row) == sizeof(uint4) && sizeof(Sample) == sizeof(uint4), "a row is one 16-byte store");
        uint4 a, b;
        __builtin_memcpy(&a, &row, 16);
        __builtin_memcpy(&b, &sample, 16);
        *reinterpret_cast<uint4*>(&rows[st.packet_first + s]) = a;
        *reinterpret_cast<uint4*>(&samples[st.packet_first + s]) = b;
    }
    __syncthreads();
    if (tid == 0 && refused) {
        atomicAdd(&results[tile.stream].samples_refused, refused);
        atomicMin(&results[tile.stream].first_bad_sample, first_bad);
    }
}

__global__ __launch_bounds__(64) void mp4_finish_kernel(const Tables* __restrict__ tables, uint32_t n, Result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t rows = tables[i].rows, bad = results[i].first_bad_sample;
    results[i].samples_available = bad < rows ? bad : rows;
}

int mp4_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Stream* streams)
{
    Mp4State& g = *b->mp4;
    OHGPU_TRY(state_events(g, 5));
    if (!g.n_streams) return OHGPU_OK;
    std::vector<Mp4Tile> tiles;
    std::vector<Mp4Plan> plan(g.n_streams);
    uint64_t stsc = 0, stts = 0;
    for (size_t i = 0; i < g.n_streams; i++) {
        const Stream& s = streams[i];
        // a row lies in one of the first `rows` entries of either table (S_k >= k), and a table has no more entries than its bytes allow
        const uint32_t stsc_cap = s.packet_capacity < s.src_bytes / 12u ? s.packet_capacity : s.src_bytes / 12u;
        const uint32_t stts_cap = s.packet_capacity < s.src_bytes / 8u ? s.packet_capacity : s.src_bytes / 8u;
        plan[i] = Mp4Plan{(uint32_t)tiles.size(), 0u, (uint32_t)stsc, (uint32_t)stts};
        if (!g.plain)
            for (uint64_t s0 = 0; s0 < s.packet_capacity; s0 += kTile) tiles.push_back(Mp4Tile{(uint32_t)i, (uint32_t)s0});
        plan[i].n_tiles = (uint32_t)tiles.size() - plan[i].tile_first;
        stsc += stsc_cap; stts += stts_cap;
    }
    if (stsc > 0x7fffffffull || stts > 0x7fffffffull || tiles.size() > 0x7fffffffull)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4_batch_create: %zu rows are more than one batch takes", g.n_packets);
    g.n_tiles = (uint32_t)tiles.size(); g.n_stsc = (uint32_t)stsc; g.n_stts = (uint32_t)stts;
    OHGPU_TRY(dev_array(ctx, g, &g.d_streams, g.n_streams, streams));
    OHGPU_TRY(dev_array<Result>(ctx, g, &g.d_results, g.n_streams));
    OHGPU_TRY(dev_array<Tables>(ctx, g, &g.d_tables, g.n_streams));
    OHGPU_TRY(dev_array(ctx, g, &g.d_plan, g.n_streams, plan.data()));
    OHGPU_TRY(dev_array(ctx, g, &g.d_tiles, g.n_tiles, tiles.data()));
    OHGPU_TRY(dev_array<uint64_t>(ctx, g, &g.d_tile_carry, g.n_tiles));
    OHGPU_TRY(dev_array<uint64_t>(ctx, g, &g.d_stsc_carry, g.n_tiles ? g.n_stsc + 1u : 0u));               // (the carries are the tiles': a
    OHGPU_TRY(dev_array<uint64_t>(ctx, g, &g.d_stts_carry, g.n_tiles ? 2u * (size_t)g.n_stts + 1u : 0u));   //  batch without tiles has none)
    OHGPU_TRY(dev_array<Row>(ctx, g, &g.d_packets, g.n_packets));
    OHGPU_TRY(dev_array<Sample>(ctx, g, &g.d_samples, g.n_packets));
    if (g.n_packets) OHGPU_HIP_TRY_ALLOC(hipMemset(g.d_packets, 0xa5, g.n_packets * sizeof(Row)));
    if (g.n_packets) OHGPU_HIP_TRY_ALLOC(hipMemset(g.d_samples, 0xa5, g.n_packets * sizeof(Sample)));
    OHGPU_HIP_TRY_ALLOC(hipStreamSynchronize(nullptr));                // (the fills are queued: a run on another stream must not meet them)
    return OHGPU_OK;
}

int mp4_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, hipStream_t s)
{
    Mp4State& g = *b->mp4;
    OHGPU_TRY(run_begin(g, s));      // (the tables serve one run at a time)
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u;
    const Stream* const streams = (const Stream*)g.d_streams;
    Tables* const tables = (Tables*)g.d_tables;
    Result* const results = (Result*)g.d_results;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    if (g.plain) {
        hipLaunchKernelGGL(mp4_plain_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, results, tables, (Row*)g.d_packets, (Sample*)g.d_samples);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        for (int k = 1; k < 4; k++) OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[k], s));
        return run_end(g, s);
    }
    hipLaunchKernelGGL(mp4_walk_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, results, tables);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(mp4_sums_kernel, dim3(g.n_tiles), dim3(kMp4Threads), 0, s, streams, (const Tables*)tables, (const Mp4Tile*)g.d_tiles, src, (uint64_t*)g.d_tile_carry);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[2], s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(mp4_carries_kernel, dim3(ns), dim3(64), 0, s, streams, (const Tables*)tables, (const Mp4Plan*)g.d_plan, src, (uint64_t*)g.d_tile_carry,
                           (uint64_t*)g.d_stsc_carry, (uint64_t*)g.d_stts_carry, g.n_stts);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[3], s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(mp4_expand_kernel, dim3(g.n_tiles), dim3(kMp4Threads), 0, s, streams, (const Tables*)tables, (const Mp4Plan*)g.d_plan, (const Mp4Tile*)g.d_tiles, src,
                           (const uint64_t*)g.d_tile_carry, (const uint64_t*)g.d_stsc_carry, (const uint64_t*)g.d_stts_carry, g.n_stts, (Row*)g.d_packets,
                           (Sample*)g.d_samples, results);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    hipLaunchKernelGGL(mp4_finish_kernel, dim3(lane_blocks), dim3(64), 0, s, (const Tables*)tables, ns, results);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    return run_end(g, s);
}

}  // namespace ohgpu
