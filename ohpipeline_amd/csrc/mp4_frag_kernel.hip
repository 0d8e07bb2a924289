// mp4_frag_kernel.hip -- fragmented MPEG-4 on the device (the format's text is csrc/mp4_frag_core.h).
//   walk      a lane per stream: the boxes, the result's head, the stream's record and a record a run (where its entries lie, its
//             defaults, what the boxes say of its place and time; the totals of a run whose entries carry neither field).
//   run sums  a wave per run slot, persistent over the run table: the lanes stride the run's entries, the wave reduces -- the run's
//             bytes and frames in 64 bits.  An entry lies at any address: it is read as the aligned dwords that hold it.
//   carries   a lane per stream, serial over its runs: the samples, frames and gathered bytes in front of each run, the place of a run
//             that follows its predecessor; the public run rows.
//   expand    a workgroup per tile of kTile samples of one stream (the tile list is made at create, from packet_capacity): every
//             sample finds its run, the sizes and durations are scanned in the tile, and a sample's place in its run is the difference
//             of two prefixes -- or, in the run the tile's first sample lies in, the prefix plus that run's entries in front of the
//             tile, summed once a workgroup.  One 16-byte store a lane into each table; the refusals are counted and the lowest kept by
//             atomics on the result.
//   finish    a lane per stream: samples_available, the runs the gather begins and ends in, bytes_gathered.
//   gather    a wave per run slot, persistent: the run's piece through ohmrx::gather_lane.
//   plain     (kernel variant 1) one launch, a lane per stream: all of it in the serial text the CPU driver runs.
// The two persistent launches step over the run table by the grid's waves; a slot says on the device whether it holds a run.  No
// workgroup waits for another inside a launch: the order of the phases is the launch boundary.
// Every load lies inside the aligned dwords that hold a stream's range, which ohgpu_mp4f_batch_check placed inside the source arena:
// the walk accepts a trun only when its entries lie inside its box, a box only inside its parent, and a sample is gathered only when
// emit() found it inside the stream.  Every store lies inside the stream's rows [packet_first, + min(samples, packet_capacity)), its
// run slots [run_first, + min(runs, run_capacity)), its own records, or [dst_offset, + bytes_gathered <= dst_capacity).
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

using namespace mp4frag;

constexpr uint32_t kMp4fThreads = 256, kMp4fWaves = kMp4fThreads / 64, kMp4fPerThread = kTile / kMp4fThreads;
constexpr uint32_t kMp4fGroupsPerCu = 8;
static_assert(kTile % kMp4fThreads == 0, "a tile is a whole number of samples a thread");

__global__ __launch_bounds__(64) void mp4f_walk_kernel(const Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, Result* __restrict__ results,
                                                       Rec* __restrict__ recs, RunRec* __restrict__ runrecs)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    walk(s, src + s.src_offset, false, &results[i], &recs[i], runrecs + s.run_first);
}

// the run in slot j of the run table, if the last walk left one there
__device__ __forceinline__ bool slot_run(const Stream* streams, const Rec* recs, const uint32_t* slot_stream, uint32_t j, uint32_t* stream, uint32_t* k)
{
    const uint32_t i = slot_stream[j];
    if (i == kNone) return false;
    *stream = i;
    *k = j - streams[i].run_first;
    return *k < recs[i].runs_written;
}

__global__ __launch_bounds__(kMp4fThreads) void mp4f_sums_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs, const uint32_t* __restrict__ slot_stream,
                                                                 uint32_t n_slots, const uint8_t* __restrict__ src, RunRec* __restrict__ runrecs)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
    const uint32_t stride = gridDim.x * kMp4fWaves;
    for (uint32_t j = blockIdx.x * kMp4fWaves + wave; j < n_slots; j += stride) {
        uint32_t i, k;
        if (!slot_run(streams, recs, slot_stream, j, &i, &k)) continue;
        const RunRec r = runrecs[j];
        if (!needs_sums(r)) continue;
        const uint8_t* const base = src + streams[i].src_offset;
        uint64_t bytes = 0, frames = 0;
        for (uint32_t e = lane; e < r.samples; e += 64u) { bytes += entry_size(base, r, e); frames += entry_dur(base, r, e); }
        for (int o = 32; o; o >>= 1) {
            bytes += (uint64_t)__shfl_xor((unsigned long long)bytes, o);
            frames += (uint64_t)__shfl_xor((unsigned long long)frames, o);
        }
        if (lane == 0) { runrecs[j].bytes = bytes; runrecs[j].frames = frames; }
    }
}

__global__ __launch_bounds__(64) void mp4f_carries_kernel(const Stream* __restrict__ streams, uint32_t n, Rec* __restrict__ recs, RunRec* __restrict__ runrecs,
                                                          Run* __restrict__ runs, Result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    carries(s, &recs[i], runrecs + s.run_first, runs + s.run_first, &results[i]);
}

// the sums of both values over the workgroup; `part` has two words a wave
__device__ __forceinline__ void block_sum2(uint64_t* a, uint64_t* b, uint64_t* part)
{
    uint64_t x = *a, y = *b;
    for (int o = 32; o; o >>= 1) {
        x += (uint64_t)__shfl_xor((unsigned long long)x, o);
        y += (uint64_t)__shfl_xor((unsigned long long)y, o);
    }
    __syncthreads();                                                  // (part's last readers are done)
    if (threadIdx.x % 64u == 0) { part[2u * (threadIdx.x / 64u)] = x; part[2u * (threadIdx.x / 64u) + 1u] = y; }
    __syncthreads();
    x = y = 0;
    for (uint32_t w = 0; w < kMp4fWaves; w++) { x += part[2u * w]; y += part[2u * w + 1u]; }
    *a = x; *b = y;
}

__global__ __launch_bounds__(kMp4fThreads) void mp4f_expand_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs, const RunRec* __restrict__ runrecs,
                                                                   const Mp4fTile* __restrict__ tiles, const uint8_t* __restrict__ src, Row* __restrict__ rows,
                                                                   Sample* __restrict__ samples, Result* __restrict__ results)
{
    __shared__ uint64_t psize[kTile + 1], pdur[kTile + 1];            // the sizes / durations of the tile's samples in front of each, and of all of them
    __shared__ uint64_t part[2 * kMp4fWaves];
    __shared__ uint32_t refused, first_bad;
    const Mp4fTile tile = tiles[blockIdx.x];
    const Rec rec = recs[tile.stream];
    if (tile.s0 >= rec.rows) return;                                  // (uniform over the workgroup)
    const Stream st = streams[tile.stream];
    const uint8_t* const base = src + st.src_offset;
    const RunRec* const runs = runrecs + st.run_first;
    const uint32_t s0 = tile.s0, tid = threadIdx.x, lane = tid % 64u, wave = tid / 64u;

    // the in-tile scan: a thread takes kMp4fPerThread neighbours, the threads' totals are scanned a wave at a time
    uint32_t size[kMp4fPerThread], dur[kMp4fPerThread];
    uint64_t mine_s = 0, mine_d = 0;
    {
        const uint32_t first = s0 + tid * kMp4fPerThread;
        uint32_t k_run = first < rec.rows ? run_of(runs, rec.runs_written, first) : 0u;
        for (uint32_t k = 0; k < kMp4fPerThread; k++) {
            const uint32_t s = first + k;
            size[k] = dur[k] = 0;
            if (s < rec.rows) {
                while (s >= runs[k_run].first_sample + runs[k_run].samples) k_run++;      // (a run has a sample at the least, and s lies in a written run)
                const RunRec& r = runs[k_run];
                size[k] = entry_size(base, r, s - r.first_sample);
                dur[k] = entry_dur(base, r, s - r.first_sample);
            }
            mine_s += size[k]; mine_d += dur[k];
        }
    }
    uint64_t incl_s = mine_s, incl_d = mine_d;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint64_t up_s = (uint64_t)__shfl_up((unsigned long long)incl_s, o), up_d = (uint64_t)__shfl_up((unsigned long long)incl_d, o);
        if (lane >= o) { incl_s += up_s; incl_d += up_d; }
    }
    if (lane == 63u) { part[2u * wave] = incl_s; part[2u * wave + 1u] = incl_d; }
    if (tid == 0) { refused = 0; first_bad = kNone; }
    __syncthreads();
    uint64_t before_s = incl_s - mine_s, before_d = incl_d - mine_d;
    for (uint32_t w = 0; w < wave; w++) { before_s += part[2u * w]; before_d += part[2u * w + 1u]; }
    for (uint32_t k = 0; k < kMp4fPerThread; k++) {
        psize[tid * kMp4fPerThread + k] = before_s; pdur[tid * kMp4fPerThread + k] = before_d;
        before_s += size[k]; before_d += dur[k];
    }
    if (tid == kMp4fThreads - 1u) { psize[kTile] = before_s; pdur[kTile] = before_d; }
    // the run the tile's first sample lies in may have begun in front of the tile: its entries up to the tile, summed once
    const uint32_t head_run = run_of(runs, rec.runs_written, s0);
    const uint32_t head_first = runs[head_run].first_sample;
    uint64_t head_s = 0, head_d = 0;
    if (head_first < s0) {                                            // (uniform over the workgroup)
        const RunRec& r = runs[head_run];
        for (uint32_t e = tid; e < s0 - head_first; e += kMp4fThreads) { head_s += entry_size(base, r, e); head_d += entry_dur(base, r, e); }
        block_sum2(&head_s, &head_d, part);
    }
    __syncthreads();
    for (uint32_t k = 0; k < kMp4fPerThread; k++) {
        const uint32_t s = s0 + k * kMp4fThreads + tid;
        if (s >= rec.rows) break;
        const uint32_t at = s - s0, k_run = run_of(runs, rec.runs_written, s);
        const RunRec& r = runs[k_run];
        uint64_t in_s = psize[at], in_d = pdur[at];
        if (r.first_sample >= s0) { in_s -= psize[r.first_sample - s0]; in_d -= pdur[r.first_sample - s0]; }
        else { in_s += head_s; in_d += head_d; }
        Row row;
        Sample sample;
        if (emit(st, rec, r, k_run, in_s, in_d, (uint32_t)(psize[at + 1u] - psize[at]), (uint32_t)(pdur[at + 1u] - pdur[at]), &row, &sample)) {
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

__global__ __launch_bounds__(64) void mp4f_finish_kernel(const Stream* __restrict__ streams, uint32_t n, Rec* __restrict__ recs, const RunRec* __restrict__ runrecs,
                                                         const Row* __restrict__ rows, Result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    finish(s, &recs[i], runrecs + s.run_first, rows + s.packet_first, &results[i]);
}

__global__ __launch_bounds__(kMp4fThreads) void mp4f_gather_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs, const RunRec* __restrict__ runrecs,
                                                                   const uint32_t* __restrict__ slot_stream, uint32_t n_slots, const Row* __restrict__ rows,
                                                                   const Result* __restrict__ results, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
    const uint32_t stride = gridDim.x * kMp4fWaves;
    for (uint32_t j = blockIdx.x * kMp4fWaves + wave; j < n_slots; j += stride) {
        uint32_t i, k;
        if (!slot_run(streams, recs, slot_stream, j, &i, &k)) continue;
        const Stream& s = streams[i];
        uint64_t from, to;
        uint32_t bytes;
        if (!piece_of(s, recs[i], runrecs + s.run_first, rows + s.packet_first, results[i], k, &from, &to, &bytes)) continue;
        ohmrx::gather_lane(src + from, dst + to, bytes, lane, 64u);
    }
}

__global__ __launch_bounds__(64) void mp4f_plain_kernel(const Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        Result* __restrict__ results, Rec* __restrict__ recs, RunRec* __restrict__ runrecs, Run* __restrict__ runs,
                                                        Row* __restrict__ rows, Sample* __restrict__ samples)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    const uint8_t* const base = src + s.src_offset;
    RunRec* const my = runrecs + s.run_first;
    Result r;
    Rec rec;
    walk(s, base, false, &r, &rec, my);
    for (uint32_t k = 0; k < rec.runs_written; k++)
        if (needs_sums(my[k])) totals_serial(base, my[k], my[k].samples, &my[k].bytes, &my[k].frames);
    carries(s, &rec, my, runs + s.run_first, &r);
    expand_serial(s, base, rec, my, rows + s.packet_first, samples + s.packet_first, &r);
    finish(s, &rec, my, rows + s.packet_first, &r);
    for (uint32_t k = 0; k < rec.runs_written; k++) {
        uint64_t from, to;
        uint32_t bytes;
        if (piece_of(s, rec, my, rows + s.packet_first, r, k, &from, &to, &bytes)) ohmrx::gather_lane(src + from, dst + to, bytes, 0u, 1u);
    }
    results[i] = r;
    recs[i] = rec;
}

// The two persistent launches: a wave a run slot, at most kMp4fGroupsPerCu workgroups a CU (tests/test_gpu_mp4f_textbook.py restates it)
uint32_t mp4f_wave_blocks(uint64_t slots, uint32_t cus)
{
    const uint64_t want = (slots + kMp4fWaves - 1) / kMp4fWaves, cap = (uint64_t)cus * kMp4fGroupsPerCu;
    return (uint32_t)(want < cap ? want : cap);
}

int mp4f_plan(ohgpu_ctx* ctx, Mp4fState& g, const Stream* streams, const char* who)
{
    OHGPU_TRY(state_events(g, 7));
    if (!g.n_streams) return OHGPU_OK;
    std::vector<Mp4fTile> tiles;
    std::vector<uint32_t> slot_stream(g.n_runs, kNone);
    for (size_t i = 0; i < g.n_streams; i++) {
        const Stream& s = streams[i];
        if (!g.plain)
            for (uint64_t s0 = 0; s0 < s.packet_capacity; s0 += kTile) tiles.push_back(Mp4fTile{(uint32_t)i, (uint32_t)s0});
        for (uint32_t k = 0; k < s.run_capacity; k++) slot_stream[s.run_first + k] = (uint32_t)i;
    }
    if (tiles.size() > 0x7fffffffull) return set_error(OHGPU_ERR_INVALID, "%s: %zu rows are more than one batch takes", who, g.n_packets);
    g.n_tiles = (uint32_t)tiles.size();
    g.wave_blocks = mp4f_wave_blocks(g.n_runs, ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256u);
    OHGPU_TRY(dev_array(ctx, g, &g.d_streams, g.n_streams, streams));
    OHGPU_TRY(dev_array<Result>(ctx, g, &g.d_results, g.n_streams));
    OHGPU_TRY(dev_array<Rec>(ctx, g, &g.d_recs, g.n_streams));
    OHGPU_TRY(dev_array<RunRec>(ctx, g, &g.d_runrecs, g.n_runs));
    OHGPU_TRY(dev_array(ctx, g, &g.d_slot_stream, g.n_runs, slot_stream.data()));
    OHGPU_TRY(dev_array(ctx, g, &g.d_tiles, g.n_tiles, tiles.data()));
    OHGPU_TRY(dev_array<Run>(ctx, g, &g.d_runs, g.n_runs));
    OHGPU_TRY(dev_array<Row>(ctx, g, &g.d_packets, g.n_packets));
    OHGPU_TRY(dev_array<Sample>(ctx, g, &g.d_samples, g.n_packets));
    return OHGPU_OK;                                                  // (the tables are filled at the head of every run: mp4f_fill)
}

// The three public tables as a run finds them: 0xa5 in every row.  A run writes the rows its streams have and no others, so without this
// a row of the run before -- of a stream that now has fewer samples or runs -- would stand in the table as if it were this run's.
int mp4f_fill(const Mp4fState& g, hipStream_t s)
{
    if (g.n_runs) OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_runs, 0xa5, g.n_runs * sizeof(Run), s));
    if (g.n_packets) OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_packets, 0xa5, g.n_packets * sizeof(Row), s));
    if (g.n_packets) OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_samples, 0xa5, g.n_packets * sizeof(Sample), s));
    return OHGPU_OK;
}

// What stands between a walk and the gather, with the events of the phases: the family of csrc/cenc_kernel.hip runs it behind a walk of
// its own.
int mp4f_tables(const Mp4fState& g, const uint8_t* src, hipStream_t s)
{
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u, n_slots = (uint32_t)g.n_runs;
    const Stream* const streams = (const Stream*)g.d_streams;
    Result* const results = (Result*)g.d_results;
    Rec* const recs = (Rec*)g.d_recs;
    RunRec* const runrecs = (RunRec*)g.d_runrecs;
    const uint32_t* const slot_stream = (const uint32_t*)g.d_slot_stream;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
    if (g.wave_blocks) {
        hipLaunchKernelGGL(mp4f_sums_kernel, dim3(g.wave_blocks), dim3(kMp4fThreads), 0, s, streams, (const Rec*)recs, slot_stream, n_slots, src, runrecs);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[2], s));
    hipLaunchKernelGGL(mp4f_carries_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, recs, runrecs, (Run*)g.d_runs, results);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[3], s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(mp4f_expand_kernel, dim3(g.n_tiles), dim3(kMp4fThreads), 0, s, streams, (const Rec*)recs, (const RunRec*)runrecs, (const Mp4fTile*)g.d_tiles, src,
                           (Row*)g.d_packets, (Sample*)g.d_samples, results);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[4], s));
    hipLaunchKernelGGL(mp4f_finish_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, recs, (const RunRec*)runrecs, (const Row*)g.d_packets, results);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[5], s));
    return OHGPU_OK;
}

int mp4f_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    Mp4fState& g = *b->mp4f;
    OHGPU_TRY(run_begin(g, s));      // (the tables serve one run at a time)
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u, n_slots = (uint32_t)g.n_runs;
    const Stream* const streams = (const Stream*)g.d_streams;
    Result* const results = (Result*)g.d_results;
    Rec* const recs = (Rec*)g.d_recs;
    RunRec* const runrecs = (RunRec*)g.d_runrecs;
    const uint32_t* const slot_stream = (const uint32_t*)g.d_slot_stream;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    OHGPU_TRY(mp4f_fill(g, s));
    if (g.plain) {
        hipLaunchKernelGGL(mp4f_plain_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, dst, results, recs, runrecs, (Run*)g.d_runs, (Row*)g.d_packets, (Sample*)g.d_samples);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        for (int k = 1; k < 6; k++) OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[k], s));
        return run_end(g, s);
    }
    hipLaunchKernelGGL(mp4f_walk_kernel, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, results, recs, runrecs);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_TRY(mp4f_tables(g, src, s));
    if (g.gathers && g.wave_blocks) {
        hipLaunchKernelGGL(mp4f_gather_kernel, dim3(g.wave_blocks), dim3(kMp4fThreads), 0, s, streams, (const Rec*)recs, (const RunRec*)runrecs, slot_stream, n_slots,
                           (const Row*)g.d_packets, (const Result*)results, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(g, s);
}

}  // namespace ohgpu
