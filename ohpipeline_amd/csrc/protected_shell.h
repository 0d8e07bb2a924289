// protected_shell.h -- what the decrypt-gathers of the two protected fragmented MPEG-4 families share on the device and around their
// launches (csrc/cenc_kernel.hip; csrc/cbcs_kernel.hip).  Where the first family counts keystream
// blocks and the second work units, this text says UNIT; the index arithmetic is csrc/frag_units.h's.
//   rows        public_row(): the public packet row of a sample, by the gather's own arithmetic; tile_exclusive_scan(): the exclusive
//               prefix of the units over a tile's rows (a shuffle scan a wave, the waves folded through the LDS) and the tile's sum.
//   tiles       tiles_body(): a lane per stream, serial over its tiles -- the sums become the units in front of each tile; the
//               stream's units; what the family reports as the stream's blocks.
//   crypt       unit_loop(): the persistent loop, a wave per chunk slot and a lane a unit; the family's functor serves the unit.
//   the host    protected_plan() lays out tiles and slots, protected_run() is a run but for the family's launches (the release, with
//               its wipe of the key schedules, is api_common.h's protected_free).
// The kernels themselves, the staging of the cipher's tables in the LDS and the cipher are the families' own.
#pragma once

#include <hip/hip_runtime.h>

#include "api_common.h"
#include "frag_units.h"

namespace ohgpu {

using namespace mp4frag;

constexpr uint32_t kProtThreads = 256, kProtWaves = kProtThreads / 64, kProtPerThread = kTile / kProtThreads, kProtGroupsPerCu = 8;
static_assert(kTile % kProtThreads == 0 && kProtThreads == 256, "a tile is a whole number of samples a thread; a thread stages one word of each table");
static_assert(cenc::kLaneBlocks == fragu::kLanes && cbcs::kLaneUnits == fragu::kLanes && fragu::kLanes == 64, "a chunk slot is a wave's: a lane a unit");

// Row s of the public packet table: nothing at dst_offset unless the row is gathered (then true, *from: the expansion's row, *k_run: its run)
__device__ __forceinline__ bool public_row(const Stream& st, const Rec& rec, const Result& res, const RunRec* runs, const Row* src_rows, Row* rows, uint32_t s, Row* from,
                                           uint32_t* k_run)
{
    Row out;
    out.src_offset = st.dst_offset; out.bytes = 0; out.reserved = 0;
    const bool gathered = cenc::gathered_row(st, res, s);
    if (gathered) {
        *k_run = run_of(runs, rec.runs_written, s);
        *from = src_rows[st.packet_first + s];
        out.src_offset = cenc::row_place(st, rec, runs, *k_run, *from); out.bytes = from->bytes;
    }
    uint4 v;
    __builtin_memcpy(&v, &out, 16);
    *reinterpret_cast<uint4*>(&rows[st.packet_first + s]) = v;
    return gathered;
}

// n[]: the units of this thread's PerThread consecutive rows.  *before: the units of the tile's rows in front of the thread's first;
// *tile_total: through its last -- in the workgroup's last thread, the tile's.  part[]: kProtWaves words of LDS; one barrier.
template <uint32_t PerThread>
__device__ __forceinline__ void tile_exclusive_scan(const uint32_t (&n)[PerThread], uint64_t* part, uint64_t* before, uint64_t* tile_total)
{
    const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
    uint64_t mine = 0;
    for (uint32_t k = 0; k < PerThread; k++) mine += n[k];
    uint64_t incl = mine;
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((unsigned long long)incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63u) part[wave] = incl;
    __syncthreads();
    uint64_t sum = incl - mine;
    for (uint32_t w = 0; w < wave; w++) sum += part[w];
    *before = sum;
    *tile_total = sum + mine;
}

// blocks(i, units): what the family reports as stream i's blocks
template <typename Blocks>
__device__ __forceinline__ void tiles_body(uint32_t n, const Rec* recs, const uint32_t* tile_first, uint64_t* tile_units, uint64_t* nunits, cenc::Extra* extras, Blocks blocks)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t t0 = tile_first[i], used = (recs[i].rows + kTile - 1u) / kTile;        // (rows <= packet_capacity: the stream has that many tiles)
    uint64_t acc = 0;
    for (uint32_t t = t0; t < t0 + used; t++) {
        const uint64_t v = tile_units[t];
        tile_units[t] = acc;
        acc += v;
    }
    nunits[i] = acc;
    extras[i].blocks = blocks(i, acc);
}

// row_first(r): the units of the tile's rows in front of row r of the batch's table; unit(i, st, r, j): serve unit j of row r of stream
// i (the same i for the whole wave)
template <typename RowFirst, typename Unit>
__device__ __forceinline__ void unit_loop(const Stream* streams, uint32_t n_streams, const Rec* recs, const uint32_t* tile_first, const uint64_t* tile_units,
                                          const uint64_t* chunk_first, uint64_t n_chunks, const uint64_t* nunits, RowFirst row_first, Unit unit)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
    fragu::for_each_slot((uint64_t)blockIdx.x * kProtWaves + wave, (uint64_t)gridDim.x * kProtWaves, n_chunks, chunk_first, n_streams, nunits,
        [=](uint32_t i, uint64_t first, uint64_t total) {
            const uint64_t u = first + lane;
            if (u >= total) return;
            const Stream& st = streams[i];
            const fragu::Place p = fragu::locate(u, tile_first[i], tile_units, recs[i].rows, [=, &st](uint32_t r) { return row_first(st.packet_first + r); });
            unit(i, st, st.packet_first + p.row, p.j);
        });
}

// ---- around the launches
// The family's state with its counts, keys and kind of route set: mp4f_plan over the plain descriptors, the tiles and the chunk slots
// (sub_capacity(i): the stream's subsample rows, 0 for a family without), the device copy of the descriptors as given -- the caller
// has taken the keys out --, and every array of CencState (RowFirst: what the family keeps a row in d_row_first).  Nothing more for a batch of no streams.
template <typename RowFirst, typename CStream, typename SubCapacity>
int protected_plan(ohgpu_ctx* ctx, CencState& g, const std::vector<Stream>& plain, const std::vector<CStream>& stripped, const char* who, SubCapacity sub_capacity)
{
    const size_t n = g.n_streams;
    OHGPU_TRY(mp4f_plan(ctx, g, plain.data(), who));
    if (!n) return OHGPU_OK;
    g.tile_first.assign(n + 1, 0);
    std::vector<uint64_t> chunk_first(n + 1, 0);
    const fragu::SlotPlan p = fragu::slot_plan(plain.data(), n, g.plain, [&](size_t i) { return fragu::unit_bound(plain[i], sub_capacity(i)); }, ctx->num_cus, kProtWaves,
                                               kProtGroupsPerCu, g.tile_first.data(), chunk_first.data());
    g.n_chunks = p.n_chunks;
    g.crypt_blocks = p.groups;
    g.keys_bytes = g.keys.size() * sizeof(uint32_t);
    OHGPU_TRY(dev_array(ctx, g, &g.d_cstreams, n, stripped.data()));
    OHGPU_TRY(dev_array(ctx, g, &g.d_keys, g.keys.size(), g.keys.data()));
    OHGPU_TRY(dev_array<cenc::Extra>(ctx, g, &g.d_extras, n));
    OHGPU_TRY(dev_array<Row>(ctx, g, &g.d_rows, g.n_packets));
    OHGPU_TRY(dev_array<RowFirst>(ctx, g, &g.d_row_first, g.n_packets));
    OHGPU_TRY(dev_array(ctx, g, &g.d_tile_first, n + 1, g.tile_first.data()));
    OHGPU_TRY(dev_array<uint64_t>(ctx, g, &g.d_tile_units, g.n_tiles));
    OHGPU_TRY(dev_array(ctx, g, &g.d_chunk_first, n + 1, chunk_first.data()));
    OHGPU_TRY(dev_array<uint64_t>(ctx, g, &g.d_nunits, n));
    return OHGPU_OK;
}

// A run but for the launches: plain() is the one launch of kernel variant 1, walk() the family's walk, gather() -> int its
// decrypt-gather behind mp4f_tables.
template <typename Plain, typename Walk, typename Gather>
int protected_run(CencState& g, const uint8_t* src, hipStream_t s, Plain plain, Walk walk, Gather gather)
{
    OHGPU_TRY(run_begin(g, s));      // (the tables serve one run at a time)
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    OHGPU_TRY(mp4f_fill(g, s));                                       // (no row of the run before stands in a table: csrc/mp4_frag_kernel.hip)
    if (g.n_packets) OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_rows, 0xa5, g.n_packets * sizeof(Row), s));
    if (g.plain) {
        plain();
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        for (int k = 1; k < 6; k++) OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[k], s));
        return run_end(g, s);
    }
    walk();
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_TRY(mp4f_tables(g, src, s));
    OHGPU_TRY(gather());
    return run_end(g, s);
}

}  // namespace ohgpu
