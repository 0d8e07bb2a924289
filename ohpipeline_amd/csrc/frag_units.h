// frag_units.h -- the index arithmetic of the protected fragmented MPEG-4 families' decrypt-gather, once for
// both: csrc/cenc_kernel.hip counts keystream blocks, csrc/cbcs_kernel.hip work units, and here either is a UNIT.  Every function is
// __host__ __device__ and needs no HIP header: csrc/protected_shell.h runs this text in the persistent launch and in the two plans,
// tests/cpp/frag_units_driver.cpp runs the same text on the CPU under the sanitizers, against a brute-force list of every unit.
//
//   the rows     a stream's rows lie in tiles of kTile.  row_first(r) is the units of the tile's rows in front of row r, tile_units[t]
//                the units of the stream's tiles in front of tile t, totals[i] the units of stream i.  A row, a tile or a stream may
//                have no unit at all: the searches below take the LAST entry that is <= the key, which is never an empty one.
//   the slots    a chunk slot is kLanes consecutive units of one stream, a lane each.  Stream i owns the slots [chunk_first[i],
//                chunk_first[i + 1]), laid out at create from a bound on its units (unit_bound); what a run finds is at most that.
//   a wave       takes slot g, then g + stride, ...: for_each_slot() finds whose slot g is and where the wave goes next -- by the
//                stride from a slot that holds units, and from a slot behind its stream's last unit to the first g + k * stride at or
//                behind the next stream's first slot.  locate() then finds a unit's row and its place in the row.
#pragma once

#include "mp4_frag_core.h"

namespace fragu {

using mp4frag::kTile;
using mp4frag::Stream;

constexpr uint32_t kLanes = 64;           // the units of a chunk slot (cenc::kLaneBlocks, cbcs::kLaneUnits)

// a wave's lanes agree on the slot's stream: on the device the index is made uniform, so what it selects stays in scalar registers
#if defined(__HIP_DEVICE_COMPILE__)
#define FRAGU_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define FRAGU_UNIFORM(x) (x)
#endif

// The last k of [lo, hi) whose at(k) is <= key, where at() does not fall; lo where none is (at(lo) is not read) or hi <= lo + 1.
template <typename At>
MP4B_HD uint32_t last_le(uint32_t lo, uint32_t hi, uint64_t key, At at)
{
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (at(mid) <= key) lo = mid; else hi = mid;
    }
    return lo;
}
MP4B_HD uint32_t last_le(const uint64_t* first, uint32_t n, uint64_t key)
{
    return last_le(0u, n, key, [first](uint32_t k) { return first[k]; });
}

// ---- the chunk slots
// One wave's whole trip: from slot g on, by the stride, below n_chunks.  chunk(i, first, total) for every slot that holds units: the
// stream, the slot's first unit and the stream's units (its lanes take first + lane, where that is below total).
template <typename Chunk>
MP4B_HD void for_each_slot(uint64_t g, uint64_t stride, uint64_t n_chunks, const uint64_t* chunk_first, uint32_t n_streams, const uint64_t* totals, Chunk chunk)
{
    while (g < n_chunks) {
        const uint32_t i = FRAGU_UNIFORM(last_le(chunk_first, n_streams, g));      // the stream the slot lies in
        const uint64_t total = totals[i], first = (g - chunk_first[i]) * kLanes;
        if (first >= total) {                                         // behind the stream's last unit: on to the next stream's slots
            g += (chunk_first[i + 1u] - g + stride - 1u) / stride * stride;
            continue;
        }
        g += stride;
        chunk(i, first, total);
    }
}

// ---- a unit's row
struct Place { uint32_t row, j; };        // the stream's row and the unit's index inside it
// t0: the stream's first tile of tile_units[]; row_first(r): of the stream's row r
template <typename RowFirst>
MP4B_HD Place locate(uint64_t unit, uint32_t t0, const uint64_t* tile_units, uint32_t n_rows, RowFirst row_first)
{
    const uint32_t t = last_le(0u, (n_rows + kTile - 1u) / kTile, unit, [=](uint32_t k) { return tile_units[t0 + k]; });
    const uint64_t in_tile = unit - tile_units[t0 + t];
    const uint32_t s0 = t * kTile, s1 = s0 + kTile < n_rows ? s0 + kTile : n_rows;
    const uint32_t row = last_le(s0, s1, in_tile, row_first);
    return {row, (uint32_t)(in_tile - row_first(row))};
}

// ---- the plan.  A bound on a stream's units from its capacities: the sum of ceil(size / 16) over rows that fit the room is at most
// dst_capacity / 16 + packet_capacity; a part of a sample of B bytes is at most B / 16 + 1 units, + 2 under a keystream offset, so
// every subsample row a stream may fill adds 3 (sub_capacity: 0 where samples are served whole).
MP4B_HD uint64_t unit_bound(const Stream& s, uint32_t sub_capacity)
{
    return s.packet_capacity && s.dst_capacity ? s.dst_capacity / 16u + s.packet_capacity + 3ull * sub_capacity : 0u;
}
// tile_first and chunk_first take n + 1 entries each; bound(i) is stream i's unit_bound.  A plain batch (one launch, a lane per
// stream) has neither tiles nor slots.  groups: the persistent launch, `waves` slots a workgroup, at most groups_per_cu a CU.
struct SlotPlan { uint64_t n_chunks; uint32_t groups; };
template <typename Bound>
inline SlotPlan slot_plan(const Stream* streams, size_t n, bool plain, Bound bound, int num_cus, uint32_t waves, uint32_t groups_per_cu, uint32_t* tile_first,
                          uint64_t* chunk_first)
{
    tile_first[0] = 0; chunk_first[0] = 0;
    for (size_t i = 0; i < n; i++) {
        tile_first[i + 1] = tile_first[i] + (plain ? 0u : (uint32_t)(((uint64_t)streams[i].packet_capacity + kTile - 1u) / kTile));
        chunk_first[i + 1] = chunk_first[i] + (plain ? 0u : (bound(i) + kLanes - 1u) / kLanes);
    }
    SlotPlan p;
    p.n_chunks = chunk_first[n];
    const uint64_t want = (p.n_chunks + waves - 1u) / waves, cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * groups_per_cu;
    p.groups = (uint32_t)(want < cap ? want : cap);
    return p;
}

}  // namespace fragu
