// frag_units_driver.cpp -- csrc/frag_units.h on the CPU, for tests/test_frag_units_cpu.py (built with -fsanitize=address,undefined; its
// own main, nothing preloaded).  One batch of four streams whose rows, tiles and slots hold every kind of emptiness; every unit is listed
// by brute force, and the waves of a launch -- for_each_slot() from each wave's first slot, then locate() a lane -- must meet each unit
// exactly once, at the right stream, row and place in the row.  The slot plan is held against the two families' expressions, restated.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ohpipeline_amd/csrc/cenc_core.h"
#include "../../ohpipeline_amd/csrc/frag_units.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

namespace {

using fragu::kLanes;
using fragu::kTile;
constexpr uint32_t kStreams = 4, kWaves = 4, kGroupsPerCu = 8;

// the units of every row: stream 0 has no rows; stream 1 one row of one unit; stream 2 two tiles and three rows -- tile 0 with runs
// of empty rows at its start, in its middle and at its end and rows of 1, 63, 64 and 65 units between them (a row straddles a chunk's
// edge), tile 1 with no unit at all, tile 2 of three rows; stream 3 has no room for a row.
std::vector<std::vector<uint32_t>> make_rows()
{
    std::vector<std::vector<uint32_t>> n(kStreams);
    n[1] = {1};
    n[2].assign(2 * kTile + 3, 0);
    const uint32_t sizes[4] = {1, 63, 64, 65};
    for (uint32_t r = 10; r < kTile - 24; r++)
        if (r < 500 || r >= 521) n[2][r] = sizes[r % 4];
    n[2][2 * kTile + 1] = 65;
    return n;
}

struct Batch {
    std::vector<mp4frag::Stream> streams;
    std::vector<uint32_t> tile_first, sub_capacity;
    std::vector<uint64_t> chunk_first, tile_units, totals, row_first;     // row_first: the batch's table, a stream's rows from packet_first on
    std::vector<cenc::RowRec> rowrecs;                                    // the same prefixes in the first family's record
    fragu::SlotPlan plan;
};

Batch make_batch(const std::vector<std::vector<uint32_t>>& n, int num_cus)
{
    Batch b;
    b.streams.assign(kStreams, mp4frag::Stream{});
    b.sub_capacity = {0, 0, 0, 0};
    uint32_t row = 0;
    for (uint32_t i = 0; i < kStreams; i++) {
        uint64_t units = 0;
        for (uint32_t v : n[i]) units += v;
        b.totals.push_back(units);
        b.streams[i].packet_first = row;
        b.streams[i].packet_capacity = (uint32_t)n[i].size();
        b.streams[i].dst_capacity = i == 1 ? 16u * kLanes * 40u : i == 3 ? 4096u : (uint32_t)(16u * units);      // stream 1: 40 slots for one unit
        row += (uint32_t)n[i].size();
    }
    b.tile_first.assign(kStreams + 1, 0xa5a5a5a5u);
    b.chunk_first.assign(kStreams + 1, 0xa5a5a5a5a5a5a5a5ull);
    b.plan = fragu::slot_plan(b.streams.data(), kStreams, false, [&](size_t i) { return fragu::unit_bound(b.streams[i], b.sub_capacity[i]); }, num_cus, kWaves,
                              kGroupsPerCu, b.tile_first.data(), b.chunk_first.data());
    b.tile_units.assign(b.tile_first[kStreams], 0);
    b.row_first.assign(row, 0);
    b.rowrecs.assign(row, cenc::RowRec{});
    for (uint32_t i = 0; i < kStreams; i++) {
        uint64_t in_stream = 0, in_tile = 0;
        for (uint32_t r = 0; r < n[i].size(); r++) {
            if (r % kTile == 0) { b.tile_units[b.tile_first[i] + r / kTile] = in_stream; in_tile = 0; }
            b.row_first[b.streams[i].packet_first + r] = in_tile;
            b.rowrecs[b.streams[i].packet_first + r].block_first = in_tile;
            in_tile += n[i][r]; in_stream += n[i][r];
        }
    }
    return b;
}

void check_plan(const std::vector<std::vector<uint32_t>>& n)
{
    for (int num_cus : {0, 256})
        for (int family = 0; family < 2; family++)
            for (int plain = 0; plain < 2; plain++) {
                Batch b = make_batch(n, num_cus);
                if (family) b.sub_capacity = {0, 5, 700, 9};
                const fragu::SlotPlan p = fragu::slot_plan(b.streams.data(), kStreams, plain != 0, [&](size_t i) { return fragu::unit_bound(b.streams[i], b.sub_capacity[i]); },
                                                           num_cus, kWaves, kGroupsPerCu, b.tile_first.data(), b.chunk_first.data());
                uint32_t tiles = 0;
                uint64_t chunks = 0;
                for (uint32_t i = 0; i < kStreams; i++) {
                    const mp4frag::Stream& s = b.streams[i];
                    CHECK(b.tile_first[i] == tiles && b.chunk_first[i] == chunks);
                    // the first family's blocks, the second's units, as their plans stated them
                    const uint64_t blocks = s.packet_capacity && s.dst_capacity ? s.dst_capacity / 16u + s.packet_capacity : 0u;
                    const uint64_t units = s.packet_capacity && s.dst_capacity ? s.dst_capacity / 16u + s.packet_capacity + 3ull * b.sub_capacity[i] : 0u;
                    tiles += plain ? 0u : (uint32_t)(((uint64_t)s.packet_capacity + 1024u - 1u) / 1024u);
                    chunks += plain ? 0u : ((family ? units : blocks) + 64u - 1u) / 64u;
                }
                CHECK(b.tile_first[kStreams] == tiles && b.chunk_first[kStreams] == chunks && p.n_chunks == chunks);
                const uint64_t want = (chunks + 4u - 1u) / 4u, cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * 8u;
                CHECK(p.groups == (uint32_t)(want < cap ? want : cap));
                CHECK(plain ? chunks == 0 && tiles == 0 : tiles == 4 && b.chunk_first[1] == 0 && b.chunk_first[2] == 41 && b.chunk_first[3] == b.chunk_first[4]);
            }
}

// every wave of a launch of `stride` waves; rec: through the first family's record instead of the plain array
void check_trips(const std::vector<std::vector<uint32_t>>& n, const Batch& b, uint64_t stride, bool rec)
{
    struct At { uint32_t row, j; };
    std::vector<std::vector<At>> want(kStreams);
    std::vector<std::vector<uint32_t>> met(kStreams);
    for (uint32_t i = 0; i < kStreams; i++) {
        for (uint32_t r = 0; r < n[i].size(); r++)
            for (uint32_t j = 0; j < n[i][r]; j++) want[i].push_back({r, j});
        CHECK(want[i].size() == b.totals[i]);
        met[i].assign(want[i].size(), 0);
    }
    uint64_t chunks_met = 0;
    for (uint64_t wave = 0; wave < stride; wave++)
        fragu::for_each_slot(wave, stride, b.plan.n_chunks, b.chunk_first.data(), kStreams, b.totals.data(), [&](uint32_t i, uint64_t first, uint64_t total) {
            CHECK(i < kStreams && total == b.totals[i] && first < total && first % kLanes == 0);
            chunks_met++;
            const uint32_t row0 = b.streams[i].packet_first, rows = (uint32_t)n[i].size();
            for (uint32_t lane = 0; lane < kLanes && first + lane < total; lane++) {
                const uint64_t u = first + lane;
                const fragu::Place p = rec ? fragu::locate(u, b.tile_first[i], b.tile_units.data(), rows, [&](uint32_t r) { CHECK(r < rows); return b.rowrecs[row0 + r].block_first; })
                                           : fragu::locate(u, b.tile_first[i], b.tile_units.data(), rows, [&](uint32_t r) { CHECK(r < rows); return b.row_first[row0 + r]; });
                CHECK(p.row == want[i][u].row && p.j == want[i][u].j);
                met[i][u]++;
            }
        });
    uint64_t chunks_full = 0;
    for (uint32_t i = 0; i < kStreams; i++) {
        for (uint32_t v : met[i]) CHECK(v == 1);
        chunks_full += (b.totals[i] + kLanes - 1u) / kLanes;
    }
    CHECK(chunks_met == chunks_full);
}

void check_search()
{
    const uint64_t v[6] = {0, 0, 3, 3, 3, 9};
    CHECK(fragu::last_le(v, 0, 5) == 0 && fragu::last_le(v, 1, 5) == 0);      // (nothing is read of an empty table)
    CHECK(fragu::last_le(v, 6, 0) == 1 && fragu::last_le(v, 6, 2) == 1 && fragu::last_le(v, 6, 3) == 4 && fragu::last_le(v, 6, 8) == 4 && fragu::last_le(v, 6, 9) == 5);
    CHECK(fragu::last_le(2u, 5u, 100, [&](uint32_t k) { CHECK(k > 2 && k < 5); return v[k]; }) == 4);
}

}  // namespace

int main()
{
    const std::vector<std::vector<uint32_t>> n = make_rows();
    CHECK(n[2][0] == 0 && n[2][9] == 0 && n[2][500] == 0 && n[2][520] == 0 && n[2][kTile - 1] == 0 && n[2][12] == 1 && n[2][13] == 63 && n[2][14] == 64 && n[2][15] == 65);
    check_search();
    check_plan(n);
    const Batch b = make_batch(n, 0);
    CHECK(b.totals[0] == 0 && b.totals[1] == 1 && b.totals[3] == 0 && b.chunk_first[2] - b.chunk_first[1] == 41 && b.tile_units[b.tile_first[2] + 1] == b.tile_units[b.tile_first[2] + 2]);
    for (uint64_t stride : {(uint64_t)1, (uint64_t)4, b.plan.n_chunks + 3u})
        for (int rec = 0; rec < 2; rec++) check_trips(n, b, stride, rec != 0);
    printf("frag_units: %llu units in %llu slots, every unit met once\n", (unsigned long long)(b.totals[1] + b.totals[2]), (unsigned long long)b.plan.n_chunks);
    return 0;
}
