// cenc_core_driver.cpp -- runs csrc/cenc_core.h (over csrc/mp4_frag_core.h) on the CPU the way csrc/cenc_kernel.hip runs it on the device,
// for tests/test_cenc_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all; a program of its own, no preload).
//   cenc_core_driver JOB OUT
// JOB:  u64 n_streams, n_packets, n_runs, src_bytes, dst_bytes; the descriptors (cenc::Stream); the source arena.
// OUT:  twice -- the phases' route, then the plain route -- the results (cenc::Result per stream), the run table (mp4frag::Run, n_runs
//       rows), the packet table (mp4box::Row: places in the destination arena) and the sample table (mp4box::Sample, n_packets rows each),
//       the destination arena; the tables and the arena 0xA5 where nothing was written.
// The phases' route in the device's order: every stream walked under cenc::Protection; the run totals, the carries, the expansion a tile
// at a time and finish() as tests/cpp/mp4f_core_driver.cpp has them (the expansion serially here: its tiling is that driver's to hold);
// then the decrypt-gather as the three launches do it -- per tile the public rows, the IV places and the exclusive prefix of the
// keystream blocks; per stream the tiles' prefixes; per keystream block of the stream the two searches and cenc::crypt_lane.  The plain
// route: the serial text.  Every stream's bytes are copied into a heap block of exactly src_bytes (with -DOHGPU_ALIGNED_READS: rounded
// up to a whole word, read as the device reads), every stream's room in the destination is a heap block of exactly dst_capacity, the
// run records one of exactly run_capacity and the row tables of exactly packet_capacity, so that a stray index or a store outside a
// sample's range is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static unsigned long long g_steps[4];
#define MP4B_STEP(kind) (g_steps[kind]++)
#include "../../ohpipeline_amd/csrc/cenc_core.h"

using namespace mp4frag;

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T>
static T* block(size_t n, int fill)
{
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    memset((void*)p, fill, n ? n * sizeof(T) : 1);
    return p;
}

static constexpr cenc::Forward kForward = cenc::make_forward();
static const raopcore::Tables kTables = raopcore::make_tables();

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint64_t head[5];
    if (!read_all(f, head, 5)) return 1;
    const size_t ns = head[0], n_packets = head[1], n_runs = head[2], dst_bytes = head[4];
    std::vector<cenc::Stream> streams(ns);
    std::vector<uint8_t> arena(head[3]);
    if (!read_all(f, streams.data(), ns) || !read_all(f, arena.data(), arena.size())) { fprintf(stderr, "short job file\n"); return 1; }
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }

    for (int plain = 0; plain < 2; plain++) {
        std::vector<cenc::Result> results(ns);
        std::vector<Run> runs(n_runs);
        std::vector<Row> rows(n_packets);
        std::vector<Sample> samples(n_packets);
        std::vector<uint8_t> dst(dst_bytes, 0xa5);
        memset((void*)runs.data(), 0xa5, n_runs * sizeof(Run));
        memset((void*)rows.data(), 0xa5, n_packets * sizeof(Row));
        memset((void*)samples.data(), 0xa5, n_packets * sizeof(Sample));
        for (size_t i = 0; i < ns; i++) {
            const cenc::Stream& cs = streams[i];
            const Stream& s = cs.s;
#if defined(OHGPU_ALIGNED_READS)
            uint8_t* const bytes = block<uint8_t>((s.src_bytes + 3u) & ~(size_t)3u, 0);
#else
            uint8_t* const bytes = block<uint8_t>(s.src_bytes, 0);
#endif
            if (s.src_bytes) memcpy(bytes, arena.data() + s.src_offset, s.src_bytes);
            // the core takes arena bases: the stream's own blocks stand where the arenas would
            const uint8_t* const src0 = bytes - s.src_offset;
            uint8_t* const room = block<uint8_t>(s.dst_capacity, 0xa5);
            uint8_t* const dst0 = room - s.dst_offset;
            RunRec* recs = block<RunRec>(s.run_capacity, 0xa5);
            Row* src_rows = block<Row>(s.packet_capacity, 0xa5);
            Row* my_rows = block<Row>(s.packet_capacity, 0xa5);
            Sample* my_samples = block<Sample>(s.packet_capacity, 0xa5);
            Run* my_runs = block<Run>(s.run_capacity, 0xa5);
            uint32_t w[cenc::kScheduleWords] = {};
            if (cs.key_flags & cenc::kHaveKey) raopcore::expand_encrypt_key(cs.key, w, kTables);
            Rec rec;
            Result& r = results[i].r;
            cenc::Extra& x = results[i].x;
            memset(g_steps, 0, sizeof(g_steps));
            cenc::walk(cs, bytes, false, &r, &x, &rec, recs);
            if (g_steps[0] > kMaxBoxes + 1ull + 2ull * (mp4box::kMaxBoxes + 1ull)) { fprintf(stderr, "stream %zu: the walk read %llu box headers\n", i, g_steps[0]); return 1; }
            if (g_steps[1] > s.src_bytes / 4u + 1u) { fprintf(stderr, "stream %zu: the walk's entry loops took %llu steps\n", i, g_steps[1]); return 1; }
            if (rec.runs_written > s.run_capacity) { fprintf(stderr, "stream %zu: more runs written than there is room for\n", i); return 1; }
            for (uint32_t k = 0; k < rec.runs_written; k++)
                if (needs_sums(recs[k])) totals_serial(bytes, recs[k], recs[k].samples, &recs[k].bytes, &recs[k].frames);
            carries(s, &rec, recs, my_runs, &r);
            if (rec.rows > s.packet_capacity) { fprintf(stderr, "stream %zu: more rows than there is room for\n", i); return 1; }
            expand_serial(s, bytes, rec, recs, src_rows, my_samples, &r);
            // (expand_serial wrote places as if the stream lay at src_offset of an arena: so they are, from src0)
            finish(s, &rec, recs, src_rows, &r);
            if (r.bytes_gathered > s.dst_capacity) { fprintf(stderr, "stream %zu: more gathered than there is room for\n", i); return 1; }
            if (plain) {
                cenc::gather_serial(cs, src0, dst0, rec, recs, src_rows, r, w, kForward.te0, my_rows, &x);
            } else {
                const uint32_t n_tiles = (rec.rows + kTile - 1u) / kTile;
                cenc::RowRec* rowrecs = block<cenc::RowRec>(s.packet_capacity, 0xa5);
                uint64_t* tile_blocks = block<uint64_t>(n_tiles, 0xa5);
                const bool prot = x.is_protected != 0u;
                for (uint32_t t = 0; t < n_tiles; t++) {                      // the rows launch
                    uint64_t before = 0;
                    for (uint32_t row = t * kTile; row < (t + 1u) * kTile && row < rec.rows; row++) {
                        Row out;
                        out.src_offset = s.dst_offset; out.bytes = 0; out.reserved = 0;
                        cenc::RowRec rr;
                        rr.block_first = before; rr.iv_pos = 0; rr.pad = 0;
                        if (cenc::gathered_row(s, r, row)) {
                            const uint32_t k = run_of(recs, rec.runs_written, row);
                            out.src_offset = cenc::row_place(s, rec, recs, k, src_rows[row]); out.bytes = src_rows[row].bytes;
                            before += cenc::blocks_of(src_rows[row].bytes);
                            if (prot) rr.iv_pos = recs[k].iv_pos + (row - recs[k].first_sample) * x.iv_size;
                        }
                        my_rows[row] = out; rowrecs[row] = rr;
                    }
                    tile_blocks[t] = before;
                }
                uint64_t total = 0;                                           // the tiles launch
                for (uint32_t t = 0; t < n_tiles; t++) { const uint64_t v = tile_blocks[t]; tile_blocks[t] = total; total += v; }
                x.blocks = prot ? total : 0u;
                if (total > s.dst_capacity / 16u + s.packet_capacity) { fprintf(stderr, "stream %zu: more keystream blocks than the launch has slots for\n", i); return 1; }
                for (uint64_t b = 0; b < total; b++) {                        // the crypt launch: a lane a block
                    uint32_t ta = 0, tb = n_tiles;
                    while (tb - ta > 1u) { const uint32_t mid = ta + (tb - ta) / 2u; if (tile_blocks[mid] <= b) ta = mid; else tb = mid; }
                    const uint64_t in_tile = b - tile_blocks[ta];
                    const uint32_t s0 = ta * kTile, s1 = s0 + kTile < rec.rows ? s0 + kTile : rec.rows;
                    uint32_t ra = s0, rb = s1;
                    while (rb - ra > 1u) { const uint32_t mid = ra + (rb - ra) / 2u; if (rowrecs[mid].block_first <= in_tile) ra = mid; else rb = mid; }
                    const uint32_t j = (uint32_t)(in_tile - rowrecs[ra].block_first);
                    if ((uint64_t)j * 16u >= src_rows[ra].bytes) { fprintf(stderr, "stream %zu: block %llu found row %u, which does not hold it\n", i, (unsigned long long)b, ra); return 1; }
                    cenc::Iv iv = {};
                    if (prot) iv = cenc::read_iv(bytes, rowrecs[ra].iv_pos, x.iv_size);
                    cenc::crypt_lane(src0 + src_rows[ra].src_offset, dst0 + my_rows[ra].src_offset, src_rows[ra].bytes, j, prot ? w : nullptr, iv, kForward.te0);
                }
                free(rowrecs); free(tile_blocks);
            }
            // home: the stream's ranges of the tables and of the arena
            if (rec.rows) memcpy((void*)(rows.data() + s.packet_first), my_rows, rec.rows * sizeof(Row));
            if (rec.rows) memcpy((void*)(samples.data() + s.packet_first), my_samples, rec.rows * sizeof(Sample));
            if (rec.runs_written) memcpy((void*)(runs.data() + s.run_first), my_runs, rec.runs_written * sizeof(Run));
            if (s.dst_capacity) memcpy(dst.data() + s.dst_offset, room, s.dst_capacity);
            free(bytes); free(room); free(recs); free(src_rows); free(my_rows); free(my_samples); free(my_runs);
        }
        fwrite(results.data(), sizeof(cenc::Result), ns, f);
        fwrite(runs.data(), sizeof(Run), n_runs, f);
        fwrite(rows.data(), sizeof(Row), n_packets, f);
        fwrite(samples.data(), sizeof(Sample), n_packets, f);
        fwrite(dst.data(), 1, dst_bytes, f);
    }
    fclose(f);
    return 0;
}
