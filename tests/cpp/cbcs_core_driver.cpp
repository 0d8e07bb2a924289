// cbcs_core_driver.cpp -- runs csrc/cbcs_core.h (over csrc/cenc_core.h and csrc/mp4_frag_core.h) on the CPU the way csrc/cbcs_kernel.hip
// runs it on the device, for tests/test_cbcs_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all; a program
// of its own, no preload).
//   cbcs_core_driver JOB OUT [CUS]
// JOB:  u64 n_streams, n_packets, n_runs, n_subsamples, src_bytes, dst_bytes; the descriptors (cbcs::Stream); the source arena.
// OUT:  twice -- the phases' route, then the plain route -- the results (cbcs::Result per stream), the run table, the packet table
//       (places in the destination arena) and the sample table, the destination arena; 0xA5 where nothing was written.
// The phases' route in the device's order: every stream walked under cbcs::Protection, which writes its subsample rows and sample
// records; the rows served put where packet_capacity stands; the run totals, the carries, the expansion and finish(); then the
// decrypt-gather as the three launches do it -- per tile the public rows and the exclusive prefix of the work units, per stream the
// tiles' prefixes, and per work unit of the stream the three searches (tile, row, entry) and cbcs::unit_lane.  With CUS given the units
// are taken in the order the persistent launch takes them: chunk slots of 64 laid out from the capacities, 32 CUS waves that stride over
// them and jump over the slots behind a stream's last unit; every unit must be met exactly once.  The plain route: the serial text.
// Every stream's bytes are copied into a heap block of exactly src_bytes (with -DOHGPU_ALIGNED_READS: rounded up to a whole word, read
// as the device reads), its room in the destination is a heap block of exactly dst_capacity, its run records, row tables and subsample
// rows blocks of exactly their capacities, so that a stray index or a store outside a sample's range is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ohpipeline_amd/csrc/cbcs_core.h"

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

struct Work {                 // what the phases' route keeps of a stream between its launches
    uint8_t* bytes; uint8_t* room;
    RunRec* recs; Row* src_rows; Row* my_rows; Sample* my_samples; Run* my_runs;
    cbcs::SubRow* subs; cbcs::SampleRec* samprecs;
    uint64_t* unit_first; uint64_t* tile_units;
    uint32_t keys[cbcs::kKeyWords];
    Rec rec; Stream s; uint64_t total; std::vector<uint8_t> met;
};

int main(int argc, char** argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s JOB OUT [CUS]\n", argv[0]); return 2; }
    const uint64_t cus = argc == 4 ? strtoull(argv[3], nullptr, 10) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint64_t head[6];
    if (!read_all(f, head, 6)) return 1;
    const size_t ns = head[0], n_packets = head[1], n_runs = head[2], dst_bytes = head[5];
    std::vector<cbcs::Stream> streams(ns);
    std::vector<uint8_t> arena(head[4]);
    if (!read_all(f, streams.data(), ns) || !read_all(f, arena.data(), arena.size())) { fprintf(stderr, "short job file\n"); return 1; }
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    cbcs::Tables t;
    t.te0 = kForward.te0; t.td0 = kTables.td0; t.isbox = kTables.isbox;

    for (int plain = 0; plain < 2; plain++) {
        std::vector<cbcs::Result> results(ns);
        std::vector<Run> runs(n_runs);
        std::vector<Row> rows(n_packets);
        std::vector<Sample> samples(n_packets);
        std::vector<uint8_t> dst(dst_bytes, 0xa5);
        memset((void*)runs.data(), 0xa5, n_runs * sizeof(Run));
        memset((void*)rows.data(), 0xa5, n_packets * sizeof(Row));
        memset((void*)samples.data(), 0xa5, n_packets * sizeof(Sample));
        std::vector<Work> work(ns);
        std::vector<uint64_t> chunk_first(ns + 1, 0);
        for (size_t i = 0; i < ns; i++) {
            const cbcs::Stream& cs = streams[i];
            Work& w = work[i];
            w.s = cs.c.s;
            Stream& s = w.s;
#if defined(OHGPU_ALIGNED_READS)
            w.bytes = block<uint8_t>((s.src_bytes + 3u) & ~(size_t)3u, 0);
#else
            w.bytes = block<uint8_t>(s.src_bytes, 0);
#endif
            if (s.src_bytes) memcpy(w.bytes, arena.data() + s.src_offset, s.src_bytes);
            w.room = block<uint8_t>(s.dst_capacity, 0xa5);
            w.recs = block<RunRec>(s.run_capacity, 0xa5);
            w.src_rows = block<Row>(s.packet_capacity, 0xa5);
            w.my_rows = block<Row>(s.packet_capacity, 0xa5);
            w.my_samples = block<Sample>(s.packet_capacity, 0xa5);
            w.my_runs = block<Run>(s.run_capacity, 0xa5);
            w.subs = block<cbcs::SubRow>(cs.sub_capacity, 0xa5);
            w.samprecs = block<cbcs::SampleRec>(s.packet_capacity, 0xa5);
            memset(w.keys, 0, sizeof(w.keys));
            if (cs.c.key_flags & cenc::kHaveKey) {
                raopcore::expand_encrypt_key(cs.c.key, w.keys, kTables);
                raopcore::expand_decrypt_key(cs.c.key, w.keys + raopcore::kRoundKeyWords, kTables);
            }
            const uint64_t units = s.packet_capacity && s.dst_capacity ? s.dst_capacity / 16u + s.packet_capacity + 3ull * cs.sub_capacity : 0u;
            chunk_first[i + 1] = chunk_first[i] + (units + cbcs::kLaneUnits - 1u) / cbcs::kLaneUnits;
            // the core takes arena bases: the stream's own blocks stand where the arenas would
            const uint8_t* const src0 = w.bytes - s.src_offset;
            uint8_t* const dst0 = w.room - s.dst_offset;
            Result& r = results[i].c.r;
            cenc::Extra& x = results[i].c.x;
            cbcs::More& m = results[i].m;
            uint32_t rows_cap;
            cbcs::walk(cs, w.bytes, false, w.subs, w.samprecs, &r, &x, &m, &w.rec, w.recs, &rows_cap);
            Rec& rec = w.rec;
            if (rec.runs_written > s.run_capacity || m.subsamples > cs.sub_capacity || rows_cap > s.packet_capacity) { fprintf(stderr, "stream %zu: more written than there is room for\n", i); return 1; }
            s.packet_capacity = rows_cap;
            for (uint32_t k = 0; k < rec.runs_written; k++)
                if (needs_sums(w.recs[k])) totals_serial(w.bytes, w.recs[k], w.recs[k].samples, &w.recs[k].bytes, &w.recs[k].frames);
            carries(s, &rec, w.recs, w.my_runs, &r);
            if (rec.rows > s.packet_capacity) { fprintf(stderr, "stream %zu: more rows than there is room for\n", i); return 1; }
            expand_serial(s, w.bytes, rec, w.recs, w.src_rows, w.my_samples, &r);
            finish(s, &rec, w.recs, w.src_rows, &r);
            if (r.bytes_gathered > s.dst_capacity) { fprintf(stderr, "stream %zu: more gathered than there is room for\n", i); return 1; }
            w.total = 0;
            if (plain) {
                cbcs::gather_serial(cs, src0, dst0, rec, w.recs, w.src_rows, r, w.keys, t, w.subs, w.samprecs, m, w.my_rows, &x);
                continue;
            }
            const uint32_t n_tiles = (rec.rows + kTile - 1u) / kTile, kind = cbcs::kind_of(x);
            w.unit_first = block<uint64_t>(cs.c.s.packet_capacity, 0xa5);
            w.tile_units = block<uint64_t>(n_tiles, 0xa5);
            uint64_t blocks = 0;
            for (uint32_t tile = 0; tile < n_tiles; tile++) {                 // the rows launch
                uint64_t before = 0;
                for (uint32_t row = tile * kTile; row < (tile + 1u) * kTile && row < rec.rows; row++) {
                    Row out;
                    out.src_offset = s.dst_offset; out.bytes = 0; out.reserved = 0;
                    w.unit_first[row] = before;
                    if (cenc::gathered_row(s, r, row)) {
                        const uint32_t k = run_of(w.recs, rec.runs_written, row);
                        out.src_offset = cenc::row_place(s, rec, w.recs, k, w.src_rows[row]); out.bytes = w.src_rows[row].bytes;
                        uint32_t units, mine;
                        cbcs::sample_work(kind, m, w.samprecs, row, out.bytes, &units, &mine);
                        before += units; blocks += mine;
                    }
                    w.my_rows[row] = out;
                }
                w.tile_units[tile] = before;
            }
            for (uint32_t tile = 0; tile < n_tiles; tile++) { const uint64_t v = w.tile_units[tile]; w.tile_units[tile] = w.total; w.total += v; }      // the tiles launch
            x.blocks = blocks;
            if (w.total > units) { fprintf(stderr, "stream %zu: %llu work units where the launch has slots for %llu\n", i, (unsigned long long)w.total, (unsigned long long)units); return 1; }
            w.met.assign(w.total, 0);
        }
        // the crypt launch: a lane a unit
        auto unit = [&](size_t i, uint64_t u) -> bool {
            Work& w = work[i];
            const cbcs::Stream& cs = streams[i];
            const cenc::Extra& x = results[i].c.x;
            const cbcs::More& m = results[i].m;
            const Rec& rec = w.rec;
            const uint32_t n_tiles = (rec.rows + kTile - 1u) / kTile, kind = cbcs::kind_of(x);
            uint32_t ta = 0, tb = n_tiles;
            while (tb - ta > 1u) { const uint32_t mid = ta + (tb - ta) / 2u; if (w.tile_units[mid] <= u) ta = mid; else tb = mid; }
            const uint64_t in_tile = u - w.tile_units[ta];
            const uint32_t s0 = ta * kTile, s1 = s0 + kTile < rec.rows ? s0 + kTile : rec.rows;
            uint32_t ra = s0, rb = s1;
            while (rb - ra > 1u) { const uint32_t mid = ra + (rb - ra) / 2u; if (w.unit_first[mid] <= in_tile) ra = mid; else rb = mid; }
            const uint32_t j = (uint32_t)(in_tile - w.unit_first[ra]), size = w.src_rows[ra].bytes;
            uint32_t units, mine;
            cbcs::sample_work(kind, m, w.samprecs, ra, size, &units, &mine);
            if (j >= units) { fprintf(stderr, "stream %zu: unit %llu found row %u, which does not hold it\n", i, (unsigned long long)u, ra); return false; }
            cbcs::SubRow e = cbcs::whole_sample(kind, size);
            uint32_t v = j;
            cbcs::SampleIv iv = {};
            if (kind != cbcs::kCopy) {
                const cbcs::SampleRec sr = w.samprecs[ra];
                iv = cbcs::read_sample_iv(w.bytes, sr.iv_pos, x.iv_size ? x.iv_size : m.civ_size);
                if (sr.n_sub) {
                    if ((uint64_t)sr.sub_first + sr.n_sub > cs.sub_capacity) { fprintf(stderr, "stream %zu: row %u has entries outside the stream's share\n", i, ra); return false; }
                    e = w.subs[sr.sub_first + cbcs::entry_of(w.subs + sr.sub_first, sr.n_sub, j)];
                    v = j - e.unit_first;
                }
            }
            if (v >= cbcs::pieces(e.clear) + cbcs::prot_units(kind, e.prot, e.ks)) { fprintf(stderr, "stream %zu: unit %llu found an entry that does not hold it\n", i, (unsigned long long)u); return false; }
            if (w.met[u]++) { fprintf(stderr, "stream %zu: unit %llu met twice\n", i, (unsigned long long)u); return false; }
            cbcs::unit_lane(w.bytes - w.s.src_offset + w.src_rows[ra].src_offset, w.room - w.s.dst_offset + w.my_rows[ra].src_offset, e, v, kind, m.crypt, m.skip, w.keys, iv, t);
            return true;
        };
        if (!plain && !cus) {
            for (size_t i = 0; i < ns; i++)
                for (uint64_t u = 0; u < work[i].total; u++) if (!unit(i, u)) return 1;
        } else if (!plain) {
            const uint64_t n_chunks = chunk_first[ns], want = (n_chunks + 3u) / 4u, groups = want < 8u * cus ? want : 8u * cus, stride = groups * 4u;
            for (uint64_t wave = 0; wave < stride; wave++)
                for (uint64_t g = wave; g < n_chunks;) {
                    size_t lo = 0, hi = ns;
                    while (hi - lo > 1u) { const size_t mid = lo + (hi - lo) / 2u; if (chunk_first[mid] <= g) lo = mid; else hi = mid; }
                    const uint64_t u0 = (g - chunk_first[lo]) * cbcs::kLaneUnits;
                    if (u0 >= work[lo].total) { g += (chunk_first[lo + 1u] - g + stride - 1u) / stride * stride; continue; }
                    g += stride;
                    for (uint64_t lane = 0; lane < cbcs::kLaneUnits && u0 + lane < work[lo].total; lane++) if (!unit(lo, u0 + lane)) return 1;
                }
        }
        for (size_t i = 0; i < ns; i++) {
            Work& w = work[i];
            const Stream& s = streams[i].c.s;
            if (!plain)
                for (uint64_t u = 0; u < w.total; u++) if (!w.met[u]) { fprintf(stderr, "stream %zu: unit %llu never met\n", i, (unsigned long long)u); return 1; }
            // home: the stream's ranges of the tables and of the arena
            if (w.rec.rows) memcpy((void*)(rows.data() + s.packet_first), w.my_rows, w.rec.rows * sizeof(Row));
            if (w.rec.rows) memcpy((void*)(samples.data() + s.packet_first), w.my_samples, w.rec.rows * sizeof(Sample));
            if (w.rec.runs_written) memcpy((void*)(runs.data() + s.run_first), w.my_runs, w.rec.runs_written * sizeof(Run));
            if (s.dst_capacity) memcpy(dst.data() + s.dst_offset, w.room, s.dst_capacity);
            free(w.bytes); free(w.room); free(w.recs); free(w.src_rows); free(w.my_rows); free(w.my_samples); free(w.my_runs); free(w.subs); free(w.samprecs);
            if (!plain) { free(w.unit_first); free(w.tile_units); }
        }
        fwrite(results.data(), sizeof(cbcs::Result), ns, f);
        fwrite(runs.data(), sizeof(Run), n_runs, f);
        fwrite(rows.data(), sizeof(Row), n_packets, f);
        fwrite(samples.data(), sizeof(Sample), n_packets, f);
        fwrite(dst.data(), 1, dst_bytes, f);
    }
    fclose(f);
    return 0;
}
