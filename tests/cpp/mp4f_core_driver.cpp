// mp4f_core_driver.cpp -- runs csrc/mp4_frag_core.h on the CPU the way csrc/mp4_frag_kernel.hip runs it on the device, for
// tests/test_mp4f_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   mp4f_core_driver JOB OUT
// JOB:  u64 n_streams, n_packets, n_runs, src_bytes, dst_bytes; the descriptors (mp4frag::Stream); the source arena.
// OUT:  twice -- the phases' route, then the plain route -- the results (mp4frag::Result per stream), the run table (mp4frag::Run, n_runs
//       rows), the packet table (mp4box::Row) and the sample table (mp4box::Sample, n_packets rows each), the destination arena; the
//       tables and the arena 0xA5 where nothing was written.
// The phases' route in the device's order: every stream walked; every run's totals, 64 lanes striding its entries; per stream the
// carries; every tile expanded -- the in-tile prefixes, the head run's entries in front of the tile, a row a sample through run_of(); per
// stream finish(); every run's piece through ohmrx::gather_lane, a lane at a time.  The plain route: the serial text.  Every stream's
// bytes are copied into a heap block of exactly src_bytes (built with -DOHGPU_ALIGNED_READS the core reads as the device does, in aligned
// words, and the block is rounded up to a whole word), its run records are a heap block of exactly run_capacity, the prefixes one of
// exactly kTile + 1, so that a stray index is the sanitizer's to report.  A step counter holds every loop to its bound: box headers by
// kMaxBoxes (and mp4box::kMaxBoxes inside a sample description), entry loops by the stream's bytes, sample loops by the rows, searches by
// 32 steps a sample.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static unsigned long long g_steps[4];
#define MP4B_STEP(kind) (g_steps[kind]++)
#include "../../ohpipeline_amd/csrc/mp4_frag_core.h"
#include "../../ohpipeline_amd/csrc/ohm_rx_core.h"

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
static void steps_reset() { memset(g_steps, 0, sizeof(g_steps)); }
static bool bound(const char* what, size_t i, unsigned long long got, unsigned long long most)
{
    if (got <= most) return true;
    fprintf(stderr, "stream %zu: %s took %llu steps where %llu bound it\n", i, what, got, most);
    return false;
}

struct Tables {
    std::vector<Result> results;
    Run* runs; Row* rows; Sample* samples; uint8_t* dst;
    size_t n_runs, n_packets, dst_bytes;
    Tables(size_t ns, size_t nr, size_t np, size_t nd) : results(ns), runs(block<Run>(nr, 0xa5)), rows(block<Row>(np, 0xa5)), samples(block<Sample>(np, 0xa5)),
                                                         dst(block<uint8_t>(nd, 0xa5)), n_runs(nr), n_packets(np), dst_bytes(nd) {}
    void write(FILE* f)
    {
        fwrite(results.data(), sizeof(Result), results.size(), f);
        fwrite(runs, sizeof(Run), n_runs, f);
        fwrite(rows, sizeof(Row), n_packets, f);
        fwrite(samples, sizeof(Sample), n_packets, f);
        fwrite(dst, 1, dst_bytes, f);
        free(runs); free(rows); free(samples); free(dst);
    }
};

// the piece's bytes lie in the stream's own block: *from is absolute in the arena
static bool gather_piece(const Stream& s, const uint8_t* bytes, Tables& t, const Rec& rec, const RunRec* recs, const Result& r, uint32_t k, uint32_t lanes)
{
    uint64_t from, to;
    uint32_t n;
    if (!piece_of(s, rec, recs, t.rows + s.packet_first, r, k, &from, &to, &n)) return true;
    if (from < s.src_offset || from - s.src_offset + n > s.src_bytes || to < s.dst_offset || to - s.dst_offset + n > s.dst_capacity || to + n > t.dst_bytes) {
        fprintf(stderr, "run %u: a piece outside its stream or its room\n", k);
        return false;
    }
    for (uint32_t lane = 0; lane < lanes; lane++) ohmrx::gather_lane(bytes + (from - s.src_offset), t.dst + to, n, lane, lanes);
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint64_t head[5];
    if (!read_all(f, head, 5)) return 1;
    const size_t ns = head[0], n_packets = head[1], n_runs = head[2], dst_bytes = head[4];
    std::vector<Stream> streams(ns);
    std::vector<uint8_t> arena(head[3]);
    if (!read_all(f, streams.data(), ns) || !read_all(f, arena.data(), arena.size())) { fprintf(stderr, "short job file\n"); return 1; }
    fclose(f);
    std::vector<uint8_t*> bytes(ns);
    for (size_t i = 0; i < ns; i++) {
#if defined(OHGPU_ALIGNED_READS)
        bytes[i] = block<uint8_t>((streams[i].src_bytes + 3u) & ~(size_t)3u, 0);     // (the device's reader: whole aligned words, see mp4_box_core.h)
#else
        bytes[i] = block<uint8_t>(streams[i].src_bytes, 0);
#endif
        if (streams[i].src_bytes) memcpy(bytes[i], arena.data() + streams[i].src_offset, streams[i].src_bytes);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }

    for (int plain = 0; plain < 2; plain++) {
        Tables t(ns, n_runs, n_packets, dst_bytes);
        for (size_t i = 0; i < ns; i++) {
            const Stream& s = streams[i];
            const uint8_t* p = bytes[i];
            RunRec* recs = block<RunRec>(s.run_capacity, 0xa5);
            Rec rec;
            Result& r = t.results[i];
            steps_reset();
            walk(s, p, false, &r, &rec, recs);
            if (!bound("the walk's box headers", i, g_steps[0], kMaxBoxes + 1ull + mp4box::kMaxBoxes + 1ull)) return 1;
            if (!bound("the walk's entry loops", i, g_steps[1], s.src_bytes / 4u + 1u)) return 1;
            if (g_steps[2] || g_steps[3]) { fprintf(stderr, "stream %zu: the walk touched samples\n", i); return 1; }
            if (rec.runs_written > s.run_capacity) { fprintf(stderr, "stream %zu: more runs written than there is room for\n", i); return 1; }
            steps_reset();
            Row* rows = t.rows + s.packet_first;
            Sample* samples = t.samples + s.packet_first;
            if (plain) {
                for (uint32_t k = 0; k < rec.runs_written; k++)
                    if (needs_sums(recs[k])) totals_serial(p, recs[k], recs[k].samples, &recs[k].bytes, &recs[k].frames);
                carries(s, &rec, recs, t.runs + s.run_first, &r);
                if (!bound("the totals and the carries", i, g_steps[1], s.src_bytes / 4u + rec.runs_written)) return 1;
                expand_serial(s, p, rec, recs, rows, samples, &r);
                finish(s, &rec, recs, rows, &r);
                for (uint32_t k = 0; k < rec.runs_written; k++)
                    if (!gather_piece(s, p, t, rec, recs, r, k, 1)) return 1;
                if (!bound("the serial expansion's samples", i, g_steps[2], rec.rows)) return 1;
            } else {
                // run sums: 64 lanes stride the entries
                for (uint32_t k = 0; k < rec.runs_written; k++) {
                    RunRec& rr = recs[k];
                    if (!needs_sums(rr)) continue;
                    uint64_t b = 0, d = 0;
                    for (uint32_t lane = 0; lane < 64u; lane++)
                        for (uint32_t e = lane; e < rr.samples; e += 64u) { b += entry_size(p, rr, e); d += entry_dur(p, rr, e); }
                    rr.bytes = b; rr.frames = d;
                }
                carries(s, &rec, recs, t.runs + s.run_first, &r);
                if (rec.rows > s.packet_capacity) { fprintf(stderr, "stream %zu: more rows than there is room for\n", i); return 1; }
                // expand: a tile at a time
                uint64_t* psize = block<uint64_t>(kTile + 1u, 0xa5);
                uint64_t* pdur = block<uint64_t>(kTile + 1u, 0xa5);
                uint32_t refused = 0, first_bad = kNone, tiles = 0;
                for (uint32_t s0 = 0; s0 < rec.rows; s0 += kTile, tiles++) {
                    uint64_t bs = 0, bd = 0;
                    uint32_t k_run = run_of(recs, rec.runs_written, s0);
                    for (uint32_t k = 0; k < kTile; k++) {
                        const uint32_t at = s0 + k;
                        psize[k] = bs; pdur[k] = bd;
                        if (at < rec.rows) {
                            while (at >= recs[k_run].first_sample + recs[k_run].samples) k_run++;
                            bs += entry_size(p, recs[k_run], at - recs[k_run].first_sample);
                            bd += entry_dur(p, recs[k_run], at - recs[k_run].first_sample);
                        }
                    }
                    psize[kTile] = bs; pdur[kTile] = bd;
                    const uint32_t head_run = run_of(recs, rec.runs_written, s0), head_first = recs[head_run].first_sample;
                    uint64_t head_s = 0, head_d = 0;
                    for (uint32_t e = 0; head_first < s0 && e < s0 - head_first; e++) { head_s += entry_size(p, recs[head_run], e); head_d += entry_dur(p, recs[head_run], e); }
                    for (uint32_t at = s0; at < s0 + kTile && at < rec.rows; at++) {
                        const uint32_t k = at - s0, kr = run_of(recs, rec.runs_written, at);
                        const RunRec& rr = recs[kr];
                        uint64_t in_s = psize[k], in_d = pdur[k];
                        if (rr.first_sample >= s0) { in_s -= psize[rr.first_sample - s0]; in_d -= pdur[rr.first_sample - s0]; }
                        else { in_s += head_s; in_d += head_d; }
                        if (emit(s, rec, rr, kr, in_s, in_d, (uint32_t)(psize[k + 1u] - psize[k]), (uint32_t)(pdur[k + 1u] - pdur[k]), &rows[at], &samples[at])) {
                            refused++;
                            if (at < first_bad) first_bad = at;
                        }
                    }
                }
                free(psize); free(pdur);
                r.samples_refused = refused; r.first_bad_sample = first_bad;
                if (!bound("the expansion's samples", i, g_steps[2], rec.rows)) return 1;
                if (!bound("the expansion's searches", i, g_steps[3], 32ull * rec.rows + 64ull * tiles)) return 1;
                steps_reset();
                finish(s, &rec, recs, rows, &r);
                if (!bound("finish's searches", i, g_steps[3], 64)) return 1;
                for (uint32_t k = 0; k < rec.runs_written; k++)
                    if (!gather_piece(s, p, t, rec, recs, r, k, 64)) return 1;
            }
            free(recs);
        }
        t.write(f);
    }
    fclose(f);
    for (uint8_t* b : bytes) free(b);
    return 0;
}
