// mp4_core_driver.cpp -- runs csrc/mp4_box_core.h on the CPU the way csrc/mp4_table_kernel.hip runs it on the device, for
// tests/test_mp4_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   mp4_core_driver JOB OUT
// JOB:  u64 n_streams, n_packets, src_bytes; the descriptors (mp4box::Stream); the source arena.
// OUT:  twice -- the fused route, then the plain route -- the results (mp4box::Result per stream), the packet table (mp4box::Row,
//       n_packets rows), the sample table (mp4box::Sample, n_packets rows); both tables 0xA5 where nothing was written.
// The fused route in the device's order: every stream walked; every tile's sum; per stream the four carries; every tile expanded --
// its in-tile prefix, the head of the chunk its first sample lies in, a row a sample through the searches; the refusals counted.  The
// plain route: the walk and expand_serial.  Every stream's bytes are copied into a heap block of exactly src_bytes, the carries and
// the prefix are heap blocks exactly as large as the plan says (built with -DOHGPU_ALIGNED_READS the core reads as the device does, in
// aligned words, and a stream's block is rounded up to a whole word), so that a stray index is the sanitizer's to report.  A step counter
// holds every loop to the bound the format's text names: box headers by kMaxBoxes, entry loops by the entry counts, sample loops by N.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static unsigned long long g_steps[4];
#define MP4B_STEP(kind) (g_steps[kind]++)
#include "../../ohpipeline_amd/csrc/mp4_box_core.h"

using namespace mp4box;

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T>
static T* block(size_t n, int fill)
{
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    memset(p, fill, n ? n * sizeof(T) : 1);
    return p;
}
static void steps_reset() { memset(g_steps, 0, sizeof(g_steps)); }
static bool bound(const char* what, size_t i, unsigned long long got, unsigned long long most)
{
    if (got <= most) return true;
    fprintf(stderr, "stream %zu: %s took %llu steps where %llu bound it\n", i, what, got, most);
    return false;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint64_t head[3];
    if (!read_all(f, head, 3)) return 1;
    const size_t ns = head[0], n_packets = head[1];
    std::vector<Stream> streams(ns);
    std::vector<uint8_t> arena(head[2]);
    if (!read_all(f, streams.data(), ns) || !read_all(f, arena.data(), arena.size())) { fprintf(stderr, "short job file\n"); return 1; }
    fclose(f);
    // (the rows' src_offset is absolute: the stream's own block stands for [src_offset, + src_bytes) of the arena)
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

    // ---- the fused route
    {
        std::vector<Result> results(ns);
        std::vector<Tables> tables(ns);
        Row* rows = block<Row>(n_packets, 0xa5);
        Sample* samples = block<Sample>(n_packets, 0xa5);
        for (size_t i = 0; i < ns; i++) {
            steps_reset();
            walk(streams[i], bytes[i], &results[i], &tables[i]);
            if (!bound("the walk's box headers", i, g_steps[0], kMaxBoxes + 1ull)) return 1;
            if (!bound("the walk's entry loops", i, g_steps[1], streams[i].src_bytes / 12u + streams[i].src_bytes / 8u)) return 1;
            if (g_steps[2] || g_steps[3]) { fprintf(stderr, "stream %zu: the walk touched samples\n", i); return 1; }
        }
        for (size_t i = 0; i < ns; i++) {
            const Stream& s = streams[i];
            const Tables& t = tables[i];
            const uint8_t* p = bytes[i];
            const uint32_t n_tiles = (uint32_t)(((uint64_t)s.packet_capacity + kTile - 1u) / kTile);
            const uint32_t stsc_cap = s.packet_capacity < s.src_bytes / 12u ? s.packet_capacity : s.src_bytes / 12u;
            const uint32_t stts_cap = s.packet_capacity < s.src_bytes / 8u ? s.packet_capacity : s.src_bytes / 8u;
            if (t.rows > s.packet_capacity || t.stsc_used > stsc_cap || t.stts_used > stts_cap) { fprintf(stderr, "stream %zu: the plan is too small\n", i); return 1; }
            uint64_t* tile_carry = block<uint64_t>(n_tiles, 0xa5);
            uint64_t* stsc_carry = block<uint64_t>(stsc_cap, 0xa5);
            uint64_t* stts_carry = block<uint64_t>(stts_cap, 0xa5);
            uint64_t* stts_frames = block<uint64_t>(stts_cap, 0xa5);
            uint64_t* prefix = block<uint64_t>(kTile, 0xa5);
            steps_reset();
            // sums
            for (uint32_t tile = 0; tile < n_tiles; tile++) {
                uint64_t sum = 0;
                for (uint32_t s0 = tile * kTile, k = 0; k < kTile && s0 + k < t.rows; k++) sum += size_at(p, t, s0 + k);
                tile_carry[tile] = sum;
            }
            // carries
            const uint32_t used_tiles = (t.rows + kTile - 1u) / kTile;
            uint64_t run = 0;
            for (uint32_t k = 0; k < used_tiles; k++) { const uint64_t v = tile_carry[k]; tile_carry[k] = run; run += v; }
            run = 0;
            for (uint32_t k = 0; k < t.stsc_used; k++) { stsc_carry[k] = run; run += stsc_run_samples(p, t, k); }
            uint64_t run_frames = 0;
            run = 0;
            for (uint32_t m = 0; m < t.stts_used; m++) {
                stts_carry[m] = run; stts_frames[m] = run_frames;
                run += stts_count(p, t, m); run_frames += (uint64_t)stts_count(p, t, m) * stts_delta(p, t, m);
            }
            // expand
            uint32_t refused = 0, first_bad = kNone;
            for (uint32_t tile = 0; tile < used_tiles; tile++) {
                const uint32_t s0 = tile * kTile;
                uint64_t before = 0;
                for (uint32_t k = 0; k < kTile; k++) { prefix[k] = before; before += s0 + k < t.rows ? size_at(p, t, s0 + k) : 0u; }
                const uint32_t k0 = last_at_most(stsc_carry, t.stsc_used, s0);
                const uint32_t head_sample = s0 - (uint32_t)((s0 - stsc_carry[k0]) % stsc_spc(p, t, k0));
                uint64_t head_prefix = 0;
                if (head_sample < s0) {
                    const uint32_t head_tile = head_sample / kTile;
                    head_prefix = tile_carry[head_tile];
                    for (uint32_t s1 = head_tile * kTile; s1 < head_sample; s1++) head_prefix += size_at(p, t, s1);
                }
                const uint64_t my_carry = tile_carry[tile];
                bool strayed = false;
                auto global_prefix = [&](uint32_t at) {
                    if (at >= s0) return my_carry + prefix[at - s0];
                    if (at != head_sample) strayed = true;
                    return head_prefix;
                };
                for (uint32_t s1 = s0; s1 < s0 + kTile && s1 < t.rows; s1++)
                    if (row_for(s, p, t, s1, stsc_carry, stts_carry, stts_frames, global_prefix, &rows[s.packet_first + s1], &samples[s.packet_first + s1])) {
                        refused++;
                        if (s1 < first_bad) first_bad = s1;
                    }
                if (strayed) { fprintf(stderr, "stream %zu tile %u: a prefix in front of the tile that is not its head\n", i, tile); return 1; }
            }
            if (!bound("the expansion's samples", i, g_steps[2], t.rows)) return 1;
            if (!bound("the expansion's searches", i, g_steps[3], 64ull * t.rows + 32ull * used_tiles)) return 1;
            results[i].samples_refused = refused;
            results[i].first_bad_sample = first_bad;
            results[i].samples_available = first_bad < t.rows ? first_bad : t.rows;
            free(tile_carry); free(stsc_carry); free(stts_carry); free(stts_frames); free(prefix);
        }
        fwrite(results.data(), sizeof(Result), ns, f);
        fwrite(rows, sizeof(Row), n_packets, f);
        fwrite(samples, sizeof(Sample), n_packets, f);
        free(rows); free(samples);
    }
    // ---- the plain route
    {
        std::vector<Result> results(ns);
        Row* rows = block<Row>(n_packets, 0xa5);
        Sample* samples = block<Sample>(n_packets, 0xa5);
        for (size_t i = 0; i < ns; i++) {
            Tables t;
            walk(streams[i], bytes[i], &results[i], &t);
            steps_reset();
            if (results[i].status == kOk) expand_serial(streams[i], bytes[i], t, rows + streams[i].packet_first, samples + streams[i].packet_first, &results[i]);
            if (!bound("the serial expansion's samples", i, g_steps[2], t.rows)) return 1;
            if (!bound("the serial expansion's entry steps", i, g_steps[1], (unsigned long long)t.stsc_entries + t.stts_entries)) return 1;
        }
        fwrite(results.data(), sizeof(Result), ns, f);
        fwrite(rows, sizeof(Row), n_packets, f);
        fwrite(samples, sizeof(Sample), n_packets, f);
        free(rows); free(samples);
    }
    fclose(f);
    for (uint8_t* b : bytes) free(b);
    return 0;
}
