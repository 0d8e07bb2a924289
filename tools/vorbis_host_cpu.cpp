// vorbis_host_cpu.cpp -- the Vorbis core's serial text (csrc/vorbis_core.h) on host threads: the host leg of tools/bench_vorbis.py.
//   vorbis_host_cpu <case> <streams> <threads> <reps>
// <case>: u32 bytes + identification packet, u32 bytes + setup packet, u32 n, then n times u32 bytes + packet (tests/test_vorbis_core_cpu.py's
// form).  Every one of <streams> copies of the stream is decoded whole by one thread -- the setup image is parsed once, as a batch's
// caller does; then per packet head, floors, residue, coupling, curve, the direct-form DCT-IV, window, overlap-add and rounding to 16-bit
// big-endian frames -- <threads> threads taking streams in turn.  Prints "<samples a channel of one stream> <checksum> <ms>": the best
// of <reps> repetitions.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <vector>

#include "../ohpipeline_amd/csrc/vorbis_core.h"

using namespace vorbiscore;

struct Case {
    std::vector<uint32_t> img;
    ParsedInfo info;
    std::vector<std::vector<uint8_t>> packets;
    std::map<uint32_t, std::vector<float>> slopes, cos8;
    float db[256];
};

static uint64_t decode_stream(const Case& c, std::vector<uint8_t>& out)
{
    const uint32_t n = (uint32_t)c.packets.size(), ch = c.info.channels;
    const uint32_t* img = c.img.data();
    std::vector<Rec> recs(n);
    for (uint32_t i = 0; i < n; i++) head_packet(img, c.packets[i].data(), (uint32_t)c.packets[i].size(), &recs[i]);
    Stream s;
    memset(&s, 0, sizeof(s));
    s.n_packets = n; s.max_samples = ~0ull; s.channels = ch; s.bs0 = c.info.bs0; s.bs1 = c.info.bs1;
    scan_stream(s, recs.data());
    const Image& im = image_head(img);
    std::vector<uint8_t> cls(im.class_bytes ? im.class_bytes : 1);
    std::vector<std::vector<float>> blocks(n);
    std::vector<float> rows, u;
    std::vector<FloorOut> floors(ch);
    uint64_t samples = 0;
    for (uint32_t i = 0; i < n; i++) {
        const Rec& r = recs[i];
        if (r.status != kOk) continue;
        const uint32_t bs = r.blocksize, half = bs / 2u;
        rows.assign((size_t)ch * half, 0.0f);
        decode_packet(img, c.packets[i].data(), (uint32_t)c.packets[i].size(), r, Rows{rows.data(), half}, floors.data(), cls.data());
        const Mode& mode = image_mode(img, r.mode);
        const Mapping& map = image_mapping(img, mode.mapping);
        blocks[i].assign((size_t)ch * bs, 0.0f);
        u.resize(half);
        for (uint32_t k = 0; k < ch; k++) {
            if (!floors[k].used) continue;
            float* row = rows.data() + (size_t)k * half;
            Segment segs[64];
            int32_t tx, ty;
            const uint32_t ns = floor_segments(image_floor(img, map.sub_floor[map.mux[k]]), floors[k], segs, &tx, &ty);
            for (uint32_t g = 0; g < ns; g++) draw_segment(segs[g], (int32_t)half, [&](int32_t x, int32_t y) { row[x] = row[x] * c.db[y]; });
            for (uint32_t x = (uint32_t)tx; x < half; x++) row[x] = row[x] * c.db[ty];
            const float* cos8 = c.cos8.at(bs).data();
            for (uint32_t x = 0; x < half; x++) u[x] = dct4_direct(row, half, cos8, x);
            for (uint32_t x = 0; x < bs; x++)
                blocks[i][(size_t)k * bs + x] = unfold_at(u.data(), half, x) * window_at(x, bs, c.info.bs0, mode.blockflag != 0, r.prev_flag != 0, r.next_flag != 0,
                                                                                         c.slopes.at(bs).data(), c.slopes.at(c.info.bs0).data());
        }
        for (uint32_t j = 0; j < r.samples; j++)
            for (uint32_t k = 0; k < ch; k++) {
                const int32_t v = to_pcm16(overlap_at(blocks[r.prev_packet].data() + (size_t)k * r.prev_block, r.prev_block, blocks[i].data() + (size_t)k * bs, bs, j));
                out.push_back((uint8_t)((uint32_t)v >> 8)); out.push_back((uint8_t)v);
            }
        samples += r.samples;
        if (r.prev_block && r.prev_packet != i) std::vector<float>().swap(blocks[r.prev_packet]);
    }
    return samples;
}

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s case streams threads reps\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    auto blob = [&] { uint32_t n = 0; std::vector<uint8_t> v; if (fread(&n, 4, 1, f) == 1) { v.resize(n); if (n && fread(v.data(), 1, n, f) != n) v.clear(); } return v; };
    Case c;
    const std::vector<uint8_t> ident = blob(), setup = blob();
    const char* why = "";
    if (parse_setup(ident.data(), ident.size(), setup.data(), setup.size(), &c.img, &c.info, &why) != kParseOk) { fprintf(stderr, "parse_setup: %s\n", why); return 1; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t i = 0; i < n; i++) { c.packets.push_back(blob()); c.packets.back().reserve(1); }
    fclose(f);
    db_table(c.db);
    for (uint32_t bs : {c.info.bs0, c.info.bs1}) {
        c.slopes[bs].resize(bs / 2u);
        window_slope(bs, c.slopes[bs].data());
        c.cos8[bs].resize(4u * bs);
        for (uint32_t j = 0; j < 4u * bs; j++) c.cos8[bs][j] = (float)std::cos(2.0 * 3.14159265358979323846 * j / (4.0 * bs));
    }
    const int streams = atoi(argv[2]), threads = atoi(argv[3]), reps = atoi(argv[4]);
    double best = 1e30;
    uint64_t samples = 0, sum = 0;
    for (int rep = 0; rep < reps; rep++) {
        std::atomic<int> next(0);
        std::vector<uint64_t> sums(threads, 0), counts(threads, 0);
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++)
            pool.emplace_back([&, t] {
                std::vector<uint8_t> out;
                for (int k = next++; k < streams; k = next++) {
                    out.clear();
                    counts[t] = decode_stream(c, out);
                    uint64_t h = 1469598103934665603ull;
                    for (uint8_t b : out) h = (h ^ b) * 1099511628211ull;
                    sums[t] = h;
                }
            });
        for (auto& th : pool) th.join();
        best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        for (int t = 0; t < threads; t++) if (counts[t]) { samples = counts[t]; sum = sums[t]; }
    }
    printf("%llu %llu %.3f\n", (unsigned long long)samples, (unsigned long long)sum, best);
    return 0;
}
