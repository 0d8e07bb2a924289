// ogg_host_cpu.cpp -- the host leg of tools/bench_ogg.py: this project's own Ogg core (csrc/ogg_page_core.h) on the CPU, a stream a
// task on THREADS threads -- the walk with every page's checksum run serially through the byte table as it comes, then the pieces
// copied with memcpy.  Not the reference's page library: the same text the device runs, on the host.
//   ogg_host_cpu FILE STREAMS THREADS REPEATS     FILE holds one stream's bytes; every stream is a copy of it.  Prints the median
//   wall time of a pass over all streams in milliseconds, and the bytes one stream delivered.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../ohpipeline_amd/csrc/ogg_page_core.h"

using namespace oggpage;

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s FILE STREAMS THREADS REPEATS\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<uint8_t> one;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) one.insert(one.end(), buf, buf + n);
    fclose(f);
    const size_t n_streams = strtoul(argv[2], nullptr, 10), threads = strtoul(argv[3], nullptr, 10), repeats = strtoul(argv[4], nullptr, 10);
    std::vector<uint8_t> src(one.size() * n_streams), dst(one.size() * n_streams);
    for (size_t i = 0; i < n_streams; i++) memcpy(src.data() + i * one.size(), one.data(), one.size());
    Tables tables;
    make_tables(&tables);
    std::vector<Result> results(n_streams);
    std::vector<double> ms;
    for (size_t r = 0; r < repeats; r++) {
        std::atomic<size_t> next{0};
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (size_t t = 0; t < threads; t++)
            pool.emplace_back([&] {
                std::vector<Piece> pieces;
                for (size_t i; (i = next++) < n_streams;) {
                    Stream s = {};
                    s.src_offset = s.dst_offset = i * one.size();
                    s.src_bytes = (uint32_t)one.size();
                    s.dst_capacity = one.size();
                    s.flags = kAnySeq | kAnySerial | kFlacMapping;
                    pieces.resize(piece_capacity(s));
                    auto good = [&](uint32_t, const uint8_t* page, uint32_t bytes) { return crc_run(tables.byte, page, 0, bytes) == stored_crc(page); };
                    uint32_t n_pieces = 0;
                    walk(s, (uint32_t)i, src.data(), nullptr, pieces.data(), good, &results[i], &n_pieces);
                    for (uint32_t k = 0; k < n_pieces; k++)
                        memcpy(dst.data() + s.dst_offset + pieces[k].run_pos, src.data() + s.src_offset + pieces[k].src_pos, pieces[k].bytes);
                }
            });
        for (auto& t : pool) t.join();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("%llu %.3f\n", (unsigned long long)results[0].bytes_delivered, ms[ms.size() / 2]);
    return results[0].status == kOk ? 0 : 1;
}
