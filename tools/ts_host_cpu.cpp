// ts_host_cpu.cpp -- the host leg of tools/bench_ts.py: this project's own transport stream and ADTS core (csrc/ts_packet_core.h) on the
// CPU, a stream a task on THREADS threads -- tspkt::demux (classify, tables, sums, the gather piece by piece) and then adts::walk over
// the run with recognition.  Not the reference's container: the same serial text the device's plain route runs, on the host.
//   ts_host_cpu FILE STREAMS THREADS REPEATS     FILE holds one stream's bytes; every stream is a copy of it.  Prints the bytes one
//   stream delivered, the frames its chain found, and the median wall time of a pass over all streams in milliseconds.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../ohpipeline_amd/csrc/ts_packet_core.h"

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
    const uint32_t np = (uint32_t)(one.size() / tspkt::kPacket);
    const size_t room = (size_t)np * 184u + 16u;
    std::vector<uint8_t> src(one.size() * n_streams + 4), dst(room * n_streams);
    for (size_t i = 0; i < n_streams; i++) memcpy(src.data() + i * one.size(), one.data(), one.size());
    std::vector<tspkt::Result> results(n_streams);
    std::vector<adts::Result> chains(n_streams);
    std::vector<double> ms;
    for (size_t r = 0; r < repeats; r++) {
        std::atomic<size_t> next{0};
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (size_t t = 0; t < threads; t++)
            pool.emplace_back([&] {
                std::vector<tspkt::Pkt> pk(np + 1);
                std::vector<uint32_t> run_end(np + 1), src_at(np + 1);
                for (size_t i; (i = next++) < n_streams;) {
                    tspkt::Stream s = {};
                    s.src_offset = i * one.size();
                    s.dst_offset = i * room;
                    s.src_bytes = (uint32_t)one.size();
                    s.dst_capacity = (uint64_t)np * 184u;
                    tspkt::demux(s, src.data(), dst.data(), nullptr, pk.data(), run_end.data(), src_at.data(), &results[i]);
                    adts::Stream a = {};
                    a.src_offset = s.dst_offset;
                    a.src_bytes = results[i].bytes_delivered;
                    a.flags = adts::kRecognise;
                    adts::walk(a, dst.data(), nullptr, &chains[i]);
                }
            });
        for (auto& t : pool) t.join();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("%u %u %.3f\n", results[0].bytes_delivered, chains[0].frames, ms[ms.size() / 2]);
    return results[0].status == tspkt::kOk && chains[0].status == adts::kOk ? 0 : 1;
}
