// mp4f_serial.cpp -- the baseline of tools/bench_mp4f.py on the host: csrc/mp4_frag_core.h's serial text (what the plain route's lane
// runs: the walk, the runs' totals, the carries, the serial expansion, finish, every piece through ohmrx::gather_lane with one lane) over
// STREAMS copies of one file, stream i at address i mod 16 and gathered to address (i / 16) mod 16, on THREADS host threads that take the
// streams in turns.  Built without sanitizers (tests/cpp/mp4f_core_driver.cpp is the build with them):
//   g++ -O2 -std=c++17 -pthread tools/mp4f_serial.cpp -o mp4f_serial;  mp4f_serial FILE STREAMS THREADS RUNS
// Prints one line: the runs' wall times in milliseconds (the arenas and tables are allocated and touched before the first), then the sum of
// bytes_gathered, the number of streams whose status is OK, and a position-weighted sum of the first and the last stream's gathered bytes,
// which the caller checks.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../ohpipeline_amd/csrc/mp4_frag_core.h"
#include "../ohpipeline_amd/csrc/ohm_rx_core.h"

using namespace mp4frag;

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s FILE STREAMS THREADS RUNS\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<uint8_t> file;
    for (uint8_t buf[1 << 16];;) { const size_t got = fread(buf, 1, sizeof(buf), f); if (!got) break; file.insert(file.end(), buf, buf + got); }
    fclose(f);
    const size_t ns = (size_t)atol(argv[2]), threads = std::min<size_t>((size_t)atol(argv[3]), 16), runs = (size_t)atol(argv[4]);
    if (!ns || !threads || !runs || file.size() >= 0x80000000ull) return 2;
    // the shape: one walk that expands nothing
    Stream probe = {};
    probe.src_bytes = (uint32_t)file.size(); probe.codecs = kCodecAlac | kCodecFlac;
    Result shape;
    Rec rec0;
    walk(probe, file.data(), false, &shape, &rec0, nullptr);
    if (shape.status != kOk) { fprintf(stderr, "the file's status is %u\n", shape.status); return 1; }
    const size_t rows = (size_t)shape.samples, n_runs = shape.runs, stride_src = (file.size() + 15) / 16 * 16 + 16, stride_dst = stride_src;
    std::vector<uint8_t> src(ns * stride_src + 16), dst(ns * stride_dst + 16, 0xa5);
    std::vector<Stream> streams(ns);
    for (size_t i = 0; i < ns; i++) {
        Stream& s = streams[i];
        s = probe;
        s.src_offset = i * stride_src + i % 16; s.flags = kGather;
        s.packet_first = (uint32_t)(i * rows); s.packet_capacity = (uint32_t)rows; s.run_first = (uint32_t)(i * n_runs); s.run_capacity = (uint32_t)n_runs;
        s.dst_offset = i * stride_dst + (i / 16) % 16; s.dst_capacity = file.size();
        memcpy(src.data() + s.src_offset, file.data(), file.size());
    }
    std::vector<Result> results(ns);
    std::vector<RunRec> recs(ns * n_runs);
    std::vector<Run> run_rows(ns * n_runs);
    std::vector<Row> packets(ns * rows);
    std::vector<Sample> samples(ns * rows);
    auto one = [&](size_t i) {
        const Stream& s = streams[i];
        const uint8_t* p = src.data() + s.src_offset;
        RunRec* my = recs.data() + s.run_first;
        Rec rec;
        Result& r = results[i];
        walk(s, p, false, &r, &rec, my);
        for (uint32_t k = 0; k < rec.runs_written; k++)
            if (needs_sums(my[k])) totals_serial(p, my[k], my[k].samples, &my[k].bytes, &my[k].frames);
        carries(s, &rec, my, run_rows.data() + s.run_first, &r);
        expand_serial(s, p, rec, my, packets.data() + s.packet_first, samples.data() + s.packet_first, &r);
        finish(s, &rec, my, packets.data() + s.packet_first, &r);
        for (uint32_t k = 0; k < rec.runs_written; k++) {
            uint64_t from, to;
            uint32_t n;
            if (piece_of(s, rec, my, packets.data() + s.packet_first, r, k, &from, &to, &n)) ohmrx::gather_lane(src.data() + from, dst.data() + to, n, 0u, 1u);
        }
    };
    for (size_t run = 0; run < runs; run++) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (size_t t = 0; t < threads; t++) pool.emplace_back([&, t] { for (size_t i = t; i < ns; i += threads) one(i); });
        for (std::thread& th : pool) th.join();
        printf("%.3f ", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    uint64_t gathered = 0, ok = 0;
    for (const Result& r : results) { gathered += r.bytes_gathered; ok += r.status == kOk && r.samples_refused == 0; }
    // a position-weighted sum of the first and the last stream's gathered run, for the caller to hold against its own
    uint64_t sums[2] = {0, 0};
    for (int e = 0; e < 2; e++) {
        const Stream& s = streams[e ? ns - 1 : 0];
        const uint64_t n = results[e ? ns - 1 : 0].bytes_gathered;
        for (uint64_t k = 0; k < n; k++) sums[e] += (uint64_t)dst[s.dst_offset + k] * (k % 65521u + 1u);
    }
    printf("\n%llu %llu %llu %llu\n", (unsigned long long)gathered, (unsigned long long)ok, (unsigned long long)sums[0], (unsigned long long)sums[1]);
    return 0;
}
