// dsd_pcm_cpu.cpp -- csrc/dsd_pcm_core.h (the text the plain DSD -> PCM kernel runs per thread) on host threads: the CPU figure that
// tools/bench_dsd_pcm.py prints beside the device's.  Streams of seeded bits, P = 0, one stream after another per thread.
// usage: dsd_pcm_cpu D T coef.bin streams frames threads   ->   one line: output frames per second
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../ohpipeline_amd/csrc/dsd_pcm_core.h"

int main(int argc, char** argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s D T coef.bin streams frames threads\n", argv[0]); return 2; }
    const uint32_t D = (uint32_t)atoi(argv[1]), T = (uint32_t)atoi(argv[2]), N = D * T;
    const uint32_t streams = (uint32_t)atoi(argv[4]), frames = (uint32_t)atoi(argv[5]), threads = (uint32_t)atoi(argv[6]);
    std::vector<int32_t> coef(N);
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(coef.data(), 4, N, f) != N) { perror("coef"); return 2; }
    fclose(f);
    const uint64_t chunks = ((uint64_t)frames * D + 15) / 16, stream_bytes = chunks * 4;
    std::vector<uint8_t> src(stream_bytes * streams), dst((size_t)frames * 6 * streams);
    uint32_t x = 12345u;
    for (uint8_t& b : src) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
    uint16_t table[512] = {0};
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (uint32_t s = t; s < streams; s += threads) {
                ohgpu_dsd_pcm_msg_desc d = {};
                d.src_offset = s * stream_bytes; d.src_chunks = chunks; d.dst_offset = (uint64_t)s * frames * 6; d.n_frames = frames;
                d.sample_block_words = 2; d.dst_endian = OHGPU_ENDIAN_BIG;
                for (uint64_t q = 0; q < 2ull * frames; q++) dsdpcm::convert_value(d, coef.data(), N, D, src.data(), dst.data(), table, q);
            }
        });
    for (std::thread& th : pool) th.join();
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint32_t sum = 0;
    for (uint8_t b : dst) sum += b;
    printf("%.1f %u\n", (double)streams * frames / sec, sum);
    return 0;
}
