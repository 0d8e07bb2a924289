// ohm_rx_host_cpu.cpp -- the host leg of tools/bench_ohm_rx.py: what a host pays for the in-order shape when it parses every datagram
// and copies every payload itself.
//   ohm_rx_host_cpu STREAMS FRAMES THREADS REPS
// Makes STREAMS x FRAMES Songcast audio datagrams of 1440 audio bytes and a 4-byte codec name (stereo S24 / 48 kHz, 5 ms) with the
// oracle's writer (oracle/ohp_songcast.h: TEST INFRASTRUCTURE, allowed here as a bench's CPU baseline), each at a multiple of 16 of one
// arena, stream by stream; then, REPS times, THREADS threads take contiguous shares of the datagrams, call the oracle's
// ohp_ohm_audio_parse on each and memcpy its payload to where an in-order receiver puts it.  No sequencer: the oracle has none, and
// in order there is nothing to put in order.  Prints the median wall time of the parallel section in milliseconds.
// This is the oracle and memcpy on the CPUs the process is granted, NOT the reference, which parses one datagram at a time on a
// protocol thread per stream.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "ohp_songcast.h"

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s STREAMS FRAMES THREADS REPS\n", argv[0]); return 2; }
    const size_t streams = (size_t)atol(argv[1]), frames = (size_t)atol(argv[2]);
    const unsigned threads = (unsigned)std::max(1, atoi(argv[3]));
    const int reps = std::max(1, atoi(argv[4]));
    const uint32_t audio_bytes = 1440, gram = 58 + 4 + audio_bytes, slot = (gram + 15) / 16 * 16;
    const size_t n = streams * frames;
    std::vector<uint8_t> src(n * slot), dst(n * audio_bytes);
    uint8_t header[OHP_OHM_STREAM_HEADER_BYTES], audio[1440];
    const int header_bytes = ohp_ohm_stream_header(header, sizeof(header), 0, 48000, 48000 * 48, 0, 24, 2, (const uint8_t*)"PCM ", 4);
    if (header_bytes != 26) { fprintf(stderr, "stream header: %d\n", header_bytes); return 1; }
    uint32_t x = 1;
    for (size_t k = 0; k < n; k++) {
        for (uint8_t& b : audio) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
        const uint32_t frame = (uint32_t)(k % frames);
        if (ohp_ohm_audio_frame(&src[k * slot], slot, OHP_OHM_FLAG_LOSSLESS, 240, frame, 0, 4800, (uint64_t)frame * 240, header, (uint32_t)header_bytes, audio, audio_bytes) != (int)gram) {
            fprintf(stderr, "datagram %zu was not made\n", k);
            return 1;
        }
    }
    std::vector<double> ms;
    std::vector<int> bad(threads, 0);
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < threads; t++)
            pool.emplace_back([&, t] {
                for (size_t k = n * t / threads; k < n * (t + 1) / threads; k++) {
                    ohp_ohm_audio a;
                    if (ohp_ohm_audio_parse(&src[k * slot], gram, &a) != OHP_OK || a.audio_bytes != audio_bytes) { bad[t]++; continue; }
                    memcpy(&dst[k * audio_bytes], &src[k * slot + a.audio_offset], a.audio_bytes);
                }
            });
        for (std::thread& th : pool) th.join();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    for (int b : bad) if (b) { fprintf(stderr, "%d datagrams did not parse\n", b); return 1; }
    if (memcmp(&dst[(n - 1) * audio_bytes], &src[(n - 1) * slot + 62], audio_bytes) != 0) { fprintf(stderr, "the last payload is not where it belongs\n"); return 1; }
    std::sort(ms.begin(), ms.end());
    printf("%.3f\n", ms[ms.size() / 2]);
    return 0;
}
