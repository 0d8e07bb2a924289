// ohm_rx_core_driver.cpp -- runs csrc/ohm_rx_core.h on the CPU the way csrc/ohm_rx_kernel.hip runs it on the device, for
// tests/test_ohm_rx_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   ohm_rx_core_driver JOB OUT
// JOB:  u32 n_streams, n_datagrams; u64 src_bytes, dst_bytes; the stream table (ohmrx::Stream); the datagram table (ohmrx::Datagram);
//       the source arena; the destination arena as it is before the run.
// OUT:  the records (ohmrx::Record per datagram); the results (ohmrx::StreamResult per stream); the destination arena.
// The three phases in the device's order: every datagram parsed, every stream sequenced with a ring of its own, every datagram
// gathered a lane at a time, 64 lanes a datagram.  The arenas are heap blocks exactly as large as the job says, so that a stray
// index is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ohpipeline_amd/csrc/ohm_rx_core.h"

using namespace ohmrx;

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint32_t counts[2];
    uint64_t sizes[2];
    if (!read_all(f, counts, 2) || !read_all(f, sizes, 2)) return 1;
    std::vector<Stream> streams(counts[0]);
    std::vector<Datagram> grams(counts[1]);
    // (heap blocks of the exact size, not vectors: nothing behind them that a stray byte could land in unseen)
    uint8_t* src = (uint8_t*)malloc(sizes[0] ? sizes[0] : 1);
    uint8_t* dst = (uint8_t*)malloc(sizes[1] ? sizes[1] : 1);
    if (!read_all(f, streams.data(), streams.size()) || !read_all(f, grams.data(), grams.size()) || !read_all(f, src, sizes[0]) || !read_all(f, dst, sizes[1])) {
        fprintf(stderr, "short job file\n");
        return 1;
    }
    fclose(f);

    std::vector<Record> recs(grams.size());
    std::vector<StreamResult> results(streams.size());
    for (size_t k = 0; k < grams.size(); k++) parse(src + grams[k].src_offset, grams[k].bytes, &recs[k]);
    for (size_t i = 0; i < streams.size(); i++) {
        uint32_t* ring = (uint32_t*)malloc(kRing * sizeof(uint32_t));
        memset(ring, 0xff, kRing * sizeof(uint32_t));                  // (an index that was never written would leave the records)
        sequence(streams[i], recs.data() + streams[i].first_datagram, ring, &results[i]);
        free(ring);
    }
    for (size_t k = 0; k < grams.size(); k++) {
        const Record& r = recs[k];
        if (r.disposition != kOutput || r.audio_bytes == 0) continue;
        for (uint32_t lane = 0; lane < 64; lane++)
            gather_lane(src + grams[k].src_offset + r.audio_offset, dst + r.dst_offset, r.audio_bytes, lane, 64);
    }

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    fwrite(recs.data(), sizeof(Record), recs.size(), f);
    fwrite(results.data(), sizeof(StreamResult), results.size(), f);
    fwrite(dst, 1, sizes[1], f);
    fclose(f);
    free(src); free(dst);
    return 0;
}
