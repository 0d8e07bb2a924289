// alac_core_cpu.cpp -- csrc/alac_packet_core.h (the text the Apple Lossless kernels run) on host threads: the CPU figure that
// tools/bench_alac_decode.py prints beside the device's.  This is the project's own core, not the reference's decoder.
// usage: alac_core_cpu JOB threads   ->   one line: samples (per channel) per second, a checksum
// JOB: u32 n_streams, n_packets; u64 src_bytes, dst_bytes; alaccore::Stream[], alaccore::Packet[], the source arena.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../ohpipeline_amd/csrc/alac_packet_core.h"

using namespace alaccore;

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB threads\n", argv[0]); return 2; }
    const uint32_t threads = (uint32_t)atoi(argv[2]);
    FILE* f = fopen(argv[1], "rb");
    uint32_t counts[2];
    uint64_t sizes[2];
    if (!f || fread(counts, 4, 2, f) != 2 || fread(sizes, 8, 2, f) != 2) { perror("job"); return 2; }
    std::vector<Stream> streams(counts[0]);
    std::vector<Packet> packets(counts[1]);
    std::vector<uint8_t> src(sizes[0]), dst(sizes[1]);
    if (fread(streams.data(), sizeof(Stream), streams.size(), f) != streams.size() || fread(packets.data(), sizeof(Packet), packets.size(), f) != packets.size() ||
        fread(src.data(), 1, src.size(), f) != src.size()) { fprintf(stderr, "short job\n"); return 2; }
    fclose(f);
    std::vector<uint64_t> group_base;
    std::vector<uint32_t> row_packet;
    plan_rows(streams.data(), packets.data(), packets.size(), &group_base, &row_packet);
    std::vector<int32_t> scratch((size_t)group_base.back() * kGroupRows);
    std::vector<Chan> chans(row_packet.size());
    std::vector<PacketOut> outs(packets.size());
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (size_t i = t; i < packets.size(); i += threads) {
                const Packet& pk = packets[i];
                const PlainRows rows{scratch.data(), group_base.data(), pk.row0};
                decode_packet(src.data() + pk.src_offset, pk, streams[pk.stream], chans.data() + pk.row0, rows, dst.data(), &outs[i]);
            }
        });
    for (std::thread& th : pool) th.join();
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t samples = 0;
    uint32_t sum = 0;
    for (const PacketOut& o : outs) samples += o.samples;
    for (uint8_t b : dst) sum += b;
    printf("%.1f %u\n", (double)samples / sec, sum);
    return 0;
}
