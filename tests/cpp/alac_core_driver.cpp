// alac_core_driver.cpp -- runs csrc/alac_packet_core.h on the CPU the way csrc/alac_packet_kernel.hip runs it on the device, for
// tests/test_alac_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   alac_core_driver JOB OUT fused|plain
// JOB:  u32 n_streams, n_packets; u64 src_bytes, dst_bytes; the streams (alaccore::Stream), the packets (alaccore::Packet), the
//       source arena, the destination arena as it is before the run.
// OUT:  alaccore::PacketOut per packet, then the destination arena.
// "fused" is the three phases over the transposed scratch -- every packet's entropy pass, then every row's predictor, then every
// sample's finish and store --, "plain" is decode_packet over the row-major scratch.  The scratch is exactly as large as the plan says
// and the arenas exactly as large as the job says, so that a stray index is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ohpipeline_amd/csrc/alac_packet_core.h"

using namespace alaccore;

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s JOB OUT fused|plain\n", argv[0]); return 2; }
    const bool plain = strcmp(argv[3], "plain") == 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint32_t counts[2];
    uint64_t sizes[2];
    if (!read_all(f, counts, 2) || !read_all(f, sizes, 2)) return 1;
    std::vector<Stream> streams(counts[0]);
    std::vector<Packet> packets(counts[1]);
    // (heap blocks of the exact size, not vectors: nothing behind them that a stray byte could land in unseen)
    uint8_t* src = (uint8_t*)malloc(sizes[0] ? sizes[0] : 1);
    uint8_t* dst = (uint8_t*)malloc(sizes[1] ? sizes[1] : 1);
    if (!read_all(f, streams.data(), streams.size()) || !read_all(f, packets.data(), packets.size()) || !read_all(f, src, sizes[0]) || !read_all(f, dst, sizes[1])) {
        fprintf(stderr, "short job file\n");
        return 1;
    }
    fclose(f);

    std::vector<uint64_t> group_base;
    std::vector<uint32_t> row_packet;
    plan_rows(streams.data(), packets.data(), packets.size(), &group_base, &row_packet);
    const size_t words = (size_t)group_base.back() * kGroupRows;
    int32_t* scratch = (int32_t*)malloc(words ? words * 4 : 4);
    memset(scratch, 0x5b, words * 4);
    std::vector<Chan> chans(row_packet.size());
    std::vector<PacketOut> outs(packets.size());

    if (plain) {
        for (size_t i = 0; i < packets.size(); i++) {
            const Packet& pk = packets[i];
            const PlainRows rows{scratch, group_base.data(), pk.row0};
            decode_packet(src + pk.src_offset, pk, streams[pk.stream], chans.data() + pk.row0, rows, dst, &outs[i]);
        }
    } else {
        for (size_t i = 0; i < packets.size(); i++) {
            const Packet& pk = packets[i];
            const TransposedRows rows{scratch, group_base.data(), pk.row0};
            uint32_t n = 0;
            const int st = parse_packet(src + pk.src_offset, pk.bytes, streams[pk.stream], chans.data() + pk.row0, rows, &n);
            outs[i].status = (uint32_t)st;
            outs[i].samples = st == kStatusOk ? n : 0u;
        }
        for (size_t r = 0; r < row_packet.size(); r++) {
            if (row_packet[r] == ~0u || outs[row_packet[r]].status != kStatusOk) continue;
            predict_row(chans[r], transposed_row(scratch, group_base.data(), (uint32_t)r), outs[row_packet[r]].samples);
        }
        for (size_t r = 0; r < row_packet.size(); r++) {
            if (row_packet[r] == ~0u || outs[row_packet[r]].status != kStatusOk) continue;
            const Packet& pk = packets[row_packet[r]];
            const Stream& s = streams[pk.stream];
            const Chan& ch = chans[r];
            const Row mine = transposed_row(scratch, group_base.data(), (uint32_t)r);
            const Row other = transposed_row(scratch, group_base.data(), (uint32_t)(ch.place == 1 ? r + 1 : ch.place == 2 ? r - 1 : r));
            for (uint32_t i = 0; i < outs[row_packet[r]].samples; i++)
                store_sample(s, dst, (uint64_t)pk.index * s.frame_length + i, (uint32_t)r - pk.row0,
                             finish_sample(ch, mine.get(i), other.get(i), src + pk.src_offset, pk.bytes, i));
        }
    }

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    fwrite(outs.data(), sizeof(PacketOut), outs.size(), f);
    fwrite(dst, 1, sizes[1], f);
    fclose(f);
    free(scratch); free(src); free(dst);
    return 0;
}
