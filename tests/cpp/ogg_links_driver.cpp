// ogg_links_driver.cpp -- the walk of csrc/ogg_page_core.h with OHGPU_OGG_FOLLOW_LINKS on the CPU, for tests/test_ogg_links_core_cpu.py
// (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   ogg_links_driver JOB OUT
// JOB and OUT are tests/cpp/ogg_core_driver.cpp's: u64 n_streams, n_packets, src_bytes, dst_bytes, the descriptors, the two arenas
// in; the results, the packet table and the destination arena out.  That driver takes a job through all four phases; this one is
// about the chain phase alone, so it gives the walk no bitmap: every page's checksum is run where the walk stands on it, which is
// what the walk does for itself when the candidate list overflowed.  The stream's bytes are copied into a heap block of their own
// size before the walk, so that a read in front of or behind a stream -- a magic compared against a body shorter than it, say -- is
// the sanitizer's to report, and so is a piece beyond piece_capacity() or a record beyond packet_capacity.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ohpipeline_amd/csrc/ogg_page_core.h"
#include "../../ohpipeline_amd/csrc/ohm_rx_core.h"

using namespace oggpage;

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint64_t head[4];
    if (!read_all(f, head, 4)) return 1;
    std::vector<Stream> streams(head[0]);
    std::vector<uint8_t> src(head[2]);
    uint8_t* dst = (uint8_t*)malloc(head[3] ? head[3] : 1);
    if (!read_all(f, streams.data(), streams.size()) || !read_all(f, src.data(), src.size()) || !read_all(f, dst, head[3])) {
        fprintf(stderr, "short job file\n");
        return 1;
    }
    fclose(f);

    Tables tables;
    make_tables(&tables);
    std::vector<Result> results(streams.size());
    std::vector<Packet> table(head[1]);
    if (!table.empty()) memset(table.data(), 0, table.size() * sizeof(Packet));
    for (size_t i = 0; i < streams.size(); i++) {
        Stream s = streams[i];
        uint8_t* own = (uint8_t*)malloc(s.src_bytes ? s.src_bytes : 1);
        if (s.src_bytes) memcpy(own, src.data() + s.src_offset, s.src_bytes);
        Packet* records = (Packet*)malloc(s.packet_capacity ? s.packet_capacity * sizeof(Packet) : 1);
        if (s.packet_capacity) memset(records, 0, s.packet_capacity * sizeof(Packet));
        const uint32_t room = piece_capacity(s);
        Piece* pieces = (Piece*)malloc(room * sizeof(Piece));
        auto good = [&](uint32_t, const uint8_t* page, uint32_t bytes) { return crc_run(tables.byte, page, 0, bytes) == stored_crc(page); };
        const uint64_t src_offset = s.src_offset;
        const uint32_t packet_first = s.packet_first;
        s.src_offset = 0; s.packet_first = 0;                         // (the walk adds them to the bases it is given)
        uint32_t n_pieces = 0;
        walk(s, (uint32_t)i, own, records, pieces, good, &results[i], &n_pieces);
        if (n_pieces > room) { fprintf(stderr, "stream %zu: %u pieces where %u have room\n", i, n_pieces, room); return 1; }
        uint64_t planned = 0;
        for (uint32_t k = 0; k < n_pieces; k++) {
            const Piece& g = pieces[k];
            if (g.run_pos != planned) { fprintf(stderr, "stream %zu: piece %u goes to %u where the run has %llu bytes\n", i, k, g.run_pos, (unsigned long long)planned); return 1; }
            planned += g.bytes;
            for (uint32_t lane = 0; lane < 64; lane++)
                ohmrx::gather_lane(src.data() + src_offset + g.src_pos, dst + s.dst_offset + g.run_pos, g.bytes, lane, 64);
        }
        if (planned != results[i].bytes_delivered) { fprintf(stderr, "stream %zu: the plan has %llu bytes, the result %llu\n", i, (unsigned long long)planned, (unsigned long long)results[i].bytes_delivered); return 1; }
        if (s.packet_capacity) memcpy(table.data() + packet_first, records, s.packet_capacity * sizeof(Packet));
        free(pieces); free(records); free(own);
    }

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    fwrite(results.data(), sizeof(Result), results.size(), f);
    fwrite(table.data(), sizeof(Packet), table.size(), f);
    fwrite(dst, 1, head[3], f);
    fclose(f);
    free(dst);
    return 0;
}
