// ogg_core_driver.cpp -- runs csrc/ogg_page_core.h on the CPU the way csrc/ogg_page_kernel.hip runs it on the device, for
// tests/test_ogg_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   ogg_core_driver JOB OUT [LIST]
// JOB:  u64 n_streams, n_packets, src_bytes, dst_bytes; the descriptors (oggpage::Stream); the source arena; the destination arena
//       as it is before the run.
// OUT:  the results (oggpage::Result per stream); the packet table (oggpage::Packet, n_packets records, zero where nothing was
//       written); the destination arena.
// LIST: the candidate list's capacity, where the test wants it smaller than the plan's sum(src_bytes / 27 + 1).
// The four phases in the device's order: every byte position of every stream tried for a page image; every listed candidate's
// checksum as the xor of 64 lanes' terms, a good one's bit set; every stream walked, its pieces appended to the work list; every piece
// gathered a lane at a time, 64 lanes a piece.  The arenas, the list, the bitmap and every stream's piece region are heap blocks
// exactly as large as the plan says, so that a stray index is the sanitizer's to report.
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
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s JOB OUT [LIST]\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint64_t head[4];
    if (!read_all(f, head, 4)) return 1;
    std::vector<Stream> streams(head[0]);
    // (heap blocks of the exact size, not vectors: nothing behind them that a stray byte could land in unseen)
    uint8_t* src = (uint8_t*)malloc(head[2] ? head[2] : 1);
    uint8_t* dst = (uint8_t*)malloc(head[3] ? head[3] : 1);
    if (!read_all(f, streams.data(), streams.size()) || !read_all(f, src, head[2]) || !read_all(f, dst, head[3])) {
        fprintf(stderr, "short job file\n");
        return 1;
    }
    fclose(f);

    Tables tables;
    make_tables(&tables);
    uint64_t cap = 0, n_bits = 0;
    std::vector<uint64_t> bit_base(streams.size());
    for (size_t i = 0; i < streams.size(); i++) {
        bit_base[i] = n_bits;
        n_bits += ((uint64_t)streams[i].src_bytes + 31u) & ~(uint64_t)31u;
        cap += streams[i].src_bytes / 27u + 1u;
    }
    if (argc == 4) cap = strtoull(argv[3], nullptr, 10);

    // find
    Candidate* list = (Candidate*)malloc(cap ? cap * sizeof(Candidate) : 1);
    uint64_t found = 0;
    for (size_t i = 0; i < streams.size(); i++) {
        const Stream& s = streams[i];
        for (uint32_t pos = 0; pos < s.src_bytes; pos++) {
            Page pg;
            if (parse_page(src + s.src_offset + pos, s.src_bytes - pos, &pg) != 1) continue;
            if (found < cap) list[found] = Candidate{(uint32_t)i, pos, pg.bytes, 0u};
            found++;
        }
    }
    // verify
    uint32_t* bits = (uint32_t*)calloc(n_bits ? n_bits / 32u : 1u, sizeof(uint32_t));
    for (uint64_t k = 0; k < (found < cap ? found : cap); k++) {
        const Candidate& c = list[k];
        const uint8_t* page = src + streams[c.stream].src_offset + c.pos;
        uint32_t sum = 0;
        for (uint32_t lane = 0; lane < kLanes; lane++) sum ^= crc_lane(tables.byte, tables.shift, tables.shift256, page, c.bytes, lane);
        if (sum != crc_run(tables.byte, page, 0, c.bytes)) { fprintf(stderr, "the lanes' sum is not the page's checksum (%u bytes)\n", c.bytes); return 1; }
        if (sum == stored_crc(page)) {
            const uint64_t b = bit_base[c.stream] + c.pos;
            bits[b >> 5] |= 1u << (b & 31u);
        }
    }
    // chain
    std::vector<Result> results(streams.size());
    Packet* packets = (Packet*)calloc(head[1] ? head[1] : 1, sizeof(Packet));
    std::vector<Piece*> regions(streams.size());
    std::vector<const Piece*> work;
    const bool overflowed = found > cap;
    for (size_t i = 0; i < streams.size(); i++) {
        const uint64_t my_bits = bit_base[i];
        regions[i] = (Piece*)malloc(piece_capacity(streams[i]) * sizeof(Piece));
        auto good = [&](uint32_t pos, const uint8_t* page, uint32_t bytes) { return page_good(bits, my_bits, pos, overflowed, &tables, page, bytes); };
        uint32_t n_pieces = 0;
        walk(streams[i], (uint32_t)i, src, packets, regions[i], good, &results[i], &n_pieces);
        if (n_pieces > piece_capacity(streams[i])) { fprintf(stderr, "stream %zu: %u pieces\n", i, n_pieces); return 1; }
        for (uint32_t k = 0; k < n_pieces; k++) work.push_back(regions[i] + k);
    }
    // gather
    for (const Piece* g : work) {
        const Stream& s = streams[g->stream];
        for (uint32_t lane = 0; lane < 64; lane++)
            ohmrx::gather_lane(src + s.src_offset + g->src_pos, dst + s.dst_offset + g->run_pos, g->bytes, lane, 64);
    }

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    fwrite(results.data(), sizeof(Result), results.size(), f);
    fwrite(packets, sizeof(Packet), head[1], f);
    fwrite(dst, 1, head[3], f);
    fclose(f);
    for (Piece* r : regions) free(r);
    free(list); free(bits); free(packets); free(src); free(dst);
    return 0;
}
