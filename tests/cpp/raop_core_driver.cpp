// raop_core_driver.cpp -- runs csrc/raop_aes_core.h on the CPU the way csrc/raop_decrypt_kernel.hip runs it on the device, for
// tests/test_raop_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   raop_core_driver JOB OUT
// JOB:  u32 n_streams, n_packets; u64 src_bytes, dst_bytes; per stream a raopcore::StreamIn, 16 key bytes and 16 IV bytes; the packet
//       table (raopcore::PacketIn); the source arena; the destination arena as it is before the run.
// OUT:  u64 scratch_bytes; the plaintext scratch; the destination arena.
// The schedule is made per stream, the jobs and the pieces are planned as ohgpu_raop_batch_create plans them, and every piece is run
// a lane at a time, 64 lanes a piece, with the tables as plain arrays.  The scratch is exactly as large as the plan says (pre-filled
// with 0x5b) and the arenas exactly as large as the job says, so that a stray index is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ohpipeline_amd/csrc/raop_aes_core.h"

using namespace raopcore;

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static constexpr Tables kTables = make_tables();

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint32_t counts[2];
    uint64_t sizes[2];
    if (!read_all(f, counts, 2) || !read_all(f, sizes, 2)) return 1;
    std::vector<StreamIn> streams(counts[0]);
    std::vector<uint32_t> keys((size_t)counts[0] * kKeyWords);
    for (uint32_t i = 0; i < counts[0]; i++) {
        uint8_t secret[32];
        if (!read_all(f, &streams[i], 1) || !read_all(f, secret, 32)) return 1;
        expand_decrypt_key(secret, &keys[(size_t)i * kKeyWords], kTables);
        load_iv(secret + 16, &keys[(size_t)i * kKeyWords + kRoundKeyWords]);
    }
    std::vector<PacketIn> packets(counts[1]);
    // (heap blocks of the exact size, not vectors: nothing behind them that a stray byte could land in unseen)
    uint8_t* src = (uint8_t*)malloc(sizes[0] ? sizes[0] : 1);
    uint8_t* dst = (uint8_t*)malloc(sizes[1] ? sizes[1] : 1);
    if (!read_all(f, packets.data(), packets.size()) || !read_all(f, src, sizes[0]) || !read_all(f, dst, sizes[1])) {
        fprintf(stderr, "short job file\n");
        return 1;
    }
    fclose(f);

    std::vector<Job> jobs;
    const uint64_t scratch_bytes = plan_jobs(streams.data(), streams.size(), packets.data(), &jobs);
    std::vector<Piece> pieces;
    plan_pieces(jobs.data(), jobs.size(), &pieces);
    uint8_t* scratch = (uint8_t*)malloc(scratch_bytes ? scratch_bytes : 1);
    memset(scratch, 0x5b, scratch_bytes);
    for (const Piece& pc : pieces)
        for (uint32_t lane = 0; lane < (uint32_t)kPieceBlocks; lane++)
            piece_lane(pc, lane, &keys[(size_t)pc.key * kKeyWords], src, pc.to_arena ? dst : scratch, kTables.td0, kTables.isbox);

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    fwrite(&scratch_bytes, sizeof(scratch_bytes), 1, f);
    fwrite(scratch, 1, scratch_bytes, f);
    fwrite(dst, 1, sizes[1], f);
    fclose(f);
    free(scratch); free(src); free(dst);
    return 0;
}
