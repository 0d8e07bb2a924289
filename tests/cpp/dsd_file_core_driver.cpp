// dsd_file_core_driver.cpp -- runs csrc/dsd_file_core.h on the CPU the way csrc/dsd_file_kernel.hip runs it on the device, for
// tests/test_dsd_file_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   dsd_file_core_driver JOB OUT
// JOB:  u64 n_streams, src_bytes, dst_bytes; the descriptors (dsdfile::Stream); the source arena.
// OUT:  twice -- the fused route, then the plain route -- the results (dsdfile::Result per stream) and the destination arena, 0xA5
//       where nothing was written.
// The fused route in the device's order: every stream walked; then per stream the workgroups the plan gives it (from
// dst_bytes_capacity alone), each wave taking its piece lane by lane.  The plain route: the walk, the byte-wise conversion and the
// fill.  Every stream's bytes are copied into a heap block of their own that ends where they end (built with -DOHGPU_ALIGNED_READS the
// core reads as the device does, in aligned words, and the block is rounded up to a whole word) and begins src_offset mod 16 bytes in
// front of them, so that the audio lies at the address mod 16 it has in the arena and a 16-byte line that does not lie whole inside
// the stream is the sanitizer's to report; the destination arena is one heap block of exactly dst_bytes.  A step counter holds the
// walk to its bound.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static unsigned long long g_steps;
#define DSDF_STEP() (g_steps++)
#include "../../ohpipeline_amd/csrc/dsd_file_core.h"

using namespace dsdfile;

constexpr uint32_t kGroupPieces = 2, kLanes = 64;   // kDsdFileGroupPieces, a wave

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint64_t head[3];
    if (!read_all(f, head, 3)) return 1;
    const size_t ns = head[0], dst_bytes = head[2];
    std::vector<Stream> streams(ns);
    std::vector<uint8_t> arena(head[1]);
    if (!read_all(f, streams.data(), ns) || !read_all(f, arena.data(), arena.size())) { fprintf(stderr, "short job file\n"); return 1; }
    fclose(f);
    std::vector<uint8_t*> blocks(ns), bytes(ns);
    for (size_t i = 0; i < ns; i++) {
        const size_t lead = streams[i].src_offset % 16u;
        size_t size = lead + streams[i].src_bytes;
#if defined(OHGPU_ALIGNED_READS)
        size = (size + 3u) & ~(size_t)3u;
#endif
        if (posix_memalign((void**)&blocks[i], 16, size ? size : 1)) return 1;       // (16-aligned, and exactly `size` bytes to the sanitizer)
        memset(blocks[i], 0, size ? size : 1);
        bytes[i] = blocks[i] + lead;
        if (streams[i].src_bytes) memcpy(bytes[i], arena.data() + streams[i].src_offset, streams[i].src_bytes);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    for (int route = 0; route < 2; route++) {
        std::vector<Result> results(ns);
        std::vector<Rec> recs(ns);
        uint8_t* dst = nullptr;
        if (posix_memalign((void**)&dst, 16, dst_bytes ? dst_bytes : 1)) return 1;
        memset(dst, 0xa5, dst_bytes ? dst_bytes : 1);
        for (size_t i = 0; i < ns; i++) {
            g_steps = 0;
            walk(streams[i], bytes[i], &results[i], &recs[i]);
            if (g_steps > kMaxChunks + 1ull) { fprintf(stderr, "stream %zu: the walk read %llu chunk headers\n", i, g_steps); return 1; }
            const Rec& c = recs[i];
            if (c.fill_to > streams[i].dst_bytes_capacity || c.fill_from > c.fill_to) { fprintf(stderr, "stream %zu: the run is larger than its room\n", i); return 1; }
            if (c.n == 0u) continue;
            const uint8_t* audio = bytes[i] + c.data_offset;
            uint8_t* to = dst + c.dst_pos;
            if (route == 1) {
                convert_bytes(c, audio, to, 0, c.fill_from, 0, 1);
                fill_bytes(to, c.fill_from, c.fill_to, 0, 1);
                continue;
            }
            const uint64_t pieces = room_pieces(streams[i]), groups = (pieces + kGroupPieces - 1u) / kGroupPieces;
            if ((uint64_t)c.n > pieces * kPieceChunks) { fprintf(stderr, "stream %zu: the plan has too few workgroups\n", i); return 1; }
            for (uint64_t g = 0; g < groups; g++)
                for (uint32_t wave = 0; wave < kGroupPieces; wave++) {
                    const uint32_t piece = (uint32_t)g * kGroupPieces + wave;
                    if ((uint64_t)piece * kPieceChunks >= c.n) continue;
                    for (uint32_t lane = 0; lane < kLanes; lane++)
                        convert_piece(c, audio, bytes[i] + streams[i].src_bytes, to, piece, ((uintptr_t)to & 15u) == 0u, lane, kLanes);
                }
        }
        fwrite(results.data(), sizeof(Result), ns, f);
        fwrite(dst, 1, dst_bytes, f);
        free(dst);
    }
    fclose(f);
    for (uint8_t* b : blocks) free(b);
    return 0;
}
