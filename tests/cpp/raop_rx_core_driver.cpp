// raop_rx_core_driver.cpp -- runs csrc/raop_rx_core.h on the CPU the way csrc/raop_rx_kernel.hip's plain route runs it on the device, for
// tests/test_raop_rx_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all, once with field_bytes.h's byte
// reader and once, -DOHGPU_ALIGNED_READS, with the device's aligned dword reader).
//   raop_rx_core_driver JOB OUT
// JOB:  u32 n_streams, n_datagrams; u64 src_bytes; the stream table (raoprx::Stream); the datagram table (raoprx::Datagram); the source
//       arena.
// OUT:  the records (raoprx::Record per datagram); the results (raoprx::StreamResult per stream); the packet rows (raoprx::PacketRow per
//       datagram).
// The three phases in the device's order: every datagram parsed, every stream sequenced with a waiting list of its own, every datagram's
// row written.  The arena, the keys and every waiting list are heap blocks exactly as large as they must be, so that a stray index is
// the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ohpipeline_amd/csrc/raop_rx_core.h"

using namespace raoprx;

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint32_t counts[2];
    uint64_t src_bytes;
    if (!read_all(f, counts, 2) || !read_all(f, &src_bytes, 1)) return 1;
    std::vector<Stream> streams(counts[0]);
    std::vector<Datagram> grams(counts[1]);
    uint8_t* src = (uint8_t*)malloc(src_bytes ? src_bytes : 1);
    if (!read_all(f, streams.data(), streams.size()) || !read_all(f, grams.data(), grams.size()) || !read_all(f, src, src_bytes)) {
        fprintf(stderr, "short job file\n");
        return 1;
    }
    fclose(f);

    const size_t n = grams.size();
    Record* recs = (Record*)malloc(n ? n * sizeof(Record) : 1);
    Key* keys = (Key*)malloc(n ? n * sizeof(Key) : 1);
    PacketRow* rows = (PacketRow*)malloc(n ? n * sizeof(PacketRow) : 1);
    memset(rows, 0xa5, n * sizeof(PacketRow));                        // (every row must be written)
    std::vector<StreamResult> results(streams.size());
    for (size_t k = 0; k < n; k++) parse(src + grams[k].src_offset, grams[k].bytes, grams[k].port, &recs[k], &keys[k]);
    for (size_t i = 0; i < streams.size(); i++) {
        const Stream& s = streams[i];
        uint64_t* slots = (uint64_t*)malloc(kSlots * sizeof(uint64_t));
        memset(slots, 0xff, kSlots * sizeof(uint64_t));               // (an index that was never written would leave the records)
        sequence(s, keys + s.first_datagram, recs + s.first_datagram, slots, &results[i]);
        free(slots);
        for (uint32_t j = 0; j < s.n_datagrams; j++)
            table_row(grams[s.first_datagram + j], recs[s.first_datagram + j], j, results[i].n_output, rows + s.first_datagram);
    }

    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    fwrite(recs, sizeof(Record), n, f);
    fwrite(results.data(), sizeof(StreamResult), results.size(), f);
    fwrite(rows, sizeof(PacketRow), n, f);
    fclose(f);
    free(src); free(recs); free(keys); free(rows);
    return 0;
}
