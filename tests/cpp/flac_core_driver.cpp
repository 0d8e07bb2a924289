// flac_core_driver.cpp -- csrc/flac_frame_core.h on the CPU: scan, probe, chain and restore over a file of cases, the way
// csrc/flac_frame_kernel.hip runs them on the device, both routes.  tests/test_flac_core_cpu.py builds this with
// -fsanitize=address,undefined and holds the results and the whole destination arena against tests/flac_textbook.py.
// Every buffer is allocated at exactly its declared size, so that a load or a store outside a range is a sanitizer report.
//
// in:  u32 n, then per case { u32 src_bytes, channels, bits, rate, blocksize, max_blocksize, max_samples, flags; u64 first_sample;
//      src_bytes of stream }
// out: per case { Result (48 bytes); u32 arena_bytes; arena }
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flac_frame_core.h"

using namespace flaccore;

static void fill_pattern(std::vector<uint8_t>& a)
{
    for (size_t i = 0; i < a.size(); i++) a[i] = (uint8_t)((i * 37u + 11u) & 0xffu);
}

struct CaseHead { uint32_t src_bytes, channels, bits, rate, blocksize, max_blocksize, max_samples, flags; uint64_t first_sample; };

static void store_frame(const Stream& s, const Probe& c, const int32_t* rows, uint32_t row_words, uint8_t* dst)
{
    for (uint32_t i = 0; i < c.blocksize; i++) {
        const uint64_t index = (uint64_t)c.place + i;
        if (c.assignment >= 8) {
            int32_t l, r;
            decorrelate(c.assignment, rows[i], rows[row_words + i], &l, &r);
            store_sample(s, dst, index, 0, l);
            store_sample(s, dst, index, 1, r);
        } else {
            for (uint32_t ch = 0; ch < s.channels; ch++) store_sample(s, dst, index, ch, rows[(size_t)ch * row_words + i]);
        }
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    Tables tables;
    make_tables(&tables);
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, in) != 1) return 2;
    for (uint32_t k = 0; k < n_cases; k++) {
        CaseHead h;
        if (fread(&h, sizeof(h), 1, in) != 1) return 2;
        uint8_t* src = (uint8_t*)malloc(h.src_bytes ? h.src_bytes : 1);          // exactly the range
        if (h.src_bytes && fread(src, 1, h.src_bytes, in) != h.src_bytes) return 2;
        Stream s;
        memset(&s, 0, sizeof(s));
        s.src_bytes = h.src_bytes; s.max_samples = h.max_samples; s.sample_rate = h.rate; s.blocksize = h.blocksize;
        s.max_blocksize = h.max_blocksize; s.channels = (uint8_t)h.channels; s.bits = (uint8_t)h.bits; s.flags = (uint8_t)h.flags;
        s.first_sample = h.first_sample;
        s.dst_plane_stride = (s.flags & kFlagPackedBe) ? 0 : (uint64_t)h.max_samples * 4u;
        const size_t arena_bytes = (s.flags & kFlagPackedBe) ? (size_t)h.max_samples * h.channels * (h.bits / 8u) : (size_t)h.max_samples * 4u * h.channels;
        const StreamCfg cfg = cfg_of(s);
        // scan: every position, in order (the device sorts its list into this order)
        std::vector<Probe> probes;
        for (uint32_t pos = 0; pos < h.src_bytes; pos++) {
            if (scan_position(src + pos, h.src_bytes - pos, &tables, cfg) == kParseBad) continue;
            Probe c;
            memset(&c, 0, sizeof(c));
            c.pos = pos;
            c.row0 = (uint32_t)(probes.size() * h.channels);
            probes.push_back(c);
        }
        std::vector<uint8_t> arenas[2];
        Result results[2];
        for (int plain = 0; plain < 2; plain++) {
            const uint32_t row_words = h.max_blocksize;
            std::vector<Sub> subs(probes.size() * h.channels);
            std::vector<int32_t*> rows(probes.size());
            for (size_t i = 0; i < probes.size(); i++) rows[i] = (int32_t*)malloc((size_t)row_words * h.channels * 4u);   // a candidate's own, exactly
            std::vector<Probe> pr = probes;
            for (size_t i = 0; i < pr.size(); i++) {
                Probe& c = pr[i];
                Header hd;
                memset(&hd, 0, sizeof(hd));
                uint32_t len = 0;
                const int st = plain ? parse_frame<false>(src + c.pos, h.src_bytes - c.pos, &tables, cfg, &hd, nullptr, nullptr, row_words, &len)
                                     : parse_frame<true>(src + c.pos, h.src_bytes - c.pos, &tables, cfg, &hd, subs.data() + c.row0, rows[i], row_words, &len);
                c.state = (uint32_t)st;
                c.end = st == kParseOk ? c.pos + len : (st == kParseShort && scan_position(src + c.pos, h.src_bytes - c.pos, &tables, cfg) == kParseOk ? 1u : 0u);
                c.number = hd.number; c.blocksize = hd.blocksize; c.rate = hd.rate;
                c.channels = hd.channels; c.bits = hd.bits; c.assignment = hd.assignment; c.variable = hd.variable;
            }
            s.cand_first = 0; s.cand_count = (uint32_t)pr.size();
            chain_stream(s, pr.data(), (uint32_t)pr.size(), &results[plain]);
            arenas[plain].resize(arena_bytes);
            fill_pattern(arenas[plain]);
            uint8_t* dst = (uint8_t*)malloc(arena_bytes ? arena_bytes : 1);      // exactly the arena
            memcpy(dst, arenas[plain].data(), arena_bytes);
            for (size_t i = 0; i < pr.size(); i++) {
                const Probe& c = pr[i];
                if (!c.accepted) continue;
                if (plain) {
                    Header hd;
                    uint32_t len = 0;
                    if (parse_frame<true>(src + c.pos, h.src_bytes - c.pos, &tables, cfg, &hd, subs.data() + c.row0, rows[i], row_words, &len) != kParseOk) abort();
                }
                for (uint32_t ch = 0; ch < h.channels; ch++) restore_channel(subs[c.row0 + ch], rows[i] + (size_t)ch * row_words, c.blocksize);
                store_frame(s, c, rows[i], row_words, dst);
            }
            memcpy(arenas[plain].data(), dst, arena_bytes);
            free(dst);
            for (int32_t* r : rows) free(r);
        }
        if (memcmp(&results[0], &results[1], sizeof(Result)) != 0 || arenas[0] != arenas[1]) { fprintf(stderr, "case %u: the two routes differ\n", k); return 3; }
        const uint32_t ab = (uint32_t)arena_bytes;
        fwrite(&results[0], sizeof(Result), 1, out);
        fwrite(&ab, 4, 1, out);
        fwrite(arenas[0].data(), 1, arena_bytes, out);
        free(src);
    }
    fclose(in);
    fclose(out);
    return 0;
}
