// ts_core_driver.cpp -- runs csrc/ts_packet_core.h on the CPU the way csrc/ts_packet_kernel.hip runs it on the device, for
// tests/test_ts_core_cpu.py (built with -fsanitize=address,undefined -fno-sanitize-recover=all).
//   ts_core_driver ts JOB OUT     JOB: u64 n_streams, n_pes, src_bytes, dst_bytes; the descriptors (tspkt::Stream); the source arena; the
//                                 destination arena as it is before the run.  OUT: the results, the PES table, the destination arena.
//   ts_core_driver adts JOB OUT   JOB: u64 n_streams, n_frames, src_bytes, 0; the descriptors (adts::Stream); the source arena.
//                                 OUT: the results, the frame table.
// Both routes run.  The plain one is tspkt::demux / adts::walk as they stand.  The other is put together here as the kernels put it
// together: every packet classified on its own, the tables as three minima, the sums in tiles of 256 whose scan starts from nothing
// and meets the carried state afterwards, every piece of the destination gathered on its own; the ADTS map as a bitmap and the chain's
// search 64 words of it at a time.  The two must agree in every byte, or the driver fails.  The arenas and the per-packet lists are
// heap blocks of the exact size, so that a stray index is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ohpipeline_amd/csrc/ts_packet_core.h"

template <typename T>
static bool read_all(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T>
static T* block(size_t n, int fill = 0)
{
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    memset(p, fill, n ? n * sizeof(T) : 1);
    return p;
}

static const uint32_t kTile = 256;

static void ts_by_tiles(const tspkt::Stream& s, const uint8_t* src, uint8_t* dst, tspkt::Pes* table, tspkt::Pkt* pk, uint32_t* run_end, uint32_t* src_at, tspkt::Result* out)
{
    using namespace tspkt;
    const uint8_t* const base = src + s.src_offset;
    const uint32_t np = packets(s);
    for (uint32_t i = np; i-- > 0;) pk[i] = classify(s, base, i);      // (in no particular order)
    Tab t = {kNone, kNone, kNone, s.pmt_pid, s.audio_pid, 0u};
    for (uint32_t i = 0; i < np; i++) {
        if (kind_of(pk[i]) == kCorruptField && i < t.corrupt) t.corrupt = i;
        if (pat_here(s, pk[i]) && i < t.pat) t.pat = i;
    }
    if (t.pat != kNone && t.pat >= t.corrupt) t.pat = kNone;
    if (t.pat != kNone) t.pmt_pid = found_pid(pk[t.pat]);
    Result r = {};
    uint64_t pmt = ~0ull;
    for (uint32_t i = np; i-- > 0;) {
        if (i >= t.corrupt) continue;
        const uint32_t kind = kind_of(pk[i]);
        r.bad_sync += kind == kBadSync; r.tei_packets += kind == kTei; r.scrambled_packets += kind == kScrambled;
        if (!pmt_candidate(s, t, pk[i], i)) continue;
        const Pkt c = with_section(pk[i], base, (uint64_t)i * kPacket, 2u);
        const uint64_t key = ((uint64_t)i << 16) | found_pid(c);
        if (section_ok(c) && key < pmt) pmt = key;
    }
    if (pmt != ~0ull) { t.pmt = (uint32_t)(pmt >> 16); t.audio_pid = (uint32_t)(pmt & 0xffffu); t.first = t.pmt + 1u; }
    Seg carry = seg_start(s);
    uint32_t n_audio = 0, n_rec = 0, deliv = 0;
    int last_cc = -1;
    std::vector<Seg> seg(kTile);
    std::vector<Elem> elem(kTile);
    std::vector<char> aud(kTile), first(kTile), jump(kTile);
    for (uint32_t k0 = 0; k0 < np; k0 += kTile) {
        const uint32_t m = np - k0 < kTile ? np - k0 : kTile;
        uint32_t audio_here = 0;
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t k = k0 + j;
            aud[j] = is_audio(t, pk[k], k);
            first[j] = jump[j] = 0;
            seg[j] = Seg{0u, 0u, 0u};
            if (!aud[j]) continue;
            elem[j] = audio_elem(base, k, pk[k]);
            first[j] = n_audio + audio_here++ == 0u;
            if (paybit_of(pk[k])) {
                jump[j] = last_cc >= 0 && cc_of(pk[k]) != (((uint32_t)last_cc + 1u) & 15u);
                last_cc = (int)cc_of(pk[k]);
            }
            seg[j] = seg_of(s, elem[j], first[j], jump[j]);
        }
        for (uint32_t j = 1; j < m; j++) seg[j] = combine(seg[j - 1], seg[j]);   // the tile's scan knows nothing of the carry
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t k = k0 + j;
            src_at[k] = 0;
            run_end[k] = deliv;
            if (!aud[j]) continue;
            const Seg before = j ? combine(carry, seg[j - 1]) : carry;
            const Elem& e = elem[j];
            if (e.start && (before.bits & kSegRec)) record_tail(s, table, n_rec - 1u, before, true);
            const uint32_t d = delivers(before, e);
            if (makes_record(s, e, first[j])) record_head(s, table, n_rec++, deliv, k, e);
            r.bad_pes_starts += e.start && !e.good; r.cc_jumps += jump[j]; r.dropped_bytes += e.c - d;
            src_at[k] = k * kPacket + off_of(pk[k]) + e.skip;
            deliv += d;
            run_end[k] = deliv;
        }
        carry = combine(carry, seg[m - 1]);
        n_audio += audio_here;
    }
    if (carry.bits & kSegRec) record_tail(s, table, n_rec - 1u, carry, false);
    r.status = (uint8_t)status_of(s, t);
    r.trailing_bytes = (uint8_t)(s.src_bytes % kPacket);
    r.pmt_pid = (uint16_t)t.pmt_pid; r.audio_pid = (uint16_t)t.audio_pid;
    r.packets = np; r.pat_packet = t.pat; r.pmt_packet = t.pmt; r.corrupt_packet = t.corrupt;
    r.audio_packets = n_audio; r.pes_packets = n_rec; r.bytes_delivered = deliv;
    r.pes_open_bytes = open_bytes_at_end(s, carry, n_audio);
    *out = r;
    uint8_t* const run = dst + s.dst_offset;
    for (uint32_t q = piece_count(run, deliv); q-- > 0;) gather_piece(base, run, deliv, run_end, src_at, np, q);
}

static int run_ts(FILE* f, const uint64_t head[4], const char* out_path)
{
    using namespace tspkt;
    std::vector<Stream> streams(head[0]);
    uint8_t* src = block<uint8_t>(head[2]);
    uint8_t* dst = block<uint8_t>(head[3]);
    if (!read_all(f, streams.data(), streams.size()) || !read_all(f, src, head[2]) || !read_all(f, dst, head[3])) { fprintf(stderr, "short job file\n"); return 1; }
    uint8_t* dst2 = block<uint8_t>(head[3]);
    memcpy(dst2, dst, head[3]);
    Pes* table = block<Pes>(head[1]);
    Pes* table2 = block<Pes>(head[1]);
    std::vector<Result> results(streams.size()), results2(streams.size());
    for (size_t i = 0; i < streams.size(); i++) {
        const uint32_t np = packets(streams[i]);
        Pkt* pk = block<Pkt>(np);
        uint32_t* run_end = block<uint32_t>(np, 0xee);
        uint32_t* src_at = block<uint32_t>(np, 0xee);
        demux(streams[i], src, dst, table, pk, run_end, src_at, &results[i]);
        memset(run_end, 0xee, np * sizeof(uint32_t));
        memset(src_at, 0xee, np * sizeof(uint32_t));
        ts_by_tiles(streams[i], src, dst2, table2, pk, run_end, src_at, &results2[i]);
        free(pk); free(run_end); free(src_at);
        if (memcmp(&results[i], &results2[i], sizeof(Result)) != 0) { fprintf(stderr, "stream %zu: the two routes' results differ\n", i); return 1; }
    }
    if (memcmp(dst, dst2, head[3]) != 0 || memcmp(table, table2, head[1] * sizeof(Pes)) != 0) { fprintf(stderr, "the two routes' bytes or records differ\n"); return 1; }
    f = fopen(out_path, "wb");
    if (!f) { perror(out_path); return 1; }
    fwrite(results.data(), sizeof(Result), results.size(), f);
    fwrite(table, sizeof(Pes), head[1], f);
    fwrite(dst, 1, head[3], f);
    fclose(f);
    free(src); free(dst); free(dst2); free(table); free(table2);
    return 0;
}

static void adts_by_map(const adts::Stream& s, const uint8_t* src, adts::Frame* table, adts::Result* out)
{
    using namespace adts;
    const uint8_t* const base = src + s.src_offset;
    const uint32_t n = s.src_bytes, words = (n + 1023u) / 1024u * 32u;
    uint32_t* map = block<uint32_t>(words);
    for (uint32_t p = 0; p < n; p++) {
        Hdr h;
        if (header_at(base, n, p, &h)) map[p >> 5] |= 1u << (p & 31u);
    }
    Result r = {};
    uint32_t start = 0;
    if (s.flags & kRecognise) {
        const uint32_t none = 0xffffffffu;
        uint32_t payload = 0, hit = none;
        for (uint32_t p = kLastStart + 1u; p-- > 0;) if (five_from(base, n, p, &payload)) hit = p;
        if (hit == none) { r.status = kNotAdts; *out = r; free(map); return; }
        five_from(base, n, hit, &payload);
        start = hit;
        Hdr h;
        header_at(base, n, start, &h);
        set_first(&r, start, h);
        r.mean_payload_bytes = payload / kRecogniseFrames;
    }
    auto next = [&](uint32_t p) {
        const uint32_t last = n - 6u;
        while (p < last) {
            for (uint32_t lane = 0; lane < 64u; lane++) {
                const uint32_t w = (p >> 5) + lane;
                uint32_t v = w < words ? map[w] : 0u;
                if (lane == 0) v &= ~0u << (p & 31u);
                if (v) return w * 32u + (uint32_t)__builtin_ctz(v);
            }
            p = ((p >> 5) + 64u) * 32u;
        }
        return last;
    };
    chain_from(s, base, start, table, next, &r);
    *out = r;
    free(map);
}

static int run_adts(FILE* f, const uint64_t head[4], const char* out_path)
{
    using namespace adts;
    std::vector<Stream> streams(head[0]);
    uint8_t* src = block<uint8_t>(head[2]);
    if (!read_all(f, streams.data(), streams.size()) || !read_all(f, src, head[2])) { fprintf(stderr, "short job file\n"); return 1; }
    Frame* table = block<Frame>(head[1]);
    Frame* table2 = block<Frame>(head[1]);
    std::vector<Result> results(streams.size()), results2(streams.size());
    for (size_t i = 0; i < streams.size(); i++) {
        walk(streams[i], src, table, &results[i]);
        adts_by_map(streams[i], src, table2, &results2[i]);
        if (memcmp(&results[i], &results2[i], sizeof(Result)) != 0) { fprintf(stderr, "stream %zu: the two routes' results differ\n", i); return 1; }
    }
    if (memcmp(table, table2, head[1] * sizeof(Frame)) != 0) { fprintf(stderr, "the two routes' frame tables differ\n"); return 1; }
    f = fopen(out_path, "wb");
    if (!f) { perror(out_path); return 1; }
    fwrite(results.data(), sizeof(Result), results.size(), f);
    fwrite(table, sizeof(Frame), head[1], f);
    fclose(f);
    free(src); free(table); free(table2);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s ts|adts JOB OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 1; }
    uint64_t head[4];
    if (!read_all(f, head, 4)) return 1;
    const int err = strcmp(argv[1], "ts") == 0 ? run_ts(f, head, argv[3]) : run_adts(f, head, argv[3]);
    fclose(f);
    return err;
}
