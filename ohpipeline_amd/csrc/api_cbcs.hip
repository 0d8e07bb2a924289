// api_cbcs.hip -- the C ABI's second protected fragmented MPEG-4 layer (ohgpu_cbcs_*): the validation of the descriptors,
// the key schedules (both of them, made here, on the host), the batch's life around csrc/cbcs_kernel.hip's launches, the results and the
// three tables, the host-buffer call, the head of a stream on the host, and the two calls that put the FLAC and the Apple Lossless
// decoder behind it.  It mirrors csrc/api_cenc.hip function for function.
#include <algorithm>
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

const char* const kNoun = "a cbcs-protected MPEG-4";

int cbcs_fetch(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, int table, void* out, size_t n_rows)
{
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchCbcs, kNoun));
    const CbcsState& g = *batch->cbcs;
    return fetch_table(who, g, "rows, the batch's table has", "", n_rows, table == 0 ? g.n_runs : g.n_packets, g.n_streams, out,
                       table == 0 ? g.d_runs : table == 1 ? g.d_rows : g.d_samples, table == 0 ? sizeof(ohgpu_mp4f_run) : 16u);
}

// what ohgpu_cbcs_process_host and the two decoder calls fetch after a run; any pointer may be null
int cbcs_fetch_all(ohgpu_ctx* ctx, const ohgpu_batch* b, size_t n, size_t n_packets, size_t n_runs, ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs,
                   ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    int e = OHGPU_OK;
    if (results) e = ohgpu_cbcs_batch_results(ctx, b, n ? results : nullptr, n);
    if (e == OHGPU_OK && runs) e = ohgpu_cbcs_batch_runs(ctx, b, n_runs ? runs : nullptr, n_runs);
    if (e == OHGPU_OK && packets) e = ohgpu_cbcs_batch_packets(ctx, b, n_packets ? packets : nullptr, n_packets);
    if (e == OHGPU_OK && samples) e = ohgpu_cbcs_batch_samples(ctx, b, n_packets ? samples : nullptr, n_packets);
    return e;
}

const ohgpu_mp4f_stream_result& head_of(const ohgpu_cbcs_stream_result& r) { return r.cenc.mp4f; }

}  // namespace

extern "C" {

int ohgpu_cbcs_batch_check(const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, uint64_t src_arena_bytes,
                           uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_batch_check: null argument");
    if (n > 0x00ffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_batch_check: too many descriptors");
    if (n_subsamples > 0xffffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_batch_check: %zu subsample rows are more than one batch takes", n_subsamples);
    std::vector<ohgpu_mp4f_stream_desc> plain(n);
    std::vector<std::pair<uint64_t, uint64_t>> shares;
    for (size_t i = 0; i < n; i++) {
        const ohgpu_cbcs_stream_desc& d = descs[i];
        // (ohgpu_cenc_batch_check's three rules, under this family's name)
        for (uint32_t r : d.reserved2) if (r) return set_error(OHGPU_ERR_INVALID, "cbcs desc %zu: reserved words must be zero", i);
        if (d.flags != OHGPU_MP4F_GATHER) return set_error(OHGPU_ERR_INVALID, "cbcs desc %zu: flags 0x%x where the family always gathers (OHGPU_MP4F_GATHER)", i, d.flags);
        if (d.key_flags & ~OHGPU_CENC_HAVE_KEY) return set_error(OHGPU_ERR_INVALID, "cbcs desc %zu: unknown key_flags 0x%x", i, d.key_flags);
        if ((uint64_t)d.subsample_first + d.subsample_capacity > n_subsamples)
            return set_error(OHGPU_ERR_INVALID, "cbcs desc %zu: subsample rows [%u, +%u) beyond the table's %zu", i, d.subsample_first, d.subsample_capacity, n_subsamples);
        if (d.subsample_capacity) shares.emplace_back(d.subsample_first, d.subsample_capacity);
        memcpy(&plain[i], &d, sizeof(plain[i]));
    }
    OHGPU_TRY(ohgpu_mp4f_batch_check(plain.data(), n, n_packets, n_runs, src_arena_bytes, dst_arena_bytes));       // (the fields the fragmented families share)
    return ranges_disjoint("ohgpu_cbcs_batch_check", "subsample", shares);
}

int ohgpu_cbcs_batch_create(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_cbcs_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_cbcs_batch_create", kBatchCbcs, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_cbcs_batch_check(descs, n, n_packets, n_runs, n_subsamples, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->cbcs = new (std::nothrow) CbcsState();
    if (!b->cbcs) return set_error(OHGPU_ERR_NOMEM, "ohgpu_cbcs_batch_create: out of host memory");
    CbcsState& g = *b->cbcs;
    g.n_streams = n; g.n_packets = n_packets; g.n_runs = n_runs; g.n_subsamples = n_subsamples;
    g.plain = ctx->variant == 1;
    g.keys.assign(n * cbcs::kKeyWords, 0u);
    for (size_t i = 0; i < n; i++) {
        b->src_bytes_touched += descs[i].src_bytes;
        if (descs[i].dst_capacity) g.gathers = true;
        if (!(descs[i].key_flags & OHGPU_CENC_HAVE_KEY)) continue;
        // the scheme is the stream's to say: the cipher's schedule for `cenc`, the inverse cipher's for `cbcs`
        raopcore::expand_encrypt_key(descs[i].key, &g.keys[i * cbcs::kKeyWords], raop_tables());
        raopcore::expand_decrypt_key(descs[i].key, &g.keys[i * cbcs::kKeyWords + raopcore::kRoundKeyWords], raop_tables());
    }
    err = cbcs_plan(ctx, b.get(), (const cbcs::Stream*)descs);
    return batch_done(err, b, out);
}

int ohgpu_cbcs_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool mine = batch && batch->kind == kBatchCbcs;
    const int go = run_guard(ctx, "ohgpu_cbcs_batch_run", batch, kBatchCbcs, mine && batch->cbcs->n_streams == 0, true, src_base, dst_base, mine && batch->cbcs->gathers);
    if (go <= 0) return go;
    return cbcs_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_cbcs_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_cbcs_stream_result* results, size_t n)
{
    const char* const who = "ohgpu_cbcs_batch_results";
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchCbcs, kNoun));
    const CbcsState& g = *batch->cbcs;
    // the shared launches keep the sibling's results; what the protection boxes gave lies in two arrays of its own: joined here
    std::vector<mp4frag::Result> head(n);
    std::vector<cenc::Extra> tail(n);
    std::vector<cbcs::More> more(n);
    OHGPU_TRY(fetch_results(who, g, n, g.n_streams, results ? (void*)head.data() : nullptr, g.d_results, sizeof(head[0])));
    OHGPU_TRY(fetch_results(who, g, n, g.n_streams, results ? (void*)tail.data() : nullptr, g.d_extras, sizeof(tail[0])));
    OHGPU_TRY(fetch_results(who, g, n, g.n_streams, results ? (void*)more.data() : nullptr, g.d_more, sizeof(more[0])));
    for (size_t i = 0; i < n; i++) {
        memcpy(&results[i].cenc.mp4f, &head[i], sizeof(head[i]));
        memcpy(&results[i].cenc.entry, &tail[i], sizeof(tail[i]));
        memcpy(&results[i].crypt_blocks, &more[i], sizeof(more[i]));
    }
    return OHGPU_OK;
}

int ohgpu_cbcs_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs)
{
    return cbcs_fetch(ctx, "ohgpu_cbcs_batch_runs", batch, 0, runs, n_runs);
}

int ohgpu_cbcs_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets)
{
    return cbcs_fetch(ctx, "ohgpu_cbcs_batch_packets", batch, 1, packets, n_packets);
}

int ohgpu_cbcs_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets)
{
    return cbcs_fetch(ctx, "ohgpu_cbcs_batch_samples", batch, 2, samples, n_packets);
}

int ohgpu_cbcs_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6])
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_cbcs_batch_phase_ms", batch, kBatchCbcs, kNoun));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_batch_phase_ms: bad argument");
    const CbcsState& g = *batch->cbcs;
    const int err = phase_ms("ohgpu_cbcs_batch_phase_ms", g.ran, g.ev, 6, ms);
    if (err == OHGPU_OK && g.plain) ms[1] = ms[2] = ms[3] = ms[4] = ms[5] = 0.0f;      // (one launch: what lies between the later events is no phase)
    return err;
}

int ohgpu_cbcs_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks)
{
    if (!batch || batch->kind != kBatchCbcs || !route) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_batch_paths: not a cbcs-protected MPEG-4 batch, or a null argument");
    *route = batch->cbcs->plain ? OHGPU_MP4F_ROUTE_PLAIN : OHGPU_MP4F_ROUTE_PHASES;
    if (tiles) *tiles = batch->cbcs->n_tiles;
    if (wave_blocks) *wave_blocks = batch->cbcs->plain ? 0u : batch->cbcs->crypt_blocks;
    return OHGPU_OK;
}

int ohgpu_cbcs_head(const void* bytes, size_t n, ohgpu_cbcs_stream_result* result)
{
    if ((n && !bytes) || !result) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_head: null argument");
    if (n >= 0x80000000ull) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_head: %zu bytes are 2^31 or more", n);
    cbcs::Stream s = {};
    s.c.s.src_bytes = (uint32_t)n;
    s.c.s.codecs = OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC;
    mp4frag::Rec rec;
    uint32_t rows_cap;
    cbcs::Result* const r = (cbcs::Result*)result;
    cbcs::walk(s, (const uint8_t*)bytes, true, nullptr, nullptr, &r->c.r, &r->c.x, &r->m, &rec, nullptr, &rows_cap);
    return OHGPU_OK;
}

int ohgpu_cbcs_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, const void* src_host,
                            uint64_t src_bytes, void* dst_host, uint64_t dst_bytes, ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets,
                            ohgpu_mp4_sample* samples)
{
    const char* const who = "ohgpu_cbcs_process_host";
    std::vector<ohgpu_cbcs_stream_result> res(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_cbcs_batch_create(ctx, descs, n, n_packets, n_runs, n_subsamples, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            const int e = ohgpu_cbcs_batch_run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : cbcs_fetch_all(ctx, b, n, n_packets, n_runs, res.data(), runs, packets, samples);
        },
        [&] {   // only what was gathered comes back
            for (size_t i = 0; i < n; i++) {
                if (!head_of(res[i]).bytes_gathered) continue;
                const int e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, 1, 0, head_of(res[i]).bytes_gathered);
                if (e != OHGPU_OK) return e;
            }
            return (int)OHGPU_OK;
        });
    if (err == OHGPU_OK && results && n) memcpy(results, res.data(), n * sizeof(res[0]));
    return err;
}

int ohgpu_cbcs_flac_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 size_t n_subsamples, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    // the fragmented families' fused call (api_common.h has the one body): this family's batch writes the CLEAR runs into the middle arena
    return frag_flac_process_host(ctx, "ohgpu_cbcs_flac_process_host", descs, flac_descs, n, src_host, src_bytes, mid_bytes, dst_host, dst_bytes, results, flac_results,
        frames, frames_capacity, n_frames,
        [&](ohgpu_batch** b) { return ohgpu_cbcs_batch_create(ctx, descs, n, n_packets, n_runs, n_subsamples, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_mid, ohgpu_cbcs_stream_result* res) {
            const int e = ohgpu_cbcs_batch_run(ctx, b, d_src, d_mid, nullptr);
            return e != OHGPU_OK ? e : cbcs_fetch_all(ctx, b, n, n_packets, n_runs, res, runs, packets, samples);
        },
        head_of);
}

int ohgpu_cbcs_alac_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 size_t n_subsamples, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    return frag_alac_process_host(ctx, "ohgpu_cbcs_alac_process_host", descs, alac_descs, n, n_packets, src_host, src_bytes, mid_bytes, dst_host, dst_bytes, results, packets,
        alac_results, packet_results,
        [&](ohgpu_batch** b) { return ohgpu_cbcs_batch_create(ctx, descs, n, n_packets, n_runs, n_subsamples, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_mid, ohgpu_cbcs_stream_result* res, ohgpu_alac_packet* table) {
            const int e = ohgpu_cbcs_batch_run(ctx, b, d_src, d_mid, nullptr);
            return e != OHGPU_OK ? e : cbcs_fetch_all(ctx, b, n, n_packets, n_runs, res, runs, table, samples);
        },
        head_of);
}

}  // extern "C"
