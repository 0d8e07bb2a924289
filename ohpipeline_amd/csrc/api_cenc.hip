// api_cenc.hip -- the C ABI's protected fragmented MPEG-4 layer (ohgpu_cenc_*): the validation of the descriptors, the
// key schedules (made here, on the host), the batch's life around csrc/cenc_kernel.hip's launches, the results and the three tables, the
// host-buffer call, the head of a stream on the host, and the two calls that put the FLAC and the Apple Lossless decoder behind it.
#include <algorithm>
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

int cenc_fetch(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, int table, void* out, size_t n_rows)
{
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchCenc, "a protected MPEG-4"));
    const CencState& g = *batch->cenc;
    return fetch_table(who, g, "rows, the batch's table has", "", n_rows, table == 0 ? g.n_runs : g.n_packets, g.n_streams, out,
                       table == 0 ? g.d_runs : table == 1 ? g.d_rows : g.d_samples, table == 0 ? sizeof(ohgpu_mp4f_run) : 16u);
}

// what ohgpu_cenc_process_host and the two decoder calls fetch after a run; any pointer may be null
int cenc_fetch_all(ohgpu_ctx* ctx, const ohgpu_batch* b, size_t n, size_t n_packets, size_t n_runs, ohgpu_cenc_stream_result* results, ohgpu_mp4f_run* runs,
                   ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    int e = OHGPU_OK;
    if (results) e = ohgpu_cenc_batch_results(ctx, b, n ? results : nullptr, n);
    if (e == OHGPU_OK && runs) e = ohgpu_cenc_batch_runs(ctx, b, n_runs ? runs : nullptr, n_runs);
    if (e == OHGPU_OK && packets) e = ohgpu_cenc_batch_packets(ctx, b, n_packets ? packets : nullptr, n_packets);
    if (e == OHGPU_OK && samples) e = ohgpu_cenc_batch_samples(ctx, b, n_packets ? samples : nullptr, n_packets);
    return e;
}

}  // namespace

extern "C" {

int ohgpu_cenc_batch_check(const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_cenc_batch_check: null argument");
    if (n > 0x00ffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_cenc_batch_check: too many descriptors");
    std::vector<ohgpu_mp4f_stream_desc> plain(n);
    for (size_t i = 0; i < n; i++) {
        const ohgpu_cenc_stream_desc& d = descs[i];
        for (uint32_t r : d.reserved2) if (r) return set_error(OHGPU_ERR_INVALID, "cenc desc %zu: reserved words must be zero", i);
        if (d.flags != OHGPU_MP4F_GATHER) return set_error(OHGPU_ERR_INVALID, "cenc desc %zu: flags 0x%x where the family always gathers (OHGPU_MP4F_GATHER)", i, d.flags);
        if (d.key_flags & ~OHGPU_CENC_HAVE_KEY) return set_error(OHGPU_ERR_INVALID, "cenc desc %zu: unknown key_flags 0x%x", i, d.key_flags);
        memcpy(&plain[i], &d, sizeof(plain[i]));
    }
    return ohgpu_mp4f_batch_check(plain.data(), n, n_packets, n_runs, src_arena_bytes, dst_arena_bytes);       // (the fields the two families share)
}

int ohgpu_cenc_batch_create(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_cenc_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_cenc_batch_create", kBatchCenc, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_cenc_batch_check(descs, n, n_packets, n_runs, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->cenc = new (std::nothrow) CencState();
    if (!b->cenc) return set_error(OHGPU_ERR_NOMEM, "ohgpu_cenc_batch_create: out of host memory");
    CencState& g = *b->cenc;
    g.n_streams = n; g.n_packets = n_packets; g.n_runs = n_runs;
    g.plain = ctx->variant == 1;
    g.keys.assign(n * cenc::kScheduleWords, 0u);
    for (size_t i = 0; i < n; i++) {
        b->src_bytes_touched += descs[i].src_bytes;
        if (descs[i].dst_capacity) g.gathers = true;
        if (descs[i].key_flags & OHGPU_CENC_HAVE_KEY) raopcore::expand_encrypt_key(descs[i].key, &g.keys[i * cenc::kScheduleWords], raop_tables());
    }
    err = cenc_plan(ctx, b.get(), (const cenc::Stream*)descs);
    return batch_done(err, b, out);
}

int ohgpu_cenc_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool mine = batch && batch->kind == kBatchCenc;
    const int go = run_guard(ctx, "ohgpu_cenc_batch_run", batch, kBatchCenc, mine && batch->cenc->n_streams == 0, true, src_base, dst_base, mine && batch->cenc->gathers);
    if (go <= 0) return go;
    return cenc_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_cenc_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_cenc_stream_result* results, size_t n)
{
    const char* const who = "ohgpu_cenc_batch_results";
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchCenc, "a protected MPEG-4"));
    const CencState& g = *batch->cenc;
    // the shared launches keep the sibling's results; what the protection boxes gave lies in an array of its own: joined here
    std::vector<mp4frag::Result> head(n);
    std::vector<cenc::Extra> tail(n);
    OHGPU_TRY(fetch_results(who, g, n, g.n_streams, results ? (void*)head.data() : nullptr, g.d_results, sizeof(head[0])));
    OHGPU_TRY(fetch_results(who, g, n, g.n_streams, results ? (void*)tail.data() : nullptr, g.d_extras, sizeof(tail[0])));
    for (size_t i = 0; i < n; i++) {
        memcpy(&results[i].mp4f, &head[i], sizeof(head[i]));
        memcpy(&results[i].entry, &tail[i], sizeof(tail[i]));
    }
    return OHGPU_OK;
}

int ohgpu_cenc_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs)
{
    return cenc_fetch(ctx, "ohgpu_cenc_batch_runs", batch, 0, runs, n_runs);
}

int ohgpu_cenc_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets)
{
    return cenc_fetch(ctx, "ohgpu_cenc_batch_packets", batch, 1, packets, n_packets);
}

int ohgpu_cenc_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets)
{
    return cenc_fetch(ctx, "ohgpu_cenc_batch_samples", batch, 2, samples, n_packets);
}

int ohgpu_cenc_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6])
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_cenc_batch_phase_ms", batch, kBatchCenc, "a protected MPEG-4"));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_cenc_batch_phase_ms: bad argument");
    const CencState& g = *batch->cenc;
    const int err = phase_ms("ohgpu_cenc_batch_phase_ms", g.ran, g.ev, 6, ms);
    if (err == OHGPU_OK && g.plain) ms[1] = ms[2] = ms[3] = ms[4] = ms[5] = 0.0f;      // (one launch: what lies between the later events is no phase)
    return err;
}

int ohgpu_cenc_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks)
{
    if (!batch || batch->kind != kBatchCenc || !route) return set_error(OHGPU_ERR_INVALID, "ohgpu_cenc_batch_paths: not a protected MPEG-4 batch, or a null argument");
    *route = batch->cenc->plain ? OHGPU_MP4F_ROUTE_PLAIN : OHGPU_MP4F_ROUTE_PHASES;
    if (tiles) *tiles = batch->cenc->n_tiles;
    if (wave_blocks) *wave_blocks = batch->cenc->plain ? 0u : batch->cenc->crypt_blocks;      // (the launch that carries the bytes; the run sums' is the sibling's rule)
    return OHGPU_OK;
}

int ohgpu_cenc_head(const void* bytes, size_t n, ohgpu_cenc_stream_result* result)
{
    if ((n && !bytes) || !result) return set_error(OHGPU_ERR_INVALID, "ohgpu_cenc_head: null argument");
    if (n >= 0x80000000ull) return set_error(OHGPU_ERR_INVALID, "ohgpu_cenc_head: %zu bytes are 2^31 or more", n);
    cenc::Stream s = {};
    s.s.src_bytes = (uint32_t)n;
    s.s.codecs = OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC;
    mp4frag::Rec rec;
    cenc::Result* const r = (cenc::Result*)result;
    cenc::walk(s, (const uint8_t*)bytes, true, &r->r, &r->x, &rec, nullptr);
    return OHGPU_OK;
}

int ohgpu_cenc_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, const void* src_host, uint64_t src_bytes,
                            void* dst_host, uint64_t dst_bytes, ohgpu_cenc_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    const char* const who = "ohgpu_cenc_process_host";
    std::vector<ohgpu_cenc_stream_result> res(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_cenc_batch_create(ctx, descs, n, n_packets, n_runs, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            const int e = ohgpu_cenc_batch_run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : cenc_fetch_all(ctx, b, n, n_packets, n_runs, res.data(), runs, packets, samples);
        },
        [&] {   // only what was gathered comes back
            for (size_t i = 0; i < n; i++) {
                if (!res[i].mp4f.bytes_gathered) continue;
                const int e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, 1, 0, res[i].mp4f.bytes_gathered);
                if (e != OHGPU_OK) return e;
            }
            return (int)OHGPU_OK;
        });
    if (err == OHGPU_OK && results && n) memcpy(results, res.data(), n * sizeof(res[0]));
    return err;
}

int ohgpu_cenc_flac_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* cenc_descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cenc_stream_result* cenc_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    // the sibling's fused call (api_common.h has the one body): this family's batch writes the CLEAR runs into the middle arena
    return frag_flac_process_host(ctx, "ohgpu_cenc_flac_process_host", cenc_descs, flac_descs, n, src_host, src_bytes, mid_bytes, dst_host, dst_bytes, cenc_results, flac_results,
        frames, frames_capacity, n_frames,
        [&](ohgpu_batch** b) { return ohgpu_cenc_batch_create(ctx, cenc_descs, n, n_packets, n_runs, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_mid, ohgpu_cenc_stream_result* res) {
            const int e = ohgpu_cenc_batch_run(ctx, b, d_src, d_mid, nullptr);
            return e != OHGPU_OK ? e : cenc_fetch_all(ctx, b, n, n_packets, n_runs, res, runs, packets, samples);
        },
        [](const ohgpu_cenc_stream_result& r) -> const ohgpu_mp4f_stream_result& { return r.mp4f; });
}

int ohgpu_cenc_alac_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* cenc_descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cenc_stream_result* cenc_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    // the protected families' fused call (api_common.h has the one body): this family's batch writes the CLEAR packets into the middle arena
    return frag_alac_process_host(ctx, "ohgpu_cenc_alac_process_host", cenc_descs, alac_descs, n, n_packets, src_host, src_bytes, mid_bytes, dst_host, dst_bytes, cenc_results,
        packets, alac_results, packet_results,
        [&](ohgpu_batch** b) { return ohgpu_cenc_batch_create(ctx, cenc_descs, n, n_packets, n_runs, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_mid, ohgpu_cenc_stream_result* res, ohgpu_alac_packet* table) {
            const int e = ohgpu_cenc_batch_run(ctx, b, d_src, d_mid, nullptr);
            return e != OHGPU_OK ? e : cenc_fetch_all(ctx, b, n, n_packets, n_runs, res, runs, table, samples);
        },
        [](const ohgpu_cenc_stream_result& r) -> const ohgpu_mp4f_stream_result& { return r.mp4f; });
}

}  // extern "C"
