// api_mp4f.hip -- the C ABI's fragmented MPEG-4 layer (ohgpu_mp4f_*): the validation of the descriptors, the batch's
// life around csrc/mp4_frag_kernel.hip's launches, the results and the three tables, the host-buffer call, the head of a stream on the
// host, and the two calls that put the FLAC and the Apple Lossless decoder behind it.
#include <algorithm>
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

int mp4f_check_desc(const ohgpu_mp4f_stream_desc& d, size_t i, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: reserved words must be zero", i);
    if (d.flags & ~OHGPU_MP4F_GATHER) return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: unknown flags 0x%x", i, d.flags);
    if (!d.codecs || (d.codecs & ~(OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC))) return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: codecs 0x%x names no codec, or an unknown one", i, d.codecs);
    if (d.src_bytes >= 0x80000000u) return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: src_bytes %u is 2^31 or more", i, d.src_bytes);
    if (d.packet_capacity && (d.packet_first > n_packets || d.packet_capacity > n_packets - d.packet_first))
        return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: rows [%u, +%u) of tables of %zu", i, d.packet_first, d.packet_capacity, n_packets);
    if (d.run_capacity && (d.run_first > n_runs || d.run_capacity > n_runs - d.run_first))
        return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: runs [%u, +%u) of a table of %zu", i, d.run_first, d.run_capacity, n_runs);
    const int err = arena_span("mp4f desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
    if (err != OHGPU_OK || !(d.flags & OHGPU_MP4F_GATHER)) return err;
    return arena_span("mp4f desc", i, "gathers into", d.dst_offset, d.dst_capacity, dst_arena_bytes, "destination");
}

int mp4f_fetch(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, int table, void* out, size_t n_rows)
{
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchMp4f, "a fragmented MPEG-4"));
    const Mp4fState& g = *batch->mp4f;
    return fetch_table(who, g, "rows, the batch's table has", "", n_rows, table == 0 ? g.n_runs : g.n_packets, g.n_streams, out,
                       table == 0 ? g.d_runs : table == 1 ? g.d_packets : g.d_samples, table == 0 ? sizeof(ohgpu_mp4f_run) : 16u);
}

// what ohgpu_mp4f_process_host and the two decoder calls fetch after a run; any pointer may be null
int mp4f_fetch_all(ohgpu_ctx* ctx, const ohgpu_batch* b, size_t n, size_t n_packets, size_t n_runs, ohgpu_mp4f_stream_result* results, ohgpu_mp4f_run* runs,
                   ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    int e = OHGPU_OK;
    if (results) e = ohgpu_mp4f_batch_results(ctx, b, n ? results : nullptr, n);
    if (e == OHGPU_OK && runs) e = ohgpu_mp4f_batch_runs(ctx, b, n_runs ? runs : nullptr, n_runs);
    if (e == OHGPU_OK && packets) e = ohgpu_mp4f_batch_packets(ctx, b, n_packets ? packets : nullptr, n_packets);
    if (e == OHGPU_OK && samples) e = ohgpu_mp4f_batch_samples(ctx, b, n_packets ? samples : nullptr, n_packets);
    return e;
}

}  // namespace

extern "C" {

int ohgpu_mp4f_batch_check(const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4f_batch_check: null argument");
    if (n > 0x00ffffffull || n_packets > 0x0fffffffull || n_runs > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4f_batch_check: too many descriptors");
    std::vector<std::pair<uint64_t, uint64_t>> rows, runs, gathers;
    for (size_t i = 0; i < n; i++) {
        const int err = mp4f_check_desc(descs[i], i, n_packets, n_runs, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        if (descs[i].packet_capacity) rows.emplace_back(descs[i].packet_first, descs[i].packet_capacity);
        if (descs[i].run_capacity) runs.emplace_back(descs[i].run_first, descs[i].run_capacity);
        if ((descs[i].flags & OHGPU_MP4F_GATHER) && descs[i].dst_capacity) gathers.emplace_back(descs[i].dst_offset, descs[i].dst_capacity);
    }
    int err = ranges_disjoint("ohgpu_mp4f_batch_check", "row", rows);
    if (err == OHGPU_OK) err = ranges_disjoint("ohgpu_mp4f_batch_check", "run", runs);
    if (err == OHGPU_OK) err = ranges_disjoint("ohgpu_mp4f_batch_check", "gather", gathers);
    return err;
}

int ohgpu_mp4f_batch_create(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_mp4f_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_mp4f_batch_create", kBatchMp4f, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_mp4f_batch_check(descs, n, n_packets, n_runs, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->mp4f = new (std::nothrow) Mp4fState();
    if (!b->mp4f) return set_error(OHGPU_ERR_NOMEM, "ohgpu_mp4f_batch_create: out of host memory");
    Mp4fState& g = *b->mp4f;
    g.n_streams = n; g.n_packets = n_packets; g.n_runs = n_runs;
    g.plain = ctx->variant == 1;
    for (size_t i = 0; i < n; i++) {
        b->src_bytes_touched += descs[i].src_bytes;
        if ((descs[i].flags & OHGPU_MP4F_GATHER) && descs[i].dst_capacity) g.gathers = true;
    }
    err = mp4f_plan(ctx, g, (const mp4frag::Stream*)descs, "ohgpu_mp4f_batch_create");
    return batch_done(err, b, out);
}

int ohgpu_mp4f_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool mine = batch && batch->kind == kBatchMp4f;
    const int go = run_guard(ctx, "ohgpu_mp4f_batch_run", batch, kBatchMp4f, mine && batch->mp4f->n_streams == 0, true, src_base, dst_base, mine && batch->mp4f->gathers);
    if (go <= 0) return go;
    return mp4f_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_mp4f_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_stream_result* results, size_t n)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_mp4f_batch_results", batch, kBatchMp4f, "a fragmented MPEG-4"));
    const Mp4fState& g = *batch->mp4f;
    return fetch_results("ohgpu_mp4f_batch_results", g, n, g.n_streams, results, g.d_results, sizeof(*results));
}

int ohgpu_mp4f_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs)
{
    return mp4f_fetch(ctx, "ohgpu_mp4f_batch_runs", batch, 0, runs, n_runs);
}

int ohgpu_mp4f_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets)
{
    return mp4f_fetch(ctx, "ohgpu_mp4f_batch_packets", batch, 1, packets, n_packets);
}

int ohgpu_mp4f_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets)
{
    return mp4f_fetch(ctx, "ohgpu_mp4f_batch_samples", batch, 2, samples, n_packets);
}

int ohgpu_mp4f_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6])
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_mp4f_batch_phase_ms", batch, kBatchMp4f, "a fragmented MPEG-4"));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4f_batch_phase_ms: bad argument");
    const Mp4fState& g = *batch->mp4f;
    const int err = phase_ms("ohgpu_mp4f_batch_phase_ms", g.ran, g.ev, 6, ms);
    if (err == OHGPU_OK && g.plain) ms[1] = ms[2] = ms[3] = ms[4] = ms[5] = 0.0f;      // (one launch: what lies between the later events is no phase)
    return err;
}

int ohgpu_mp4f_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks)
{
    if (!batch || batch->kind != kBatchMp4f || !route) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4f_batch_paths: not a fragmented MPEG-4 batch, or a null argument");
    *route = batch->mp4f->plain ? OHGPU_MP4F_ROUTE_PLAIN : OHGPU_MP4F_ROUTE_PHASES;
    if (tiles) *tiles = batch->mp4f->n_tiles;
    if (wave_blocks) *wave_blocks = batch->mp4f->plain ? 0u : batch->mp4f->wave_blocks;
    return OHGPU_OK;
}

int ohgpu_mp4f_head(const void* bytes, size_t n, ohgpu_mp4f_stream_result* result)
{
    if ((n && !bytes) || !result) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4f_head: null argument");
    if (n >= 0x80000000ull) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4f_head: %zu bytes are 2^31 or more", n);
    mp4frag::Stream s = {};
    s.src_bytes = (uint32_t)n;
    s.codecs = OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC;
    mp4frag::Rec rec;
    mp4frag::walk(s, (const uint8_t*)bytes, true, (mp4frag::Result*)result, &rec, nullptr);
    return OHGPU_OK;
}

int ohgpu_mp4f_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, const void* src_host, uint64_t src_bytes,
                            void* dst_host, uint64_t dst_bytes, ohgpu_mp4f_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    const char* const who = "ohgpu_mp4f_process_host";
    std::vector<ohgpu_mp4f_stream_result> res(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_mp4f_batch_create(ctx, descs, n, n_packets, n_runs, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            const int e = ohgpu_mp4f_batch_run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : mp4f_fetch_all(ctx, b, n, n_packets, n_runs, res.data(), runs, packets, samples);
        },
        [&] {   // only what was gathered comes back
            for (size_t i = 0; i < n; i++) {
                if (!res[i].bytes_gathered) continue;
                const int e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, 1, 0, res[i].bytes_gathered);
                if (e != OHGPU_OK) return e;
            }
            return (int)OHGPU_OK;
        });
    if (err == OHGPU_OK && results && n) memcpy(results, res.data(), n * sizeof(res[0]));
    return err;
}

int ohgpu_mp4f_flac_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* mp4f_descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_mp4f_stream_result* mp4f_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    return frag_flac_process_host(ctx, "ohgpu_mp4f_flac_process_host", mp4f_descs, flac_descs, n, src_host, src_bytes, mid_bytes, dst_host, dst_bytes, mp4f_results, flac_results,
        frames, frames_capacity, n_frames,
        [&](ohgpu_batch** b) { return ohgpu_mp4f_batch_create(ctx, mp4f_descs, n, n_packets, n_runs, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_mid, ohgpu_mp4f_stream_result* res) {
            const int e = ohgpu_mp4f_batch_run(ctx, b, d_src, d_mid, nullptr);
            return e != OHGPU_OK ? e : mp4f_fetch_all(ctx, b, n, n_packets, n_runs, res, runs, packets, samples);   // (the results: the one small read between the layers)
        },
        [](const ohgpu_mp4f_stream_result& r) -> const ohgpu_mp4f_stream_result& { return r; });
}

int ohgpu_mp4f_alac_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* mp4f_descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_mp4f_stream_result* mp4f_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    const char* const who = "ohgpu_mp4f_alac_process_host";
    if (n && (!mp4f_descs || !alac_descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    for (size_t i = 0; i < n; i++)
        if (mp4f_descs[i].flags & OHGPU_MP4F_GATHER) return set_error(OHGPU_ERR_INVALID, "%s: stream %zu gathers: the packets are decoded where they lie", who, i);
    std::vector<ohgpu_mp4f_stream_result> mres(n);
    std::vector<ohgpu_alac_packet> table(n_packets), dense;
    std::vector<ohgpu_alac_stream_desc> adescs(alac_descs, alac_descs + n);
    std::vector<ohgpu_alac_stream_result> ares(n);
    std::vector<ohgpu_alac_packet_result> pres;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_mp4f_batch_create(ctx, mp4f_descs, n, n_packets, n_runs, src_bytes, 0, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            int e = ohgpu_mp4f_batch_run(ctx, b, d_src, nullptr, nullptr);
            if (e == OHGPU_OK) e = mp4f_fetch_all(ctx, b, n, n_packets, n_runs, mres.data(), runs, table.data(), samples);   // the one small read between the layers
            if (e != OHGPU_OK) return e;
            // the Apple Lossless table has the streams' leading accepted rows one after the other without gaps
            for (size_t i = 0; i < n; i++) {
                ohgpu_alac_stream_desc& a = adescs[i];
                const bool ok = mres[i].status == OHGPU_MP4F_OK && mres[i].codec == mp4box::fourcc('a', 'l', 'a', 'c');
                const uint32_t rows = ok ? mres[i].samples_available : 0u;
                // (a stream that brings no packets still stands in the Apple Lossless batch: see ohgpu_mp4_alac_process_host)
                const ohgpu_alac_config none = {1, 0, 16, 0, 0, 1, 1, 0, 0, 0, 0};
                a.config = ok ? mres[i].config : none;
                a.first_packet = (uint32_t)dense.size();
                a.n_packets = rows;
                if (!ok && !a.flags) a.dst_plane_stride = 0;
                dense.insert(dense.end(), table.begin() + mp4f_descs[i].packet_first, table.begin() + mp4f_descs[i].packet_first + rows);
            }
            pres.resize(dense.size());
            if (dense.empty()) return (int)OHGPU_OK;
            ohgpu_batch* ab = nullptr;
            e = ohgpu_alac_batch_create(ctx, adescs.data(), n, dense.data(), dense.size(), src_bytes, dst_bytes, &ab);
            if (e != OHGPU_OK) return e;
            const BatchPtr own(ab, BatchDeleter{ctx});
            e = ohgpu_alac_batch_run(ctx, ab, d_src, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_alac_batch_results(ctx, ab, ares.data(), n, pres.data(), pres.size());
            return e;
        },
        [&] {   // only what was decoded comes back, as in ohgpu_alac_process_host
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (adescs[i].n_packets) e = alac_download_decoded(ctx, who, adescs[i], pres.data() + adescs[i].first_packet, dst_host);
            return e;
        });
    if (err != OHGPU_OK) return err;
    if (mp4f_results && n) memcpy(mp4f_results, mres.data(), n * sizeof(mres[0]));
    if (packets && n_packets) memcpy(packets, table.data(), n_packets * sizeof(table[0]));
    if (alac_results && n) memcpy(alac_results, ares.data(), n * sizeof(ares[0]));
    if (packet_results && n_packets) {
        memset(packet_results, 0, n_packets * sizeof(*packet_results));
        for (size_t i = 0; i < n; i++)
            if (adescs[i].n_packets) memcpy(packet_results + mp4f_descs[i].packet_first, pres.data() + adescs[i].first_packet, adescs[i].n_packets * sizeof(pres[0]));
    }
    return OHGPU_OK;
}

}  // extern "C"
