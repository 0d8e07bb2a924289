// api_mp4.hip -- the C ABI's MPEG-4 container layer (ohgpu_mp4_*): the validation of the descriptors, the batch's life
// around csrc/mp4_table_kernel.hip's launches, the results and both tables, the host-buffer call, the seek, and the call that puts
// the Apple Lossless decoder behind it.
#include <algorithm>
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

int mp4_check_desc(const ohgpu_mp4_stream_desc& d, size_t i, size_t n_packets, uint64_t src_arena_bytes)
{
    for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "mp4 desc %zu: reserved words must be zero", i);
    if (d.flags) return set_error(OHGPU_ERR_INVALID, "mp4 desc %zu: unknown flags 0x%x", i, d.flags);
    if (d.src_bytes >= 0x80000000u) return set_error(OHGPU_ERR_INVALID, "mp4 desc %zu: src_bytes %u is 2^31 or more", i, d.src_bytes);
    if (d.packet_capacity && (d.packet_first > n_packets || d.packet_capacity > n_packets - d.packet_first))
        return set_error(OHGPU_ERR_INVALID, "mp4 desc %zu: rows [%u, +%u) of tables of %zu", i, d.packet_first, d.packet_capacity, n_packets);
    return arena_span("mp4 desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
}

int mp4_fetch(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, bool samples, void* out, size_t n_packets)
{
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchMp4, "an MPEG-4"));
    const Mp4State& g = *batch->mp4;
    return fetch_table(who, g, "rows, the batch's tables have", "", n_packets, g.n_packets, g.n_streams, out, samples ? g.d_samples : g.d_packets, 16u);
}

}  // namespace

extern "C" {

int ohgpu_mp4_batch_check(const ohgpu_mp4_stream_desc* descs, size_t n, size_t n_packets, uint64_t src_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4_batch_check: null argument");
    if (n > 0x00ffffffull || n_packets > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4_batch_check: too many descriptors");
    std::vector<std::pair<uint64_t, uint64_t>> ranges;                 // (first, capacity) of the streams that have rows
    for (size_t i = 0; i < n; i++) {
        const int err = mp4_check_desc(descs[i], i, n_packets, src_arena_bytes);
        if (err != OHGPU_OK) return err;
        if (descs[i].packet_capacity) ranges.emplace_back(descs[i].packet_first, descs[i].packet_capacity);
    }
    return ranges_disjoint("ohgpu_mp4_batch_check", "row", ranges);
}

int ohgpu_mp4_batch_create(ohgpu_ctx* ctx, const ohgpu_mp4_stream_desc* descs, size_t n, size_t n_packets, uint64_t src_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_mp4_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_mp4_batch_create", kBatchMp4, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, 0, out, &b);
    if (err == OHGPU_OK) err = ohgpu_mp4_batch_check(descs, n, n_packets, src_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->mp4 = new (std::nothrow) Mp4State();
    if (!b->mp4) return set_error(OHGPU_ERR_NOMEM, "ohgpu_mp4_batch_create: out of host memory");
    b->mp4->n_streams = n;
    b->mp4->n_packets = n_packets;
    b->mp4->plain = ctx->variant == 1;
    for (size_t i = 0; i < n; i++) b->src_bytes_touched += descs[i].src_bytes;
    err = mp4_plan(ctx, b.get(), (const mp4box::Stream*)descs);
    return batch_done(err, b, out);
}

int ohgpu_mp4_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* stream)
{
    const bool empty = batch && batch->kind == kBatchMp4 && batch->mp4->n_streams == 0;
    const int go = run_guard(ctx, "ohgpu_mp4_batch_run", batch, kBatchMp4, empty, true, src_base, nullptr, false);
    if (go <= 0) return go;
    return mp4_run(ctx, batch, (const uint8_t*)src_base, pick_stream(ctx, stream));
}

int ohgpu_mp4_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_stream_result* results, size_t n)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_mp4_batch_results", batch, kBatchMp4, "an MPEG-4"));
    const Mp4State& g = *batch->mp4;
    return fetch_results("ohgpu_mp4_batch_results", g, n, g.n_streams, results, g.d_results, sizeof(*results));
}

int ohgpu_mp4_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets)
{
    return mp4_fetch(ctx, "ohgpu_mp4_batch_packets", batch, false, packets, n_packets);
}

int ohgpu_mp4_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets)
{
    return mp4_fetch(ctx, "ohgpu_mp4_batch_samples", batch, true, samples, n_packets);
}

int ohgpu_mp4_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4])
{
    CTX_GUARD("ohgpu_mp4_batch_phase_ms");
    if (!batch || batch->kind != kBatchMp4 || !ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4_batch_phase_ms: bad argument");
    const int err = phase_ms("ohgpu_mp4_batch_phase_ms", batch->mp4->ran, batch->mp4->ev, 4, ms);
    if (err == OHGPU_OK && batch->mp4->plain) ms[1] = ms[2] = ms[3] = 0.0f;      // (one launch: what lies between the later events is no phase)
    return err;
}

int ohgpu_mp4_seek(const ohgpu_mp4_sample* samples, size_t n, uint64_t frame, uint64_t* index, uint64_t* first_frame)
{
    if ((n && !samples) || !index || !first_frame) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4_seek: null argument");
    uint64_t at = 0;
    if (!mp4box::seek((const mp4box::Sample*)samples, n, frame, &at))
        return set_error(OHGPU_ERR_BOUNDS, "ohgpu_mp4_seek: frame %llu lies behind the table's %zu rows", (unsigned long long)frame, n);
    *index = at;
    *first_frame = samples[at].first_frame;
    return OHGPU_OK;
}

int ohgpu_mp4_process_host(ohgpu_ctx* ctx, const ohgpu_mp4_stream_desc* descs, size_t n, size_t n_packets, const void* src_host, uint64_t src_bytes,
                           ohgpu_mp4_stream_result* results, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    const char* const who = "ohgpu_mp4_process_host";
    return decoder_process_host(ctx, who, src_host, src_bytes, nullptr, 0,
        [&](ohgpu_batch** b) { return ohgpu_mp4_batch_create(ctx, descs, n, n_packets, src_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void*) {
            int e = ohgpu_mp4_batch_run(ctx, b, d_src, nullptr);
            if (e == OHGPU_OK && results) e = ohgpu_mp4_batch_results(ctx, b, n ? results : nullptr, n);
            if (e == OHGPU_OK && packets) e = ohgpu_mp4_batch_packets(ctx, b, n_packets ? packets : nullptr, n_packets);
            if (e == OHGPU_OK && samples) e = ohgpu_mp4_batch_samples(ctx, b, n_packets ? samples : nullptr, n_packets);
            return e;
        },
        [] { return (int)OHGPU_OK; });
}

int ohgpu_mp4_alac_process_host(ohgpu_ctx* ctx, const ohgpu_mp4_stream_desc* mp4_descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets,
                                const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                                ohgpu_mp4_stream_result* mp4_results, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    const char* const who = "ohgpu_mp4_alac_process_host";
    if (n && (!mp4_descs || !alac_descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    std::vector<ohgpu_mp4_stream_result> mres(n);
    std::vector<ohgpu_alac_packet> table(n_packets), dense;
    std::vector<ohgpu_alac_stream_desc> adescs(alac_descs, alac_descs + n);
    std::vector<ohgpu_alac_stream_result> ares(n);
    std::vector<ohgpu_alac_packet_result> pres;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_mp4_batch_create(ctx, mp4_descs, n, n_packets, src_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            int e = ohgpu_mp4_batch_run(ctx, b, d_src, nullptr);
            if (e == OHGPU_OK) e = ohgpu_mp4_batch_results(ctx, b, mres.data(), n);              // the one small read between the layers:
            if (e == OHGPU_OK) e = ohgpu_mp4_batch_packets(ctx, b, n_packets ? table.data() : nullptr, n_packets);   // 16 bytes a packet
            if (e == OHGPU_OK && samples) e = ohgpu_mp4_batch_samples(ctx, b, n_packets ? samples : nullptr, n_packets);
            if (e != OHGPU_OK) return e;
            // the Apple Lossless table has the streams' rows one after the other without gaps
            for (size_t i = 0; i < n; i++) {
                ohgpu_alac_stream_desc& a = adescs[i];
                const bool ok = mres[i].status == OHGPU_MP4_OK;
                const uint32_t rows = ok ? std::min(mres[i].samples, mp4_descs[i].packet_capacity) : 0u;
                // a stream that brings no packets still stands in the Apple Lossless batch, whose alac_check_desc (api_alac.hip) judges its
                // configuration and destination: a mono 16-bit configuration with no plane stride is one it accepts whatever the caller wrote
                const ohgpu_alac_config none = {1, 0, 16, 0, 0, 1, 1, 0, 0, 0, 0};
                a.config = ok ? mres[i].config : none;
                a.first_packet = (uint32_t)dense.size();
                a.n_packets = rows;
                if (!ok && !a.flags) a.dst_plane_stride = 0;
                dense.insert(dense.end(), table.begin() + mp4_descs[i].packet_first, table.begin() + mp4_descs[i].packet_first + rows);
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
    if (mp4_results && n) memcpy(mp4_results, mres.data(), n * sizeof(mres[0]));
    if (packets && n_packets) memcpy(packets, table.data(), n_packets * sizeof(table[0]));
    if (alac_results && n) memcpy(alac_results, ares.data(), n * sizeof(ares[0]));
    if (packet_results && n_packets) {
        memset(packet_results, 0, n_packets * sizeof(*packet_results));
        for (size_t i = 0; i < n; i++)
            if (adescs[i].n_packets) memcpy(packet_results + mp4_descs[i].packet_first, pres.data() + adescs[i].first_packet, adescs[i].n_packets * sizeof(pres[0]));
    }
    return OHGPU_OK;
}

}  // extern "C"
