// api_frag.h -- the C ABI bodies the three fragmented MPEG-4 families share (ohgpu_mp4f_*; ohgpu_cenc_*, 5.20;
// ohgpu_cbcs_*, 5.24): a batch's creation around the family's check and plan, the run's guard, the three tables, the phase times, the
// route, the host-buffer call and the two fused decoder calls.  A family is a traits struct F, defined in csrc/api_mp4f.hip, api_cenc.hip
// and api_cbcs.hip next to their extern "C" functions, which are single calls into this file: Desc, Res and State; kind and noun (with
// its article: "a protected MPEG-4"); state(batch); head(result), the result's ohgpu_mp4f_stream_result; packet_table(state) and
// launch_blocks(state), what ohgpu_*_batch_paths reports; check, keys (what create expands on the host before the plan), plan and run;
// and the family's own extern "C" functions for the calls that go through the public ABI.  Nothing here is exported from the library.
#pragma once

#include <array>

#include "api_common.h"

#pragma GCC visibility push(hidden)
namespace ohgpu {

struct FragCounts { size_t n, n_packets, n_runs, n_subsamples; };      // (n_subsamples: the second protected family's, else 0)
// state(batch) of a family whose state is ohgpu_batch's member M
template <class S, S* ohgpu_batch::*M>
struct FragStateOf {
    using State = S;
    static S*& state(ohgpu_batch* b) { return b->*M; }
    static S* state(const ohgpu_batch* b) { return b->*M; }
};

// The three rules the protected families add to the fields ohgpu_mp4f_batch_check holds (`what`: "cenc desc", "cbcs desc")
template <typename Desc>
int protected_desc_check(const char* what, const Desc& d, size_t i)
{
    for (uint32_t r : d.reserved2) if (r) return set_error(OHGPU_ERR_INVALID, "%s %zu: reserved words must be zero", what, i);
    if (d.flags != OHGPU_MP4F_GATHER) return set_error(OHGPU_ERR_INVALID, "%s %zu: flags 0x%x where the family always gathers (OHGPU_MP4F_GATHER)", what, i, d.flags);
    if (d.key_flags & ~OHGPU_CENC_HAVE_KEY) return set_error(OHGPU_ERR_INVALID, "%s %zu: unknown key_flags 0x%x", what, i, d.key_flags);
    return OHGPU_OK;
}

template <typename F>
int frag_batch_create(ohgpu_ctx* ctx, const char* who, const typename F::Desc* descs, const FragCounts& c, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD(who);
    BatchPtr b;
    int err = batch_begin(ctx, who, F::kind, c.n == 0 || descs, c.n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = F::check(descs, c, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    F::state(b.get()) = new (std::nothrow) typename F::State();
    if (!F::state(b.get())) return set_error(OHGPU_ERR_NOMEM, "%s: out of host memory", who);
    typename F::State& g = *F::state(b.get());
    g.n_streams = c.n; g.n_packets = c.n_packets; g.n_runs = c.n_runs;
    g.plain = ctx->variant == 1;
    for (size_t i = 0; i < c.n; i++) {
        b->src_bytes_touched += descs[i].src_bytes;
        if ((descs[i].flags & OHGPU_MP4F_GATHER) && descs[i].dst_capacity) g.gathers = true;      // (a protected family always gathers: its check)
    }
    F::keys(g, descs, c);
    err = F::plan(ctx, b.get(), descs);
    return batch_done(err, b, out);
}

template <typename F>
int frag_batch_run(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool mine = batch && batch->kind == F::kind;
    const int go = run_guard(ctx, who, batch, F::kind, mine && F::state(batch)->n_streams == 0, true, src_base, dst_base, mine && F::state(batch)->gathers);
    if (go <= 0) return go;
    return F::run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

// The stream results of the last run, joined from the arrays the launches keep them in (F::result_parts: the shared launches keep
// mp4frag's results; what the protection boxes gave lies in arrays of its own): `bytes` a stream at d, to `offset` of the result
struct ResultPart { const void* d; size_t bytes, offset; };
template <typename F>
int frag_batch_results(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, typename F::Res* results, size_t n)
{
    OHGPU_TRY(state_guard(ctx, who, batch, F::kind, F::noun));
    const typename F::State& g = *F::state(batch);
    const auto parts = F::result_parts(g);
    std::vector<std::vector<uint8_t>> home;
    for (const ResultPart& p : parts) {
        home.emplace_back(n * p.bytes);
        OHGPU_TRY(fetch_results(who, g, n, g.n_streams, results ? (void*)home.back().data() : nullptr, p.d, p.bytes));
    }
    for (size_t k = 0; k < parts.size(); k++)
        for (size_t i = 0; i < n; i++) memcpy((uint8_t*)&results[i] + parts[k].offset, &home[k][i * parts[k].bytes], parts[k].bytes);
    return OHGPU_OK;
}

// table 0: the runs, 1: the public packet table, 2: the samples
template <typename F>
int frag_fetch(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, int table, void* out, size_t n_rows)
{
    OHGPU_TRY(state_guard(ctx, who, batch, F::kind, F::noun));
    const typename F::State& g = *F::state(batch);
    return fetch_table(who, g, "rows, the batch's table has", "", n_rows, table == 0 ? g.n_runs : g.n_packets, g.n_streams, out,
                       table == 0 ? g.d_runs : table == 1 ? F::packet_table(g) : g.d_samples, table == 0 ? sizeof(ohgpu_mp4f_run) : 16u);
}

template <typename F>
int frag_batch_phase_ms(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, float ms[6])
{
    OHGPU_TRY(state_guard(ctx, who, batch, F::kind, F::noun));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "%s: bad argument", who);
    const typename F::State& g = *F::state(batch);
    const int err = phase_ms(who, g.ran, g.ev, 6, ms);
    if (err == OHGPU_OK && g.plain) ms[1] = ms[2] = ms[3] = ms[4] = ms[5] = 0.0f;      // (one launch: what lies between the later events is no phase)
    return err;
}

template <typename F>
int frag_batch_paths(const char* who, const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks)
{
    if (!batch || batch->kind != F::kind || !route) return set_error(OHGPU_ERR_INVALID, "%s: not %s batch, or a null argument", who, F::noun);
    const typename F::State& g = *F::state(batch);
    *route = g.plain ? OHGPU_MP4F_ROUTE_PLAIN : OHGPU_MP4F_ROUTE_PHASES;
    if (tiles) *tiles = g.n_tiles;
    if (wave_blocks) *wave_blocks = g.plain ? 0u : F::launch_blocks(g);
    return OHGPU_OK;
}

// ohgpu_*_head's arguments, before the family's walk
inline int frag_head_args(const char* who, const void* bytes, size_t n, const void* result)
{
    if ((n && !bytes) || !result) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    if (n >= 0x80000000ull) return set_error(OHGPU_ERR_INVALID, "%s: %zu bytes are 2^31 or more", who, n);
    return OHGPU_OK;
}

// A run on the context's stream, then what the host-buffer call and the two decoder calls fetch after it (through the family's public
// calls, under their names); any pointer may be null
template <typename F>
int frag_run_fetch(ohgpu_ctx* ctx, const ohgpu_batch* b, const void* d_src, void* d_dst, const FragCounts& c, typename F::Res* results, ohgpu_mp4f_run* runs,
                   ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    int e = F::run_c(ctx, b, d_src, d_dst, nullptr);
    if (e == OHGPU_OK && results) e = F::results(ctx, b, c.n ? results : nullptr, c.n);
    if (e == OHGPU_OK && runs) e = F::runs(ctx, b, c.n_runs ? runs : nullptr, c.n_runs);
    if (e == OHGPU_OK && packets) e = F::packets(ctx, b, c.n_packets ? packets : nullptr, c.n_packets);
    if (e == OHGPU_OK && samples) e = F::samples(ctx, b, c.n_packets ? samples : nullptr, c.n_packets);
    return e;
}

template <typename F>
int frag_process_host(ohgpu_ctx* ctx, const char* who, const typename F::Desc* descs, const FragCounts& c, const void* src_host, uint64_t src_bytes, void* dst_host,
                      uint64_t dst_bytes, typename F::Res* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    std::vector<typename F::Res> res(c.n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return F::create(ctx, descs, c, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) { return frag_run_fetch<F>(ctx, b, d_src, d_dst, c, res.data(), runs, packets, samples); },
        [&] {   // only what was gathered comes back
            for (size_t i = 0; i < c.n; i++) {
                if (!F::head(res[i]).bytes_gathered) continue;
                const int e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, 1, 0, F::head(res[i]).bytes_gathered);
                if (e != OHGPU_OK) return e;
            }
            return (int)OHGPU_OK;
        });
    if (err == OHGPU_OK && results && c.n) memcpy(results, res.data(), c.n * sizeof(res[0]));
    return err;
}

// The whole of a family's fused call to the FLAC decoder: one upload, the family's batch over a middle arena of mid_bytes that lives on
// the device only, its run and its results and tables home, a FLAC batch over the runs the family wrote -- the CLEAR runs of a protected
// family; a stream's src_bytes is its bytes_gathered, 0 for a stream that is not fLaC --, and of dst_host the samples that were decoded.
// flac_descs[i].src_offset must be descs[i].dst_offset.
template <typename F>
int frag_flac_process_host(ohgpu_ctx* ctx, const char* who, const typename F::Desc* descs, const ohgpu_flac_stream_desc* flac_descs, const FragCounts& c, const void* src_host,
                           uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes, typename F::Res* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets,
                           ohgpu_mp4_sample* samples, ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    const size_t n = c.n;
    if (n && (!descs || !flac_descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    for (size_t i = 0; i < n; i++)
        if (flac_descs[i].src_offset != descs[i].dst_offset)
            return set_error(OHGPU_ERR_INVALID, "%s: stream %zu: the FLAC descriptor reads at %llu where the demultiplexer gathers at %llu", who, i,
                             (unsigned long long)flac_descs[i].src_offset, (unsigned long long)descs[i].dst_offset);
    if (n_frames) *n_frames = 0;
    std::vector<typename F::Res> mres(n);
    std::vector<ohgpu_flac_stream_result> fres(n);
    std::vector<ohgpu_flac_stream_desc> fdescs(flac_descs, flac_descs + n);
    void* d_mid = nullptr;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return F::create(ctx, descs, c, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, &d_mid, mid_bytes ? mid_bytes : 1));      // the middle arena: the gathered bytes never leave the device
            int e = frag_run_fetch<F>(ctx, b, d_src, d_mid, c, mres.data(), runs, packets, samples);      // (the results: the one small read between the layers)
            if (e != OHGPU_OK) return e;
            for (size_t i = 0; i < n; i++) fdescs[i].src_bytes = F::head(mres[i]).codec == mp4box::fourcc('f', 'L', 'a', 'C') ? F::head(mres[i]).bytes_gathered : 0u;
            ohgpu_batch* fb = nullptr;
            e = ohgpu_flac_batch_create(ctx, fdescs.data(), n, mid_bytes, dst_bytes, &fb);
            if (e != OHGPU_OK) return e;
            const BatchPtr own(fb, BatchDeleter{ctx});
            e = ohgpu_flac_batch_run(ctx, fb, d_mid, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_flac_batch_results(ctx, fb, fres.data(), n);
            if (e == OHGPU_OK && (frames || n_frames)) e = ohgpu_flac_batch_frames(ctx, fb, frames, frames ? frames_capacity : 0, n_frames);
            return e;
        },
        [&] {   // only what was decoded comes back, as in ohgpu_flac_process_host
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++) e = flac_download_decoded(ctx, who, fdescs[i], fres[i], dst_host);
            return e;
        });
    if (d_mid) { (void)hipStreamSynchronize(ctx->stream); ctx_dev_free(ctx, d_mid); }
    if (err == OHGPU_OK && results && n) memcpy(results, mres.data(), n * sizeof(mres[0]));
    if (err == OHGPU_OK && flac_results && n) memcpy(flac_results, fres.data(), n * sizeof(fres[0]));
    return err;
}

// The whole of a protected family's fused call to the Apple Lossless decoder: the family's batch over a middle arena of mid_bytes that
// lives on the device only, its run and its results and tables home, an Apple Lossless batch over the rows the family wrote -- the CLEAR
// packets --, and of dst_host the samples that were decoded.
template <typename F>
int frag_alac_process_host(ohgpu_ctx* ctx, const char* who, const typename F::Desc* descs, const ohgpu_alac_stream_desc* alac_descs, const FragCounts& c, const void* src_host,
                           uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes, typename F::Res* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets,
                           ohgpu_mp4_sample* samples, ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    const size_t n = c.n, n_packets = c.n_packets;
    if (n && (!descs || !alac_descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    std::vector<typename F::Res> cres(n);
    std::vector<ohgpu_alac_packet> table(n_packets), dense;
    std::vector<ohgpu_alac_stream_desc> adescs(alac_descs, alac_descs + n);
    std::vector<ohgpu_alac_stream_result> ares(n);
    std::vector<ohgpu_alac_packet_result> pres;
    std::vector<uint32_t> first_row(n, 0);
    void* d_mid = nullptr;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return F::create(ctx, descs, c, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, &d_mid, mid_bytes ? mid_bytes : 1));      // the middle arena: the clear packets never leave the device
            int e = frag_run_fetch<F>(ctx, b, d_src, d_mid, c, cres.data(), runs, table.data(), samples);      // (with the one small read between the layers)
            if (e != OHGPU_OK) return e;
            // the Apple Lossless table has the streams' gathered rows one after the other without gaps: places in the middle arena
            for (size_t i = 0; i < n; i++) {
                ohgpu_alac_stream_desc& a = adescs[i];
                const ohgpu_mp4f_stream_result& m = F::head(cres[i]);
                const bool ok = m.status == OHGPU_MP4F_OK && m.codec == mp4box::fourcc('a', 'l', 'a', 'c') && m.bytes_gathered != 0u;
                const uint32_t from = descs[i].gather_first_row, rows = ok ? m.samples_available - from : 0u;
                // (a stream that brings no packets still stands in the Apple Lossless batch: see ohgpu_mp4_alac_process_host)
                const ohgpu_alac_config none = {1, 0, 16, 0, 0, 1, 1, 0, 0, 0, 0};
                a.config = ok ? m.config : none;
                a.first_packet = (uint32_t)dense.size();
                a.n_packets = rows;
                first_row[i] = descs[i].packet_first + from;
                if (!ok && !a.flags) a.dst_plane_stride = 0;
                if (rows) dense.insert(dense.end(), table.begin() + first_row[i], table.begin() + first_row[i] + rows);
            }
            pres.resize(dense.size());
            if (dense.empty()) return (int)OHGPU_OK;
            ohgpu_batch* ab = nullptr;
            e = ohgpu_alac_batch_create(ctx, adescs.data(), n, dense.data(), dense.size(), mid_bytes, dst_bytes, &ab);
            if (e != OHGPU_OK) return e;
            const BatchPtr own(ab, BatchDeleter{ctx});
            e = ohgpu_alac_batch_run(ctx, ab, d_mid, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_alac_batch_results(ctx, ab, ares.data(), n, pres.data(), pres.size());
            return e;
        },
        [&] {   // only what was decoded comes back, as in ohgpu_alac_process_host
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (adescs[i].n_packets) e = alac_download_decoded(ctx, who, adescs[i], pres.data() + adescs[i].first_packet, dst_host);
            return e;
        });
    if (d_mid) { (void)hipStreamSynchronize(ctx->stream); ctx_dev_free(ctx, d_mid); }
    if (err != OHGPU_OK) return err;
    if (results && n) memcpy(results, cres.data(), n * sizeof(cres[0]));
    if (packets && n_packets) memcpy(packets, table.data(), n_packets * sizeof(table[0]));
    if (alac_results && n) memcpy(alac_results, ares.data(), n * sizeof(ares[0]));
    if (packet_results && n_packets) {
        memset(packet_results, 0, n_packets * sizeof(*packet_results));
        for (size_t i = 0; i < n; i++)
            if (adescs[i].n_packets) memcpy(packet_results + first_row[i], pres.data() + adescs[i].first_packet, adescs[i].n_packets * sizeof(pres[0]));
    }
    return OHGPU_OK;
}

}  // namespace ohgpu
#pragma GCC visibility pop
