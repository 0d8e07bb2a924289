// api_raop_rx.hip -- the C ABI's RAOP receiver (ohgpu_raop_rx_*): the validation of the two tables, the batch's life
// around csrc/raop_rx_kernel.hip's three launches, the results and the packet table, the host-buffer call and the fused call into
// ohgpu_raop_*.
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

int rx_check_stream(const ohgpu_raop_rx_stream& s, size_t i, const ohgpu_raop_rx_datagram* grams, uint64_t next, size_t n_grams, uint64_t src_arena_bytes)
{
    if (s.reserved) return set_error(OHGPU_ERR_INVALID, "raop rx stream %zu: reserved word must be zero", i);
    for (uint8_t r : s.state_in.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "raop rx stream %zu: the state's reserved bytes must be zero", i);
    if (s.state_in.running > 1 || s.state_in.started > 1 || s.state_in.resume_pending > 1)
        return set_error(OHGPU_ERR_INVALID, "raop rx stream %zu: running, started and resume_pending are 0 or 1", i);
    if (s.max_frames < 1 || s.max_frames > OHGPU_RAOP_RX_MAX_FRAMES) return set_error(OHGPU_ERR_INVALID, "raop rx stream %zu: max_frames %u outside 1..%u", i, s.max_frames, OHGPU_RAOP_RX_MAX_FRAMES);
    if (s.first_datagram != next || s.n_datagrams > n_grams - next)
        return set_error(OHGPU_ERR_INVALID, "raop rx stream %zu: datagrams [%u, +%u) where the table goes on at %llu of %zu", i, s.first_datagram, s.n_datagrams, (unsigned long long)next, n_grams);
    for (uint32_t k = 0; k < s.n_datagrams; k++) {
        const ohgpu_raop_rx_datagram& g = grams[s.first_datagram + k];
        for (uint8_t r : g.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "raop rx stream %zu: datagram %u: reserved bytes must be zero", i, k);
        if (g.port > OHGPU_RAOP_RX_PORT_CONTROL) return set_error(OHGPU_ERR_INVALID, "raop rx stream %zu: datagram %u: port %u is neither audio nor control", i, k, g.port);
        if (g.src_offset % 4 != 0) return set_error(OHGPU_ERR_INVALID, "raop rx stream %zu: datagram %u: src_offset %llu is no multiple of 4", i, k, (unsigned long long)g.src_offset);
        const int err = arena_span("raop rx stream", i, "reads", g.src_offset, g.bytes, src_arena_bytes, "source");
        if (err != OHGPU_OK) return err;
    }
    return OHGPU_OK;
}

bool rx_empty(const ohgpu_batch* b) { return b && b->kind == kBatchRaopRx && b->raoprx->n_datagrams == 0 && b->raoprx->n_streams == 0; }

}  // namespace

extern "C" {

int ohgpu_raop_rx_batch_check(const ohgpu_raop_rx_stream* streams, size_t n, const ohgpu_raop_rx_datagram* datagrams, size_t n_datagrams, uint64_t src_arena_bytes)
{
    if ((n && !streams) || (n_datagrams && !datagrams)) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_rx_batch_check: null argument");
    if (n > 0x00ffffffull || n_datagrams > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_rx_batch_check: too many descriptors");
    uint64_t next = 0;
    for (size_t i = 0; i < n; i++) {
        const int err = rx_check_stream(streams[i], i, datagrams, next, n_datagrams, src_arena_bytes);
        if (err != OHGPU_OK) return err;
        next += streams[i].n_datagrams;
    }
    if (next != n_datagrams) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_rx_batch_check: the streams take %llu datagrams of a table of %zu", (unsigned long long)next, n_datagrams);
    return OHGPU_OK;
}

int ohgpu_raop_rx_batch_create(ohgpu_ctx* ctx, const ohgpu_raop_rx_stream* streams, size_t n, const ohgpu_raop_rx_datagram* datagrams, size_t n_datagrams,
                               uint64_t src_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_raop_rx_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_raop_rx_batch_create", kBatchRaopRx, true, n, UINT64_MAX, src_arena_bytes, 0, out, &b);
    if (err == OHGPU_OK) err = ohgpu_raop_rx_batch_check(streams, n, datagrams, n_datagrams, src_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->raoprx = new (std::nothrow) RaopRxState();
    if (!b->raoprx) return set_error(OHGPU_ERR_NOMEM, "ohgpu_raop_rx_batch_create: out of host memory");
    b->raoprx->n_streams = n;
    b->raoprx->n_datagrams = n_datagrams;
    b->raoprx->plain = ctx->variant == 1;
    for (size_t k = 0; k < n_datagrams; k++) b->src_bytes_touched += datagrams[k].bytes < 20u ? datagrams[k].bytes : 20u;   // (the headers: no payload byte is read)
    err = raop_rx_plan(ctx, b.get(), (const raoprx::Stream*)streams, (const raoprx::Datagram*)datagrams);
    return batch_done(err, b, out);
}

int ohgpu_raop_rx_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_raop_rx_batch_run", batch, kBatchRaopRx, rx_empty(batch), true, src_base, nullptr, false);
    if (go <= 0) return go;
    if ((uintptr_t)src_base % 4 != 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_rx_batch_run: src_base must be 4-byte aligned");
    return raop_rx_run(ctx, batch, (const uint8_t*)src_base, pick_stream(ctx, stream));
}

int ohgpu_raop_rx_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_raop_rx_stream_result* streams, size_t n, ohgpu_raop_rx_record* records, size_t n_datagrams)
{
    const char* const who = "ohgpu_raop_rx_batch_results";
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchRaopRx, "a RAOP receiver"));
    const RaopRxState& r = *batch->raoprx;
    if ((streams || n) && (n != r.n_streams || !streams)) return set_error(OHGPU_ERR_INVALID, "%s: room for %zu results, the batch has %zu streams", who, n, r.n_streams);
    if ((records || n_datagrams) && (n_datagrams != r.n_datagrams || !records))
        return set_error(OHGPU_ERR_INVALID, "%s: room for %zu records, the batch has %zu datagrams", who, n_datagrams, r.n_datagrams);
    if (r.n_streams == 0 && r.n_datagrams == 0) return OHGPU_OK;
    OHGPU_TRY(fetch_after_run(who, r, streams, r.d_results, streams ? n * sizeof(*streams) : 0));
    return fetch_after_run(who, r, records, r.d_records, records ? n_datagrams * sizeof(*records) : 0);
}

int ohgpu_raop_rx_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_datagrams)
{
    const char* const who = "ohgpu_raop_rx_batch_packets";
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchRaopRx, "a RAOP receiver"));
    const RaopRxState& r = *batch->raoprx;
    return fetch_table(who, r, "rows, the batch's table has", "", n_datagrams, r.n_datagrams, r.n_streams, packets, r.d_rows, sizeof(*packets));
}

int ohgpu_raop_rx_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[3])
{
    const char* const who = "ohgpu_raop_rx_batch_phase_ms";
    OHGPU_TRY(state_guard(ctx, who, batch, kBatchRaopRx, "a RAOP receiver"));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "%s: bad argument", who);
    return phase_ms(who, batch->raoprx->ran, batch->raoprx->ev, 3, ms);
}

int ohgpu_raop_rx_process_host(ohgpu_ctx* ctx, const ohgpu_raop_rx_stream* streams, size_t n, const ohgpu_raop_rx_datagram* datagrams, size_t n_datagrams,
                               const void* src_host, uint64_t src_bytes, ohgpu_raop_rx_stream_result* stream_results, ohgpu_raop_rx_record* records,
                               ohgpu_alac_packet* packets)
{
    const char* const who = "ohgpu_raop_rx_process_host";
    return decoder_process_host(ctx, who, src_host, src_bytes, nullptr, 0,
        [&](ohgpu_batch** b) { return ohgpu_raop_rx_batch_create(ctx, streams, n, datagrams, n_datagrams, src_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void*) {
            int e = ohgpu_raop_rx_batch_run(ctx, b, d_src, nullptr);
            if (e == OHGPU_OK) e = ohgpu_raop_rx_batch_results(ctx, b, stream_results && n ? stream_results : nullptr, stream_results ? n : 0,
                                                               records && n_datagrams ? records : nullptr, records ? n_datagrams : 0);
            if (e == OHGPU_OK && packets && n_datagrams) e = ohgpu_raop_rx_batch_packets(ctx, b, packets, n_datagrams);
            return e;
        },
        [] { return (int)OHGPU_OK; });
}

int ohgpu_raop_rx_alac_process_host(ohgpu_ctx* ctx, const ohgpu_raop_rx_stream* streams, const ohgpu_raop_stream_desc* descs, size_t n,
                                    const ohgpu_raop_rx_datagram* datagrams, size_t n_datagrams, const void* src_host, uint64_t src_bytes,
                                    void* dst_host, uint64_t dst_bytes, ohgpu_raop_rx_stream_result* stream_results, ohgpu_raop_rx_record* records,
                                    ohgpu_alac_packet* packets, ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    const char* const who = "ohgpu_raop_rx_alac_process_host";
    if (n && (!streams || !descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    std::vector<ohgpu_raop_rx_stream_result> rres(n);
    std::vector<ohgpu_alac_packet> table(n_datagrams), dense;
    std::vector<ohgpu_raop_stream_desc> rdescs(descs, descs + n);
    std::vector<ohgpu_alac_stream_result> ares(n);
    std::vector<ohgpu_alac_packet_result> pres;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_raop_rx_batch_create(ctx, streams, n, datagrams, n_datagrams, src_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            int e = ohgpu_raop_rx_batch_run(ctx, b, d_src, nullptr);
            if (e == OHGPU_OK) e = ohgpu_raop_rx_batch_results(ctx, b, rres.data(), n, records && n_datagrams ? records : nullptr, records ? n_datagrams : 0);
            if (e == OHGPU_OK) e = ohgpu_raop_rx_batch_packets(ctx, b, n_datagrams ? table.data() : nullptr, n_datagrams);   // 16 bytes a datagram: the one read between the layers
            if (e != OHGPU_OK) return e;
            for (size_t i = 0; i < n; i++) {      // the RAOP table has the streams' rows one after the other without gaps
                ohgpu_alac_stream_desc& a = rdescs[i].alac;
                a.first_packet = (uint32_t)dense.size();
                a.n_packets = rres[i].n_output;
                dense.insert(dense.end(), table.begin() + streams[i].first_datagram, table.begin() + streams[i].first_datagram + rres[i].n_output);
            }
            pres.resize(dense.size());
            if (dense.empty()) return (int)OHGPU_OK;
            ohgpu_batch* rb = nullptr;
            e = ohgpu_raop_batch_create(ctx, rdescs.data(), n, dense.data(), dense.size(), src_bytes, dst_bytes, &rb);
            if (e != OHGPU_OK) return e;
            const BatchPtr own(rb, BatchDeleter{ctx});
            e = ohgpu_raop_batch_run(ctx, rb, d_src, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_raop_batch_results(ctx, rb, ares.data(), n, pres.data(), pres.size());
            return e;
        },
        [&] {   // what was decoded comes back as in ohgpu_raop_process_host: samples of a decoding stream, each packet of a plaintext one
            for (size_t i = 0; i < n; i++) {
                const ohgpu_alac_stream_desc& a = rdescs[i].alac;
                if (!a.n_packets) continue;
                int e = OHGPU_OK;
                if (!(a.flags & OHGPU_RAOP_OUT_PLAINTEXT)) e = alac_download_decoded(ctx, who, a, pres.data() + a.first_packet, dst_host);
                else
                    for (uint32_t k = 0; k < a.n_packets && e == OHGPU_OK; k++) {
                        const ohgpu_alac_packet& p = dense[a.first_packet + k];
                        if (p.bytes) e = download_planes(ctx, who, dst_host, a.dst_offset, 0, 1, 1, p.src_offset - dense[a.first_packet].src_offset, p.bytes);
                    }
                if (e != OHGPU_OK) return e;
            }
            return (int)OHGPU_OK;
        });
    if (err != OHGPU_OK) return err;
    if (stream_results && n) memcpy(stream_results, rres.data(), n * sizeof(rres[0]));
    if (packets && n_datagrams) memcpy(packets, table.data(), n_datagrams * sizeof(table[0]));
    if (alac_results && n) memcpy(alac_results, ares.data(), n * sizeof(ares[0]));
    if (packet_results && n_datagrams) {
        memset(packet_results, 0, n_datagrams * sizeof(*packet_results));
        for (size_t i = 0; i < n; i++)
            if (rdescs[i].alac.n_packets) memcpy(packet_results + streams[i].first_datagram, pres.data() + rdescs[i].alac.first_packet, rdescs[i].alac.n_packets * sizeof(pres[0]));
    }
    return OHGPU_OK;
}

}  // extern "C"
