// api_ohm_rx.hip -- the C ABI's Songcast receiver (ohgpu_ohm_rx_*): the validation of the two tables, the batch's
// life around csrc/ohm_rx_kernel.hip's three launches, the results, and the host-buffer call.
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

int rx_check_stream(const ohgpu_ohm_rx_stream& s, size_t i, const ohgpu_ohm_rx_datagram* grams, uint64_t next, size_t n_grams,
                    uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    for (uint32_t r : s.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "ohm rx stream %zu: reserved words must be zero", i);
    for (uint32_t r : s.state_in.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "ohm rx stream %zu: the state's reserved words must be zero", i);
    if (s.state_in.running > 1 || s.state_in.stream_msg_due > 1) return set_error(OHGPU_ERR_INVALID, "ohm rx stream %zu: running and stream_msg_due are 0 or 1", i);
    if (s.first_datagram != next || s.n_datagrams > n_grams - next)
        return set_error(OHGPU_ERR_INVALID, "ohm rx stream %zu: datagrams [%u, +%u) where the table goes on at %llu of %zu", i, s.first_datagram, s.n_datagrams, (unsigned long long)next, n_grams);
    uint64_t most = 0;
    for (uint32_t k = 0; k < s.n_datagrams; k++) {
        const ohgpu_ohm_rx_datagram& g = grams[s.first_datagram + k];
        if (g.reserved) return set_error(OHGPU_ERR_INVALID, "ohm rx stream %zu: datagram %u: reserved word must be zero", i, k);
        if (g.src_offset % 4 != 0) return set_error(OHGPU_ERR_INVALID, "ohm rx stream %zu: datagram %u: src_offset %llu is no multiple of 4", i, k, (unsigned long long)g.src_offset);
        const int err = arena_span("ohm rx stream", i, "reads", g.src_offset, g.bytes, src_arena_bytes, "source");
        if (err != OHGPU_OK) return err;
        if (g.bytes > ohmrx::kFixedBytes) most += g.bytes - ohmrx::kFixedBytes;
    }
    const int err = arena_span("ohm rx stream", i, "writes", s.dst_offset, s.dst_capacity, dst_arena_bytes, "destination");
    if (err != OHGPU_OK) return err;
    if (s.dst_capacity < most)
        return set_error(OHGPU_ERR_BOUNDS, "ohm rx stream %zu: dst_capacity %llu where its datagrams may carry %llu audio bytes", i, (unsigned long long)s.dst_capacity, (unsigned long long)most);
    return OHGPU_OK;
}

}  // namespace

extern "C" {

int ohgpu_ohm_rx_batch_check(const ohgpu_ohm_rx_stream* streams, size_t n, const ohgpu_ohm_rx_datagram* datagrams, size_t n_datagrams,
                             uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if ((n && !streams) || (n_datagrams && !datagrams)) return set_error(OHGPU_ERR_INVALID, "ohgpu_ohm_rx_batch_check: null argument");
    if (n > 0x00ffffffull || n_datagrams > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_ohm_rx_batch_check: too many descriptors");
    uint64_t next = 0;
    for (size_t i = 0; i < n; i++) {
        const int err = rx_check_stream(streams[i], i, datagrams, next, n_datagrams, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        next += streams[i].n_datagrams;
    }
    if (next != n_datagrams) return set_error(OHGPU_ERR_INVALID, "ohgpu_ohm_rx_batch_check: the streams take %llu datagrams of a table of %zu", (unsigned long long)next, n_datagrams);
    return OHGPU_OK;
}

int ohgpu_ohm_rx_batch_create(ohgpu_ctx* ctx, const ohgpu_ohm_rx_stream* streams, size_t n, const ohgpu_ohm_rx_datagram* datagrams, size_t n_datagrams,
                              uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_ohm_rx_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_ohm_rx_batch_create", kBatchOhmRx, true, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_ohm_rx_batch_check(streams, n, datagrams, n_datagrams, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->ohmrx = new (std::nothrow) OhmRxState();
    if (!b->ohmrx) return set_error(OHGPU_ERR_NOMEM, "ohgpu_ohm_rx_batch_create: out of host memory");
    b->ohmrx->n_streams = n;
    b->ohmrx->n_datagrams = n_datagrams;
    for (size_t k = 0; k < n_datagrams; k++) b->src_bytes_touched += datagrams[k].bytes;
    static_assert(sizeof(ohmrx::Stream) == sizeof(ohgpu_ohm_rx_stream) && sizeof(ohmrx::Datagram) == sizeof(ohgpu_ohm_rx_datagram), "the tables are read as they are");
    err = ohm_rx_plan(ctx, b.get(), (const ohmrx::Stream*)streams, (const ohmrx::Datagram*)datagrams);
    return batch_done(err, b, out);
}

int ohgpu_ohm_rx_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool empty = batch && batch->kind == kBatchOhmRx && batch->ohmrx->n_datagrams == 0 && batch->ohmrx->n_streams == 0;
    const int go = run_guard(ctx, "ohgpu_ohm_rx_batch_run", batch, kBatchOhmRx, empty, true, src_base, dst_base);
    if (go <= 0) return go;
    if ((uintptr_t)src_base % 4 != 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_ohm_rx_batch_run: src_base must be 4-byte aligned");
    return ohm_rx_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_ohm_rx_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ohm_rx_stream_result* streams, size_t n,
                               ohgpu_ohm_rx_record* records, size_t n_datagrams)
{
    CTX_GUARD("ohgpu_ohm_rx_batch_results");
    if (!batch || batch->kind != kBatchOhmRx) return set_error(OHGPU_ERR_INVALID, "ohgpu_ohm_rx_batch_results: not a Songcast receiver batch");
    const OhmRxState& r = *batch->ohmrx;
    if ((streams || n) && (n != r.n_streams || !streams)) return set_error(OHGPU_ERR_INVALID, "ohgpu_ohm_rx_batch_results: room for %zu results, the batch has %zu streams", n, r.n_streams);
    if ((records || n_datagrams) && (n_datagrams != r.n_datagrams || !records))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_ohm_rx_batch_results: room for %zu records, the batch has %zu datagrams", n_datagrams, r.n_datagrams);
    if (r.n_streams == 0 && r.n_datagrams == 0) return OHGPU_OK;
    OHGPU_TRY(fetch_after_run("ohgpu_ohm_rx_batch_results", r, streams, r.d_results, streams ? n * sizeof(*streams) : 0));
    return fetch_after_run("ohgpu_ohm_rx_batch_results", r, records, r.d_records, records ? n_datagrams * sizeof(*records) : 0);
}

int ohgpu_ohm_rx_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[3])
{
    CTX_GUARD("ohgpu_ohm_rx_batch_phase_ms");
    if (!batch || batch->kind != kBatchOhmRx || !ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_ohm_rx_batch_phase_ms: bad argument");
    return phase_ms("ohgpu_ohm_rx_batch_phase_ms", batch->ohmrx->ran, batch->ohmrx->ev, 3, ms);
}

int ohgpu_ohm_rx_process_host(ohgpu_ctx* ctx, const ohgpu_ohm_rx_stream* streams, size_t n, const ohgpu_ohm_rx_datagram* datagrams, size_t n_datagrams,
                              const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                              ohgpu_ohm_rx_stream_result* stream_results, ohgpu_ohm_rx_record* records)
{
    const char* const who = "ohgpu_ohm_rx_process_host";
    std::vector<ohgpu_ohm_rx_stream_result> sres(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_ohm_rx_batch_create(ctx, streams, n, datagrams, n_datagrams, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            const int e = ohgpu_ohm_rx_batch_run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : ohgpu_ohm_rx_batch_results(ctx, b, n ? sres.data() : nullptr, n, n_datagrams ? records : nullptr, records ? n_datagrams : 0);
        },
        [&] {   // only what was gathered comes back (as one "plane" of one-byte samples per stream)
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (sres[i].out_bytes) e = download_planes(ctx, who, dst_host, streams[i].dst_offset, 0, 1, 1, 0, sres[i].out_bytes);
            return e;
        });
    if (err == OHGPU_OK && stream_results && n) memcpy(stream_results, sres.data(), n * sizeof(sres[0]));
    return err;
}

}  // extern "C"
