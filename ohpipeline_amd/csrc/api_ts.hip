// api_ts.hip -- the C ABI's MPEG transport stream demultiplexer and ADTS frame table (ohgpu_ts_*, ohgpu_adts_*): the
// validation of the descriptors, the two batches' lives around csrc/ts_packet_kernel.hip's launches, the results and the tables, the
// host-buffer calls and the fused one, and what runs on the host alone: the section checksum, one ADTS header, the ID3v2 tags.
#include <algorithm>
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

int ts_check_desc(const ohgpu_ts_stream_desc& d, size_t i, size_t n_pes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "ts desc %zu: reserved words must be zero", i);
    if (d.flags & ~(uint32_t)tspkt::kKnownFlags) return set_error(OHGPU_ERR_INVALID, "ts desc %zu: unknown flags 0x%x", i, d.flags);
    if (d.src_bytes >= 0x80000000u) return set_error(OHGPU_ERR_INVALID, "ts desc %zu: src_bytes %u is 2^31 or more", i, d.src_bytes);
    if (d.pmt_pid > 0x1fffu || d.audio_pid > 0x1fffu) return set_error(OHGPU_ERR_INVALID, "ts desc %zu: PIDs 0x%x, 0x%x where a PID has 13 bits", i, d.pmt_pid, d.audio_pid);
    if (d.pes_capacity && (d.pes_first > n_pes || d.pes_capacity > n_pes - d.pes_first))
        return set_error(OHGPU_ERR_INVALID, "ts desc %zu: PES records [%u, +%u) of a table of %zu", i, d.pes_first, d.pes_capacity, n_pes);
    int err = arena_span("ts desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
    if (err == OHGPU_OK) err = arena_span("ts desc", i, "writes", d.dst_offset, d.dst_capacity, dst_arena_bytes, "destination");
    if (err != OHGPU_OK) return err;
    const uint64_t need = (uint64_t)(d.src_bytes / tspkt::kPacket) * 184u;
    if (d.dst_capacity < need)
        return set_error(OHGPU_ERR_BOUNDS, "ts desc %zu: dst_capacity %llu where %u packets can deliver %llu bytes", i, (unsigned long long)d.dst_capacity,
                         d.src_bytes / tspkt::kPacket, (unsigned long long)need);
    return OHGPU_OK;
}

int adts_check_desc(const ohgpu_adts_stream_desc& d, size_t i, size_t n_frames, uint64_t src_arena_bytes)
{
    for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "adts desc %zu: reserved words must be zero", i);
    if (d.flags & ~(uint32_t)adts::kKnownFlags) return set_error(OHGPU_ERR_INVALID, "adts desc %zu: unknown flags 0x%x", i, d.flags);
    if (d.src_bytes >= 0x80000000u) return set_error(OHGPU_ERR_INVALID, "adts desc %zu: src_bytes %u is 2^31 or more", i, d.src_bytes);
    if (d.frame_capacity && (d.frame_first > n_frames || d.frame_capacity > n_frames - d.frame_first))
        return set_error(OHGPU_ERR_INVALID, "adts desc %zu: frames [%u, +%u) of a table of %zu", i, d.frame_first, d.frame_capacity, n_frames);
    return arena_span("adts desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- layer 1
int ohgpu_ts_batch_check(const ohgpu_ts_stream_desc* descs, size_t n, size_t n_pes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_ts_batch_check: null argument");
    if (n > 0x00ffffffull || n_pes > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_ts_batch_check: too many descriptors");
    std::vector<std::pair<uint64_t, uint64_t>> ranges;                 // (first, capacity) of the streams that record PES packets
    for (size_t i = 0; i < n; i++) {
        const int err = ts_check_desc(descs[i], i, n_pes, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        if (descs[i].pes_capacity) ranges.emplace_back(descs[i].pes_first, descs[i].pes_capacity);
    }
    return ranges_disjoint("ohgpu_ts_batch_check", "PES", ranges);
}

int ohgpu_ts_batch_create(ohgpu_ctx* ctx, const ohgpu_ts_stream_desc* descs, size_t n, size_t n_pes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_ts_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_ts_batch_create", kBatchTs, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_ts_batch_check(descs, n, n_pes, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->ts = new (std::nothrow) TsState();
    if (!b->ts) return set_error(OHGPU_ERR_NOMEM, "ohgpu_ts_batch_create: out of host memory");
    b->ts->n_streams = n;
    b->ts->n_pes = n_pes;
    b->ts->plain = ctx->variant == 1;
    for (size_t i = 0; i < n; i++) b->src_bytes_touched += descs[i].src_bytes - descs[i].src_bytes % tspkt::kPacket;
    err = ts_plan(ctx, b.get(), (const tspkt::Stream*)descs);
    return batch_done(err, b, out);
}

int ohgpu_ts_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool empty = batch && batch->kind == kBatchTs && batch->ts->n_streams == 0;
    const int go = run_guard(ctx, "ohgpu_ts_batch_run", batch, kBatchTs, empty, true, src_base, dst_base);
    if (go <= 0) return go;
    return ts_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_ts_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ts_stream_result* results, size_t n)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_ts_batch_results", batch, kBatchTs, "a transport stream"));
    const TsState& g = *batch->ts;
    return fetch_results("ohgpu_ts_batch_results", g, n, g.n_streams, results, g.d_results, sizeof(*results));
}

int ohgpu_ts_batch_pes(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ts_pes* pes, size_t n_pes)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_ts_batch_pes", batch, kBatchTs, "a transport stream"));
    const TsState& g = *batch->ts;
    return fetch_table("ohgpu_ts_batch_pes", g, "records, the batch's table has", "", n_pes, g.n_pes, g.n_streams, pes, g.d_pes, sizeof(*pes));
}

int ohgpu_ts_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[3])
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_ts_batch_phase_ms", batch, kBatchTs, "a transport stream"));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_ts_batch_phase_ms: bad argument");
    return phase_ms("ohgpu_ts_batch_phase_ms", batch->ts->ran, batch->ts->ev, 3, ms);
}

int ohgpu_ts_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks)
{
    if (!batch || batch->kind != kBatchTs || !route || !tiles || !wave_blocks) return set_error(OHGPU_ERR_INVALID, "ohgpu_ts_batch_paths: not a transport stream batch, or a null argument");
    *route = batch->ts->plain ? 2u : 1u;
    *tiles = batch->ts->n_tiles;
    *wave_blocks = batch->ts->plain ? 0u : batch->ts->wave_blocks;
    return OHGPU_OK;
}

int ohgpu_ts_process_host(ohgpu_ctx* ctx, const ohgpu_ts_stream_desc* descs, size_t n, size_t n_pes, const void* src_host, uint64_t src_bytes, void* dst_host,
                          uint64_t dst_bytes, ohgpu_ts_stream_result* results, ohgpu_ts_pes* pes)
{
    const char* const who = "ohgpu_ts_process_host";
    std::vector<ohgpu_ts_stream_result> sres(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_ts_batch_create(ctx, descs, n, n_pes, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            int e = ohgpu_ts_batch_run(ctx, b, d_src, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_ts_batch_results(ctx, b, n ? sres.data() : nullptr, n);
            if (e == OHGPU_OK && pes) e = ohgpu_ts_batch_pes(ctx, b, n_pes ? pes : nullptr, n_pes);
            return e;
        },
        [&] {   // only what was delivered comes back (as one "plane" of one-byte samples per stream)
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (sres[i].bytes_delivered) e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, 1, 0, sres[i].bytes_delivered);
            return e;
        });
    if (err == OHGPU_OK && results && n) memcpy(results, sres.data(), n * sizeof(sres[0]));
    return err;
}

uint32_t ohgpu_ts_crc(const void* bytes, size_t n)
{
    if (!bytes) return 0u;
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) c = tspkt::crc_byte(c, ((const uint8_t*)bytes)[i]);
    return c;
}

// ---------------------------------------------------------------- layer 2
int ohgpu_adts_batch_check(const ohgpu_adts_stream_desc* descs, size_t n, size_t n_frames, uint64_t src_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_adts_batch_check: null argument");
    if (n > 0x00ffffffull || n_frames > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_adts_batch_check: too many descriptors");
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (size_t i = 0; i < n; i++) {
        const int err = adts_check_desc(descs[i], i, n_frames, src_arena_bytes);
        if (err != OHGPU_OK) return err;
        if (descs[i].frame_capacity) ranges.emplace_back(descs[i].frame_first, descs[i].frame_capacity);
    }
    return ranges_disjoint("ohgpu_adts_batch_check", "frame", ranges);
}

int ohgpu_adts_batch_create(ohgpu_ctx* ctx, const ohgpu_adts_stream_desc* descs, size_t n, size_t n_frames, uint64_t src_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_adts_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_adts_batch_create", kBatchAdts, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, 0, out, &b);
    if (err == OHGPU_OK) err = ohgpu_adts_batch_check(descs, n, n_frames, src_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->adts = new (std::nothrow) AdtsState();
    if (!b->adts) return set_error(OHGPU_ERR_NOMEM, "ohgpu_adts_batch_create: out of host memory");
    b->adts->n_streams = n;
    b->adts->n_frames = n_frames;
    b->adts->plain = ctx->variant == 1;
    for (size_t i = 0; i < n; i++) b->src_bytes_touched += descs[i].src_bytes;
    err = adts_plan(ctx, b.get(), (const adts::Stream*)descs);
    return batch_done(err, b, out);
}

int ohgpu_adts_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* stream)
{
    const bool empty = batch && batch->kind == kBatchAdts && batch->adts->n_streams == 0;
    const int go = run_guard(ctx, "ohgpu_adts_batch_run", batch, kBatchAdts, empty, true, src_base, nullptr, false);
    if (go <= 0) return go;
    return adts_run(ctx, batch, (const uint8_t*)src_base, pick_stream(ctx, stream));
}

int ohgpu_adts_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_adts_stream_result* results, size_t n)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_adts_batch_results", batch, kBatchAdts, "an ADTS"));
    const AdtsState& g = *batch->adts;
    return fetch_results("ohgpu_adts_batch_results", g, n, g.n_streams, results, g.d_results, sizeof(*results));
}

int ohgpu_adts_batch_frames(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_adts_frame* frames, size_t n_frames)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_adts_batch_frames", batch, kBatchAdts, "an ADTS"));
    const AdtsState& g = *batch->adts;
    return fetch_table("ohgpu_adts_batch_frames", g, "records, the batch's table has", "", n_frames, g.n_frames, g.n_streams, frames, g.d_frames, sizeof(*frames));
}

int ohgpu_adts_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[2])
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_adts_batch_phase_ms", batch, kBatchAdts, "an ADTS"));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_adts_batch_phase_ms: bad argument");
    return phase_ms("ohgpu_adts_batch_phase_ms", batch->adts->ran, batch->adts->ev, 2, ms);
}

int ohgpu_adts_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles)
{
    if (!batch || batch->kind != kBatchAdts || !route || !tiles) return set_error(OHGPU_ERR_INVALID, "ohgpu_adts_batch_paths: not an ADTS batch, or a null argument");
    *route = batch->adts->plain ? 2u : 1u;
    *tiles = batch->adts->n_tiles;
    return OHGPU_OK;
}

int ohgpu_adts_process_host(ohgpu_ctx* ctx, const ohgpu_adts_stream_desc* descs, size_t n, size_t n_frames, const void* src_host, uint64_t src_bytes,
                            ohgpu_adts_stream_result* results, ohgpu_adts_frame* frames)
{
    const char* const who = "ohgpu_adts_process_host";
    return decoder_process_host(ctx, who, src_host, src_bytes, nullptr, 0,
        [&](ohgpu_batch** b) { return ohgpu_adts_batch_create(ctx, descs, n, n_frames, src_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void*) {
            int e = ohgpu_adts_batch_run(ctx, b, d_src, nullptr);
            if (e == OHGPU_OK && results) e = ohgpu_adts_batch_results(ctx, b, n ? results : nullptr, n);
            if (e == OHGPU_OK && frames) e = ohgpu_adts_batch_frames(ctx, b, n_frames ? frames : nullptr, n_frames);
            return e;
        },
        [] { return (int)OHGPU_OK; });
}

int ohgpu_adts_header(const void* bytes, size_t n, ohgpu_adts_frame* out)
{
    if (!bytes || !out) return set_error(OHGPU_ERR_INVALID, "ohgpu_adts_header: null argument");
    adts::Hdr h;
    if (!adts::header_at((const uint8_t*)bytes, (uint32_t)std::min<size_t>(n, 0x7fffffffu), 0, &h)) return set_error(OHGPU_ERR_INVALID, "ohgpu_adts_header: no valid ADTS header in these %zu bytes", n);
    adts::Stream one = {};
    one.frame_capacity = 1;
    adts::put_frame(one, (adts::Frame*)out, 0, 0, h, false);
    return OHGPU_OK;
}

uint64_t ohgpu_id3v2_skip(const void* bytes, size_t n) { return bytes ? adts::id3v2_skip((const uint8_t*)bytes, n) : 0u; }

// ---------------------------------------------------------------- both
int ohgpu_ts_adts_process_host(ohgpu_ctx* ctx, const ohgpu_ts_stream_desc* ts_descs, const ohgpu_adts_stream_desc* adts_descs, size_t n, size_t n_pes, size_t n_frames,
                               const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes, ohgpu_ts_stream_result* ts_results, ohgpu_ts_pes* pes,
                               ohgpu_adts_stream_result* adts_results, ohgpu_adts_frame* frames)
{
    const char* const who = "ohgpu_ts_adts_process_host";
    if (n && (!ts_descs || !adts_descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    for (size_t i = 0; i < n; i++)
        if (adts_descs[i].src_offset > ts_descs[i].dst_offset || ts_descs[i].dst_offset - adts_descs[i].src_offset > 0x00ffffffull || ts_descs[i].dst_offset > dst_bytes)
            return set_error(OHGPU_ERR_INVALID, "%s: stream %zu: the ADTS descriptor reads at %llu where the transport stream descriptor delivers at %llu", who, i,
                             (unsigned long long)adts_descs[i].src_offset, (unsigned long long)ts_descs[i].dst_offset);
    std::vector<ohgpu_ts_stream_result> tres(n);
    std::vector<ohgpu_adts_stream_desc> adescs(adts_descs, adts_descs + n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_ts_batch_create(ctx, ts_descs, n, n_pes, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            for (size_t i = 0; i < n; i++) {                           // what the last chain left unconsumed, in front of the run
                const uint64_t at = adescs[i].src_offset, kept = ts_descs[i].dst_offset - at;
                if (!kept) continue;
                OHGPU_HIP_TRY(hipMemcpyAsync((uint8_t*)d_dst + at, (const uint8_t*)dst_host + at, kept, hipMemcpyHostToDevice, ctx->stream));
                ctx->stage.h2d_bytes += kept;
            }
            int e = ohgpu_ts_batch_run(ctx, b, d_src, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_ts_batch_results(ctx, b, tres.data(), n);                 // the one small read between the layers
            if (e == OHGPU_OK && pes) e = ohgpu_ts_batch_pes(ctx, b, n_pes ? pes : nullptr, n_pes);
            if (e != OHGPU_OK) return e;
            for (size_t i = 0; i < n; i++) adescs[i].src_bytes = (uint32_t)(ts_descs[i].dst_offset - adescs[i].src_offset) + tres[i].bytes_delivered;
            ohgpu_batch* ab = nullptr;
            e = ohgpu_adts_batch_create(ctx, adescs.data(), n, n_frames, dst_bytes, &ab);           // (the run lies in the destination arena)
            if (e != OHGPU_OK) return e;
            const BatchPtr own(ab, BatchDeleter{ctx});
            e = ohgpu_adts_batch_run(ctx, ab, d_dst, nullptr);
            if (e == OHGPU_OK && adts_results) e = ohgpu_adts_batch_results(ctx, ab, adts_results, n);
            if (e == OHGPU_OK && frames) e = ohgpu_adts_batch_frames(ctx, ab, n_frames ? frames : nullptr, n_frames);
            return e;
        },
        [&] {
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (tres[i].bytes_delivered) e = download_planes(ctx, who, dst_host, ts_descs[i].dst_offset, 0, 1, 1, 0, tres[i].bytes_delivered);
            return e;
        });
    if (err == OHGPU_OK && ts_results && n) memcpy(ts_results, tres.data(), n * sizeof(tres[0]));
    return err;
}

}  // extern "C"
