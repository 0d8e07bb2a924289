// api_iff.hip -- the C ABI's PCM file layer (ohgpu_iff_*): the validation of the descriptors, the batch's life around
// csrc/iff_pcm_kernel.hip's two launches, the results, the phase times and the host-buffer call.
#include <algorithm>
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

int iff_check_desc(const ohgpu_iff_stream_desc& d, size_t i, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "iff desc %zu: reserved words must be zero", i);
    if (d.flags & ~(uint32_t)OHGPU_IFF_FLAG_WAV8_UNSIGNED) return set_error(OHGPU_ERR_INVALID, "iff desc %zu: unknown flags 0x%x", i, d.flags);
    if (d.max_bit_depth != 24u && d.max_bit_depth != 32u) return set_error(OHGPU_ERR_INVALID, "iff desc %zu: max_bit_depth %u is neither 24 nor 32", i, d.max_bit_depth);
    if (d.src_bytes >= 0x80000000u) return set_error(OHGPU_ERR_INVALID, "iff desc %zu: src_bytes %u is 2^31 or more", i, d.src_bytes);
    if (d.dst_bytes_capacity > (uint64_t)d.dst_frame_capacity * OHGPU_IFF_MAX_FRAME_BYTES)
        return set_error(OHGPU_ERR_INVALID, "iff desc %zu: dst_bytes_capacity %llu is more than %u frames of %u bytes", i, (unsigned long long)d.dst_bytes_capacity,
                         d.dst_frame_capacity, OHGPU_IFF_MAX_FRAME_BYTES);
    const int err = arena_span("iff desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
    return err != OHGPU_OK ? err : arena_span("iff desc", i, "writes", d.dst_offset, d.dst_bytes_capacity, dst_arena_bytes, "destination");
}

int iff_guard(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch)
{
    CTX_GUARD(who);
    if (!batch || batch->kind != kBatchIff) return set_error(OHGPU_ERR_INVALID, "%s: not a PCM file batch", who);
    return OHGPU_OK;
}

}  // namespace

extern "C" {

int ohgpu_iff_batch_check(const ohgpu_iff_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_iff_batch_check: null argument");
    if (n > 0x00ffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_iff_batch_check: too many descriptors");
    std::vector<std::pair<uint64_t, uint64_t>> ranges;                 // (offset, bytes) of the streams that may write
    for (size_t i = 0; i < n; i++) {
        const int err = iff_check_desc(descs[i], i, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        if (descs[i].dst_bytes_capacity) ranges.emplace_back(descs[i].dst_offset, descs[i].dst_bytes_capacity);
    }
    return ranges_disjoint("ohgpu_iff_batch_check", "destination", ranges);
}

int ohgpu_iff_batch_create(ohgpu_ctx* ctx, const ohgpu_iff_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_iff_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_iff_batch_create", kBatchIff, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_iff_batch_check(descs, n, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->iff = new (std::nothrow) IffState();
    if (!b->iff) return set_error(OHGPU_ERR_NOMEM, "ohgpu_iff_batch_create: out of host memory");
    b->iff->n_streams = n;
    b->iff->plain = ctx->variant == 1;
    for (size_t i = 0; i < n; i++) b->src_bytes_touched += descs[i].src_bytes;
    err = iff_plan(ctx, b.get(), (const iffchunk::Stream*)descs);
    return batch_done(err, b, out);
}

int ohgpu_iff_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool mine = batch && batch->kind == kBatchIff;
    const int go = run_guard(ctx, "ohgpu_iff_batch_run", batch, kBatchIff, mine && batch->iff->n_streams == 0, true, src_base, dst_base, mine && batch->iff->writes);
    if (go <= 0) return go;
    return iff_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_iff_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_iff_stream_result* results, size_t n)
{
    const int err = iff_guard(ctx, "ohgpu_iff_batch_results", batch);
    if (err != OHGPU_OK) return err;
    const IffState& g = *batch->iff;
    if (n != g.n_streams || (n && !results)) return set_error(OHGPU_ERR_INVALID, "ohgpu_iff_batch_results: room for %zu results, the batch has %zu streams", n, g.n_streams);
    if (!n) return OHGPU_OK;
    return fetch_after_run("ohgpu_iff_batch_results", g, results, g.d_results, n * sizeof(*results));
}

int ohgpu_iff_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[2])
{
    const int guard = iff_guard(ctx, "ohgpu_iff_batch_phase_ms", batch);
    if (guard != OHGPU_OK) return guard;
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_iff_batch_phase_ms: bad argument");
    const int err = phase_ms("ohgpu_iff_batch_phase_ms", batch->iff->ran, batch->iff->ev, 2, ms);
    if (err == OHGPU_OK && batch->iff->plain) ms[1] = 0.0f;          // (one launch: what lies between the later events is no phase)
    return err;
}

int ohgpu_iff_process_host(ohgpu_ctx* ctx, const ohgpu_iff_stream_desc* descs, size_t n, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                           ohgpu_iff_stream_result* results)
{
    const char* const who = "ohgpu_iff_process_host";
    std::vector<ohgpu_iff_stream_result> res(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_iff_batch_create(ctx, descs, n, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            const int e = ohgpu_iff_batch_run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : ohgpu_iff_batch_results(ctx, b, res.data(), n);
        },
        [&] {   // only what was written comes back
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (res[i].status == OHGPU_IFF_OK && res[i].frames_written)
                    e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, (uint64_t)res[i].channels * (res[i].out_bit_depth / 8u), 0, res[i].frames_written);
            return e;
        });
    if (err == OHGPU_OK && results && n) memcpy(results, res.data(), n * sizeof(res[0]));
    return err;
}

}  // extern "C"
