// api_iff.hip -- the C ABI's PCM file layer (ohgpu_iff_*): the validation of one descriptor, and the family's nouns, plan,
// run and written bytes handed to the file layers' one shell (api_file.h).
#include <algorithm>
#include <cstring>

#include "api_file.h"

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

}  // namespace

extern "C" {

int ohgpu_iff_batch_check(const ohgpu_iff_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    return file_batch_check("ohgpu_iff_batch_check", descs, n, src_arena_bytes, dst_arena_bytes, iff_check_desc);
}

int ohgpu_iff_batch_create(ohgpu_ctx* ctx, const ohgpu_iff_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    return file_batch_create(ctx, "ohgpu_iff_batch_create", kBatchIff, descs, n, src_arena_bytes, dst_arena_bytes, out, ohgpu_iff_batch_check, iff_plan);
}

int ohgpu_iff_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    return file_batch_run(ctx, "ohgpu_iff_batch_run", kBatchIff, batch, src_base, dst_base, stream, 1, iff_run);
}

int ohgpu_iff_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_iff_stream_result* results, size_t n)
{
    return file_batch_results(ctx, "ohgpu_iff_batch_results", kBatchIff, "a PCM file", batch, results, n);
}

int ohgpu_iff_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[2])
{
    return file_batch_phase_ms(ctx, "ohgpu_iff_batch_phase_ms", kBatchIff, "a PCM file", batch, ms);
}

int ohgpu_iff_process_host(ohgpu_ctx* ctx, const ohgpu_iff_stream_desc* descs, size_t n, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                           ohgpu_iff_stream_result* results)
{
    return file_process_host(ctx, "ohgpu_iff_process_host", descs, n, src_host, src_bytes, dst_host, dst_bytes, results, ohgpu_iff_batch_create, ohgpu_iff_batch_run,
                             ohgpu_iff_batch_results, [](const ohgpu_iff_stream_result& r) -> uint64_t {
                                 return r.status == OHGPU_IFF_OK ? r.frames_written * r.channels * (r.out_bit_depth / 8u) : 0u;
                             });
}

}  // extern "C"
