// api_dsd_file.hip -- the C ABI's DSD file layer (ohgpu_dsd_file_*): the validation of one descriptor, the family's nouns, plan,
// run and written bytes handed to the file layers' one shell (api_file.h), and the two host-only calls an
// element needs before it has a device result: the walk over a file's first bytes and the rounding of a seek.
#include <algorithm>
#include <cstring>

#include "api_file.h"

using namespace ohgpu;

namespace {

int dsd_file_check_desc(const ohgpu_dsd_file_stream_desc& d, size_t i, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "dsd file desc %zu: reserved words must be zero", i);
    if (d.flags) return set_error(OHGPU_ERR_INVALID, "dsd file desc %zu: unknown flags 0x%x", i, d.flags);
    if (!valid_dsd_format(d.sample_block_words, d.pad_bytes_per_chunk))
        return set_error(OHGPU_ERR_INVALID, "dsd file desc %zu: sample_block_words %u with pad_bytes_per_chunk %u is no DSD format", i, d.sample_block_words, d.pad_bytes_per_chunk);
    if (d.src_bytes >= 0x80000000u) return set_error(OHGPU_ERR_INVALID, "dsd file desc %zu: src_bytes %u is 2^31 or more", i, d.src_bytes);
    if (d.dst_offset % 16u) return set_error(OHGPU_ERR_INVALID, "dsd file desc %zu: dst_offset %llu is no multiple of 16", i, (unsigned long long)d.dst_offset);
    const int err = arena_span("dsd file desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
    return err != OHGPU_OK ? err : arena_span("dsd file desc", i, "writes", d.dst_offset, d.dst_bytes_capacity, dst_arena_bytes, "destination");
}

}  // namespace

extern "C" {

int ohgpu_dsd_file_batch_check(const ohgpu_dsd_file_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    return file_batch_check("ohgpu_dsd_file_batch_check", descs, n, src_arena_bytes, dst_arena_bytes, dsd_file_check_desc);
}

int ohgpu_dsd_file_batch_create(ohgpu_ctx* ctx, const ohgpu_dsd_file_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    return file_batch_create(ctx, "ohgpu_dsd_file_batch_create", kBatchDsdFile, descs, n, src_arena_bytes, dst_arena_bytes, out, ohgpu_dsd_file_batch_check, dsd_file_plan);
}

int ohgpu_dsd_file_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    return file_batch_run(ctx, "ohgpu_dsd_file_batch_run", kBatchDsdFile, batch, src_base, dst_base, stream, 4, dsd_file_run);
}

int ohgpu_dsd_file_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_dsd_file_stream_result* results, size_t n)
{
    return file_batch_results(ctx, "ohgpu_dsd_file_batch_results", kBatchDsdFile, "a DSD file", batch, results, n);
}

int ohgpu_dsd_file_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[2])
{
    return file_batch_phase_ms(ctx, "ohgpu_dsd_file_batch_phase_ms", kBatchDsdFile, "a DSD file", batch, ms);
}

int ohgpu_dsd_file_process_host(ohgpu_ctx* ctx, const ohgpu_dsd_file_stream_desc* descs, size_t n, const void* src_host, uint64_t src_bytes, void* dst_host,
                                uint64_t dst_bytes, ohgpu_dsd_file_stream_result* results)
{
    return file_process_host(ctx, "ohgpu_dsd_file_process_host", descs, n, src_host, src_bytes, dst_host, dst_bytes, results, ohgpu_dsd_file_batch_create,
                             ohgpu_dsd_file_batch_run, ohgpu_dsd_file_batch_results,
                             [](const ohgpu_dsd_file_stream_result& r) -> uint64_t { return r.status == OHGPU_DSD_FILE_OK ? r.bytes_written : 0u; });
}

int ohgpu_dsd_file_head(const void* bytes, uint64_t n, uint32_t sample_block_words, uint32_t pad_bytes_per_chunk, ohgpu_dsd_file_stream_result* result)
{
    if (!result || (n && !bytes)) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_head: null argument");
    if (n >= 0x80000000ull) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_head: %llu bytes are 2^31 or more", (unsigned long long)n);
    if (!valid_dsd_format(sample_block_words, pad_bytes_per_chunk))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_head: sample_block_words %u with pad_bytes_per_chunk %u is no DSD format", sample_block_words, pad_bytes_per_chunk);
    dsdfile::Stream s = {};
    s.src_bytes = (uint32_t)n;
    s.dst_bytes_capacity = 1ull << 62;                                // room for any file's chunks
    s.sample_block_words = sample_block_words;
    s.pad_bytes_per_chunk = pad_bytes_per_chunk;
    dsdfile::Result r;
    dsdfile::Rec rec;
    dsdfile::walk(s, (const uint8_t*)bytes, &r, &rec);
    memcpy(result, &r, sizeof(r));
    return OHGPU_OK;
}

int ohgpu_dsd_file_seek(uint32_t kind, uint64_t sample, uint64_t* chunk_first, uint64_t* sample_rounded)
{
    if (!chunk_first || !sample_rounded) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_seek: null argument");
    if (kind != OHGPU_DSD_FILE_KIND_DSF && kind != OHGPU_DSD_FILE_KIND_DFF) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_seek: kind %u", kind);
    // DSF: a pair of 4096-byte planes holds 32768 samples a channel; DFF: the reference's 2048-sample grid
    const uint64_t grid = kind == OHGPU_DSD_FILE_KIND_DSF ? 32768u : 2048u;
    *sample_rounded = sample & ~(grid - 1u);
    *chunk_first = *sample_rounded / 16u;
    return OHGPU_OK;
}

}  // extern "C"
