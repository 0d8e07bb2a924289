// api_dsd_file.hip -- the C ABI's DSD file layer (ohgpu_dsd_file_*): the validation of the descriptors, the batch's life
// around csrc/dsd_file_kernel.hip's two launches, the results, the phase times, the host-buffer call, and the two host-only calls an
// element needs before it has a device result: the walk over a file's first bytes and the rounding of a seek.
#include <algorithm>
#include <cstring>

#include "api_common.h"

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

int dsd_file_guard(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch)
{
    CTX_GUARD(who);
    if (!batch || batch->kind != kBatchDsdFile) return set_error(OHGPU_ERR_INVALID, "%s: not a DSD file batch", who);
    return OHGPU_OK;
}

}  // namespace

extern "C" {

int ohgpu_dsd_file_batch_check(const ohgpu_dsd_file_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_batch_check: null argument");
    if (n > 0x00ffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_batch_check: too many descriptors");
    std::vector<std::pair<uint64_t, uint64_t>> ranges;                 // (offset, bytes) of the streams that may write
    for (size_t i = 0; i < n; i++) {
        const int err = dsd_file_check_desc(descs[i], i, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        if (descs[i].dst_bytes_capacity) ranges.emplace_back(descs[i].dst_offset, descs[i].dst_bytes_capacity);
    }
    return ranges_disjoint("ohgpu_dsd_file_batch_check", "destination", ranges);
}

int ohgpu_dsd_file_batch_create(ohgpu_ctx* ctx, const ohgpu_dsd_file_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_dsd_file_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_dsd_file_batch_create", kBatchDsdFile, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_dsd_file_batch_check(descs, n, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->dsdfile = new (std::nothrow) DsdFileState();
    if (!b->dsdfile) return set_error(OHGPU_ERR_NOMEM, "ohgpu_dsd_file_batch_create: out of host memory");
    b->dsdfile->n_streams = n;
    b->dsdfile->plain = ctx->variant == 1;
    for (size_t i = 0; i < n; i++) b->src_bytes_touched += descs[i].src_bytes;
    err = dsd_file_plan(ctx, b.get(), (const dsdfile::Stream*)descs);
    return batch_done(err, b, out);
}

int ohgpu_dsd_file_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool mine = batch && batch->kind == kBatchDsdFile;
    const int go = run_guard(ctx, "ohgpu_dsd_file_batch_run", batch, kBatchDsdFile, mine && batch->dsdfile->n_streams == 0, true, src_base, dst_base,
                             mine && batch->dsdfile->writes);
    if (go <= 0) return go;
    if ((uintptr_t)src_base % 4u) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_batch_run: src_base must be a multiple of 4");
    return dsd_file_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_dsd_file_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_dsd_file_stream_result* results, size_t n)
{
    const int err = dsd_file_guard(ctx, "ohgpu_dsd_file_batch_results", batch);
    if (err != OHGPU_OK) return err;
    const DsdFileState& g = *batch->dsdfile;
    if (n != g.n_streams || (n && !results)) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_batch_results: room for %zu results, the batch has %zu streams", n, g.n_streams);
    if (!n) return OHGPU_OK;
    return fetch_after_run("ohgpu_dsd_file_batch_results", g, results, g.d_results, n * sizeof(*results));
}

int ohgpu_dsd_file_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[2])
{
    const int guard = dsd_file_guard(ctx, "ohgpu_dsd_file_batch_phase_ms", batch);
    if (guard != OHGPU_OK) return guard;
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_file_batch_phase_ms: bad argument");
    const int err = phase_ms("ohgpu_dsd_file_batch_phase_ms", batch->dsdfile->ran, batch->dsdfile->ev, 2, ms);
    if (err == OHGPU_OK && batch->dsdfile->plain) ms[1] = 0.0f;      // (one launch: what lies between the later events is no phase)
    return err;
}

int ohgpu_dsd_file_process_host(ohgpu_ctx* ctx, const ohgpu_dsd_file_stream_desc* descs, size_t n, const void* src_host, uint64_t src_bytes, void* dst_host,
                                uint64_t dst_bytes, ohgpu_dsd_file_stream_result* results)
{
    const char* const who = "ohgpu_dsd_file_process_host";
    std::vector<ohgpu_dsd_file_stream_result> res(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_dsd_file_batch_create(ctx, descs, n, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            const int e = ohgpu_dsd_file_batch_run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : ohgpu_dsd_file_batch_results(ctx, b, res.data(), n);
        },
        [&] {   // only what was written comes back
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (res[i].status == OHGPU_DSD_FILE_OK && res[i].bytes_written)
                    e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, 1, 0, res[i].bytes_written);
            return e;
        });
    if (err == OHGPU_OK && results && n) memcpy(results, res.data(), n * sizeof(res[0]));
    return err;
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
