// api_dsd.hip -- the C ABI's DSD packers, pass-through and silence (ohgpu_dsd_*).
#include <cstdio>

#include "api_common.h"

using namespace ohgpu;

extern "C" {

// The rules of ohgpu.h's DSD section in one place: ohgpu_dsd_layout, and every descriptor of ohgpu_dsd_batch_create.
static int dsd_check(const char* who, uint32_t kind, uint32_t flags, uint32_t W, uint32_t P, uint32_t n_chunks, uint64_t* src_bytes, uint64_t* dst_bytes)
{
    if (kind != OHGPU_DSD_PASS && kind != OHGPU_DSD_DSF && kind != OHGPU_DSD_DFF && kind != OHGPU_DSD_RAW)
        return set_error(OHGPU_ERR_INVALID, "%s: unknown kind %u", who, kind);
    if (flags & ~OHGPU_DSD_FLAG_SILENCE) return set_error(OHGPU_ERR_INVALID, "%s: unknown flags 0x%x", who, flags);
    // ASSERT((W * 4) % (4 + P) == 0) with W - P chunks per block: DsdDsf.cpp:108,196, DsdDff.cpp:92,334, Msg.cpp:2385
    if (!valid_dsd_format(W, P))
        return set_error(OHGPU_ERR_INVALID, "%s: sample block of %u words with %u pad bytes per chunk (P == 0, or W == P + 4 with P even)", who, W, P);
    const uint64_t cs = 4 + P, per_block = W * 4 / cs, blocks = (n_chunks + per_block - 1) / per_block;
    const bool silent = (flags & OHGPU_DSD_FLAG_SILENCE) != 0;
    if ((silent || kind == OHGPU_DSD_RAW || kind == OHGPU_DSD_PASS) && n_chunks % per_block != 0)   // ASSERT, Msg.cpp:2922
        return set_error(OHGPU_ERR_INVALID, "%s: %u chunks are not whole sample blocks of %llu (Raw, pass-through and silence take whole blocks)", who, n_chunks, (unsigned long long)per_block);
    if (src_bytes) {
        if (silent) *src_bytes = 0;
        else if (kind == OHGPU_DSD_DSF) *src_bytes = ((uint64_t)n_chunks + 2047) / 2048 * 8192;
        else if (kind == OHGPU_DSD_PASS) *src_bytes = n_chunks * cs;
        else *src_bytes = (uint64_t)n_chunks * 4;
    }
    if (dst_bytes) *dst_bytes = blocks * W * 4;
    return OHGPU_OK;
}

int ohgpu_dsd_layout(uint32_t kind, uint32_t sample_block_words, uint32_t pad_bytes_per_chunk, uint32_t n_chunks, uint64_t* src_bytes, uint64_t* dst_bytes)
{
    return dsd_check("ohgpu_dsd_layout", kind, 0, sample_block_words, pad_bytes_per_chunk, n_chunks, src_bytes, dst_bytes);
}

int ohgpu_dsd_batch_create(ohgpu_ctx* ctx, const ohgpu_dsd_desc* descs, size_t n,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_dsd_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_dsd_batch_create", kBatchDsd, descs || !n, n, 0xffffffffull, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err != OHGPU_OK) return err;
    for (size_t i = 0; i < n; i++) {
        const ohgpu_dsd_desc& d = descs[i];
        char who[48];
        snprintf(who, sizeof(who), "dsd desc %zu", i);
        uint64_t src_bytes = 0, dst_bytes = 0;
        err = dsd_check(who, d.kind, d.flags, d.sample_block_words, d.pad_bytes_per_chunk, d.n_chunks, &src_bytes, &dst_bytes);
        for (size_t k = 0; k < sizeof(d.reserved) && err == OHGPU_OK; k++)
            if (d.reserved[k]) err = set_error(OHGPU_ERR_INVALID, "%s: reserved bytes must be zero", who);
        if (err == OHGPU_OK && src_bytes > 0) err = arena_span("dsd desc", i, "reads", d.src_offset, src_bytes, src_arena_bytes, "source");   // (a silent descriptor reads no source: its src_offset is not looked at)
        if (err == OHGPU_OK && d.n_chunks > 0) err = arena_span("dsd desc", i, "writes", d.dst_offset, dst_bytes, dst_arena_bytes, "destination");
        if (err != OHGPU_OK) return err;
        b->in_frames += d.n_chunks;
        b->out_frames += d.n_chunks;
        b->src_bytes_touched += src_bytes;
        b->dst_bytes_written += dst_bytes;
    }
    err = upload_batch(ctx, b.get(), descs, n * sizeof(ohgpu_dsd_desc));
    if (err == OHGPU_OK) err = plan_dsd_line(ctx, b.get(), descs, n);
    return batch_done(err, b, out);
}

int ohgpu_dsd_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_dsd_batch_run", batch, kBatchDsd, batch && batch->dsd.n_pieces == 0, true, src_base, dst_base);
    if (go <= 0) return go;
    if (ctx->variant == 1) OHGPU_HIP_TRY(launch_dsd_v1(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream)));
    else OHGPU_HIP_TRY(launch_dsd_line(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_dsd_batch_paths(const ohgpu_batch* b, uint32_t* wide_descs, uint32_t* generic_descs, uint32_t* launches)
{
    if (!b || b->kind != kBatchDsd) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_batch_paths: not a DSD batch");
    if (wide_descs) *wide_descs = b->dsd.n_wide;
    if (generic_descs) *generic_descs = b->dsd.n_generic;
    if (launches) *launches = b->dsd.n_pieces ? 1u : 0u;
    return OHGPU_OK;
}

int ohgpu_dsd_process_host(ohgpu_ctx* ctx, const ohgpu_dsd_desc* descs, size_t n,
                           const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes)
{
    CTX_GUARD("ohgpu_dsd_process_host");
    ohgpu_batch* b = nullptr;
    const int err = ohgpu_dsd_batch_create(ctx, descs, n, src_bytes, dst_bytes, &b);
    return err != OHGPU_OK ? err : process_host(ctx, b, n, src_host, src_bytes, dst_host, dst_bytes, ohgpu_dsd_batch_run, [&](size_t i) {
        uint64_t bytes = 0;
        (void)dsd_check("dsd", descs[i].kind, descs[i].flags, descs[i].sample_block_words, descs[i].pad_bytes_per_chunk, descs[i].n_chunks, nullptr, &bytes);
        return std::make_pair(descs[i].dst_offset, bytes);
    });
}

}  // extern "C"
