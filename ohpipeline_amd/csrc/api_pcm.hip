// api_pcm.hip -- the C ABI's PCM message batches (include/ohgpu.h: ohgpu_pcm_*).
#include "api_common.h"

using namespace ohgpu;

static int validate_msg(const ohgpu_msg_desc& d, size_t i, uint64_t src_arena, uint64_t dst_arena)
{
    if (d.channels < 1 || d.channels > OHGPU_MAX_CHANNELS)
        return set_error(OHGPU_ERR_INVALID, "desc %zu: channels %u outside 1..8", i, d.channels);
    if (!valid_bits(d.src_bits) || !valid_bits(d.dst_bits))
        return set_error(OHGPU_ERR_INVALID, "desc %zu: bit depth %u -> %u (must be 8/16/24/32)", i, d.src_bits, d.dst_bits);
    if (!valid_endian(d.src_endian) || !valid_endian(d.dst_endian))
        return set_error(OHGPU_ERR_INVALID, "desc %zu: endian %u -> %u", i, d.src_endian, d.dst_endian);
    if (d.flags & ~(OHGPU_FLAG_RAMP | OHGPU_FLAG_SILENCE | OHGPU_FLAG_ZERO_LSB32))
        return set_error(OHGPU_ERR_INVALID, "desc %zu: unknown flag bits 0x%x", i, d.flags);
    if (d.ramp_start > OHGPU_RAMP_MAX || d.ramp_end > OHGPU_RAMP_MAX)
        return set_error(OHGPU_ERR_INVALID, "desc %zu: ramp [%u..%u] beyond Ramp::kMax", i, d.ramp_start, d.ramp_end);
    if ((d.flags & OHGPU_FLAG_RAMP) && d.n_frames > 131071u)     // i*iTotalRamp is TInt arithmetic (Msg.cpp:835)
        return set_error(OHGPU_ERR_INVALID, "desc %zu: ramped message of %u frames overflows the reference's TInt ramp product", i, d.n_frames);
    if (d.attenuation != OHGPU_UNITY_ATTENUATION && d.src_bits != 16)   // ASSERT(iBitDepth == 16), Msg.cpp:2741
        return set_error(OHGPU_ERR_UNSUPPORTED, "desc %zu: attenuation %u on %u-bit audio (16-bit only)", i, d.attenuation, d.src_bits);
    const uint64_t src_bytes = (uint64_t)d.n_frames * d.channels * (d.src_bits / 8);
    const uint64_t dst_bytes = (uint64_t)d.n_frames * d.channels * (d.dst_bits / 8);
    const int err = (d.flags & OHGPU_FLAG_SILENCE) ? OHGPU_OK : arena_span("desc", i, "reads", d.src_offset, src_bytes, src_arena, "source");
    return err != OHGPU_OK ? err : arena_span("desc", i, "writes", d.dst_offset, dst_bytes, dst_arena, "destination");
}

int ohgpu::pcm_batch_create_prefixed(ohgpu_ctx* ctx, const ohgpu_msg_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes,
                                     const MsgPrefix* prefixes, const uint8_t* blob, size_t blob_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_pcm_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_pcm_batch_create", kBatchPcm, descs || !n, n, 0xffffffffull, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err != OHGPU_OK) return err;
    b->uniform = true;
    for (size_t i = 0; i < n; i++) {
        err = validate_msg(descs[i], i, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        const ohgpu_msg_desc& d = descs[i];
        b->in_frames += d.n_frames;
        b->out_frames += d.n_frames;
        if (!(d.flags & OHGPU_FLAG_SILENCE)) b->src_bytes_touched += (uint64_t)d.n_frames * d.channels * (d.src_bits / 8);
        b->dst_bytes_written += (uint64_t)d.n_frames * d.channels * (d.dst_bits / 8);
        if (d.n_frames > b->max_frames) b->max_frames = d.n_frames;
        if (i == 0) {
            b->channels = d.channels; b->src_bits = d.src_bits; b->src_endian = d.src_endian;
            b->dst_bits = d.dst_bits; b->dst_endian = d.dst_endian;
        } else if (d.channels != b->channels || d.src_bits != b->src_bits || d.src_endian != b->src_endian ||
                   d.dst_bits != b->dst_bits || d.dst_endian != b->dst_endian) {
            b->uniform = false;
        }
    }
    err = upload_batch(ctx, b.get(), descs, n * sizeof(ohgpu_msg_desc));
    if (err == OHGPU_OK) err = plan_pcm_line(ctx, b.get(), descs, n, prefixes, blob, blob_bytes);
    return batch_done(err, b, out);
}

extern "C" {

int ohgpu_pcm_batch_create(ohgpu_ctx* ctx, const ohgpu_msg_desc* descs, size_t n,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    return pcm_batch_create_prefixed(ctx, descs, n, src_arena_bytes, dst_arena_bytes, nullptr, nullptr, 0, out);
}

int ohgpu_pcm_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_pcm_batch_run", batch, kBatchPcm, batch && batch->n == 0, true, src_base, dst_base);
    if (go <= 0) return go;
    if (ctx->variant != 1 && batch->line.enabled)
        OHGPU_HIP_TRY(launch_pcm_line(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream)));
    else
        OHGPU_HIP_TRY(launch_pcm_v1(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_pcm_process_host(ohgpu_ctx* ctx, const ohgpu_msg_desc* descs, size_t n,
                           const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes)
{
    CTX_GUARD("ohgpu_pcm_process_host");
    ohgpu_batch* b = nullptr;
    const int err = ohgpu_pcm_batch_create(ctx, descs, n, src_bytes, dst_bytes, &b);
    return err != OHGPU_OK ? err : process_host(ctx, b, n, src_host, src_bytes, dst_host, dst_bytes, ohgpu_pcm_batch_run, [&](size_t i) { return frames_range(descs[i]); });
}

}  // extern "C"
