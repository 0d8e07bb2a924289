// api_flywheel.hip -- the C ABI's FlywheelRamper batches (N1: ohgpu_flywheel_*).
#include "api_common.h"

using namespace ohgpu;

extern "C" {

int ohgpu_flywheel_batch_create(ohgpu_ctx* ctx, const ohgpu_flywheel_desc* descs, size_t n,
                                uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_flywheel_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_flywheel_batch_create", kBatchFlywheel, descs || !n, n, 0x0fffffffull, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err != OHGPU_OK) return err;
    for (size_t i = 0; i < n; i++) {
        const ohgpu_flywheel_desc& d = descs[i];
        const uint32_t dec = (d.sample_rate == 192000 || d.sample_rate == 176400) ? 4 : ((d.sample_rate == 88200 || d.sample_rate == 96000) ? 2 : 1);
        const uint64_t plane = d.channel_bytes, need = (uint64_t)d.in_samples * 4, out_bytes = (uint64_t)d.out_frames * d.channels * 4;
        if (d.channels < 1 || d.channels > 10) err = set_error(OHGPU_ERR_INVALID, "flywheel desc %zu: channels %u outside 1..10", i, d.channels);
        else if (d.sample_rate > 384000) err = set_error(OHGPU_ERR_INVALID, "flywheel desc %zu: sample rate %u above 384000", i, d.sample_rate);   // ASSERT, FlywheelRamper.cpp:178
        else if (need > plane) err = set_error(OHGPU_ERR_INVALID, "flywheel desc %zu: %llu-byte planes hold fewer than %u samples", i, (unsigned long long)plane, d.in_samples);   // ASSERT, :180
        else if (d.in_samples / dec < 4) err = set_error(OHGPU_ERR_INVALID, "flywheel desc %zu: %u training samples after decimation by %u (need 4)", i, d.in_samples, dec);
        else if (d.in_samples > 65536) err = set_error(OHGPU_ERR_INVALID, "flywheel desc %zu: %u training samples (limit 65536)", i, d.in_samples);
        else if (d.block_frames == 0 && d.out_frames != 0) err = set_error(OHGPU_ERR_INVALID, "flywheel desc %zu: block_frames is 0", i);
        else if (d.src_offset > src_arena_bytes || plane > src_arena_bytes || plane * d.channels > src_arena_bytes - d.src_offset)   // (plane <= arena: the product cannot wrap)
            err = set_error(OHGPU_ERR_BOUNDS, "flywheel desc %zu: training audio beyond the %llu-byte source arena", i, (unsigned long long)src_arena_bytes);
        else if (d.dst_offset > dst_arena_bytes || out_bytes > dst_arena_bytes - d.dst_offset)
            err = set_error(OHGPU_ERR_BOUNDS, "flywheel desc %zu: writes up to %llu beyond the %llu-byte destination arena", i,
                            (unsigned long long)(d.dst_offset + out_bytes), (unsigned long long)dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        b->in_frames += d.in_samples;
        b->out_frames += d.out_frames;
        b->src_bytes_touched += need * d.channels;
        b->dst_bytes_written += out_bytes;
    }
    err = upload_batch(ctx, b.get(), descs, n * sizeof(ohgpu_flywheel_desc));
    if (err == OHGPU_OK) err = plan_flywheel(ctx, b.get(), descs, n);
    return batch_done(err, b, out);
}

int ohgpu_flywheel_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_flywheel_batch_run", batch, kBatchFlywheel, batch && batch->n == 0, false, src_base, dst_base);
    if (go <= 0) return go;
    hipStream_t s = pick_stream(ctx, stream);
    const int claim = claim_single_launch(batch, s, "ohgpu_flywheel_batch_run");       // (Burg's workspace is the batch's)
    if (claim != OHGPU_OK) return claim;
    OHGPU_HIP_TRY(launch_flywheel(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, s));
    launched(batch, s);
    return OHGPU_OK;
}

int ohgpu_flywheel_process_host(ohgpu_ctx* ctx, const ohgpu_flywheel_desc* descs, size_t n,
                                const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes)
{
    CTX_GUARD("ohgpu_flywheel_process_host");
    ohgpu_batch* b = nullptr;
    const int err = ohgpu_flywheel_batch_create(ctx, descs, n, src_bytes, dst_bytes, &b);
    return err != OHGPU_OK ? err : process_host(ctx, b, n, src_host, src_bytes, dst_host, dst_bytes, ohgpu_flywheel_batch_run,
                        [&](size_t i) { return std::make_pair(descs[i].dst_offset, (uint64_t)descs[i].out_frames * descs[i].channels * 4u); });
}

}  // extern "C"
