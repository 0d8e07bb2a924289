// api_src_pull.hip -- the C ABI's pulled resampler (ohgpu_src_pull_*).
#include <algorithm>
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

extern "C" {

// the last output's input position of a message: pos_frame + ((pos_frac + (n_frames - 1) * step) >> 32), false when it overflows
static bool pull_last_frame(uint64_t pos_frame, uint32_t pos_frac, uint64_t step, uint32_t n_frames, uint64_t* last)
{
    uint64_t span = 0, u = 0;
    if (step == 0 || step > OHGPU_SRC_PULL_MAX_STEP || n_frames == 0 || __builtin_mul_overflow((uint64_t)n_frames, step, &span)) return false;
    u = (uint64_t)pos_frac + (span - step);
    if (u < span - step) return false;
    return !__builtin_add_overflow(pos_frame, u >> 32, last);
}

// one pulled message against the rules of ohgpu.h (ohgpu_src_pull_msg_desc); on success its share of the batch's totals
static int check_pull_desc(const ohgpu_src_pull_msg_desc& d, size_t i, uint32_t T, uint64_t src_arena, uint64_t dst_arena, ohgpu_batch* b)
{
    if (d.channels < 1 || d.channels > OHGPU_MAX_CHANNELS) return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: channels %u outside 1..8", i, d.channels);
    if (!valid_bits(d.src_bits) || !valid_endian(d.src_endian) || !valid_endian(d.dst_endian))
        return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: source depth %u / byte orders %u -> %u", i, d.src_bits, d.src_endian, d.dst_endian);
    if (d.dst_bits != 16 && d.dst_bits != 24 && d.dst_bits != 32)
        return set_error(OHGPU_ERR_UNSUPPORTED, "src pull desc %zu: destination depth %u (16, 24 or 32)", i, d.dst_bits);
    if (d.flags & OHGPU_FLAG_SRC_PLANAR32) return set_error(OHGPU_ERR_UNSUPPORTED, "src pull desc %zu: planar sources are not supported on the pulled path", i);
    if (d.flags & ~(OHGPU_FLAG_RAMP | OHGPU_FLAG_ZERO_LSB32)) return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: flag bits 0x%x not valid for a pulled message", i, d.flags);
    if (d.src_plane_stride != 0 || d.reserved[0] || d.reserved[1] || d.reserved[2] || d.reserved[3])
        return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: src_plane_stride and reserved must be zero", i);
    if (d.ramp_start > OHGPU_RAMP_MAX || d.ramp_end > OHGPU_RAMP_MAX) return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: ramp beyond Ramp::kMax", i);
    if ((d.flags & OHGPU_FLAG_RAMP) && d.n_frames > 131071u) return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: ramped message of %u frames", i, d.n_frames);
    if (d.attenuation != OHGPU_UNITY_ATTENUATION) return set_error(OHGPU_ERR_UNSUPPORTED, "src pull desc %zu: attenuation %u (resampled audio is 24-bit; Msg.cpp:2741 allows 16-bit only)", i, d.attenuation);
    if (d.step == 0 || d.step > OHGPU_SRC_PULL_MAX_STEP) return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: step %llu outside 1 .. OHGPU_SRC_PULL_MAX_STEP", i, (unsigned long long)d.step);
    if (d.pos_frame > (1ull << 48) || d.src_frame0 > (1ull << 48) || d.src_frames > (1ull << 40)) return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: frame index out of range", i);
    uint64_t last = d.pos_frame;
    if (d.n_frames > 0 && (!pull_last_frame(d.pos_frame, d.pos_frac, d.step, d.n_frames, &last) || last > (1ull << 49)))
        return set_error(OHGPU_ERR_INVALID, "src pull desc %zu: n_frames * step overflows", i);
    const uint64_t fb_src = (uint64_t)d.channels * (d.src_bits / 8), fb_dst = (uint64_t)d.channels * (d.dst_bits / 8);
    const uint64_t src_bytes = d.src_frames * fb_src, dst_bytes = (uint64_t)d.n_frames * fb_dst;
    int span = arena_span("src pull desc", i, "input window", d.src_offset, src_bytes, src_arena, "source");
    if (span == OHGPU_OK) span = arena_span("src pull desc", i, "writes", d.dst_offset, dst_bytes, dst_arena, "destination");
    if (span != OHGPU_OK) return span;
    if (d.n_frames > 0) {
        const int64_t n_lo = (int64_t)d.pos_frame - (int64_t)(T - 1);
        if (n_lo >= 0 ? (uint64_t)n_lo < d.src_frame0 : d.src_frame0 != 0)
            return set_error(OHGPU_ERR_BOUNDS, "src pull desc %zu: filter history starts at input frame %lld but the buffer starts at %llu", i,
                             (long long)(n_lo < 0 ? 0 : n_lo), (unsigned long long)d.src_frame0);
        if (last >= d.src_frame0 + d.src_frames)
            return set_error(OHGPU_ERR_BOUNDS, "src pull desc %zu: needs input frame %llu but the buffer ends at %llu", i,
                             (unsigned long long)last, (unsigned long long)(d.src_frame0 + d.src_frames));
        b->in_frames += last - d.pos_frame + 1;
        b->src_bytes_touched += (last - (uint64_t)(n_lo < 0 ? 0 : n_lo) + 1) * fb_src;
    }
    b->out_frames += d.n_frames;
    b->dst_bytes_written += dst_bytes;
    if (d.n_frames > b->max_frames) b->max_frames = d.n_frames;
    return OHGPU_OK;
}

int ohgpu_src_pull_design(uint32_t rate_in, uint32_t rate_out, uint32_t taps_per_phase, uint32_t phases_log2, double beta,
                          double f_pass_hz, double max_pull, int32_t* coef_q28, size_t coef_capacity)
{
    if (!coef_q28) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_design: null table");
    std::vector<int32_t> coef;
    const int err = design_src_pull(rate_in, rate_out, taps_per_phase, phases_log2, beta, f_pass_hz, max_pull, &coef);
    if (err != OHGPU_OK) return err;
    if (coef.size() > coef_capacity)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_design: capacity %zu < (P + 1) * T = %zu", coef_capacity, coef.size());
    memcpy(coef_q28, coef.data(), coef.size() * sizeof(int32_t));
    return OHGPU_OK;
}

int ohgpu_src_pull_step(uint32_t rate_in, uint32_t rate_out, uint32_t multiplier, uint64_t* step)
{
    if (!step || rate_in == 0 || rate_out == 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_step: zero rate or null result");
    // 2 * rate_in * multiplier < 2^65: in 128 bits
    const unsigned __int128 v = ((unsigned __int128)2 * rate_in * multiplier) / rate_out;
    if (v == 0 || v > OHGPU_SRC_PULL_MAX_STEP)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_step: %u -> %u at multiplier %u gives a step outside 1 .. 16 input frames", rate_in, rate_out, multiplier);
    *step = (uint64_t)v;
    return OHGPU_OK;
}

int ohgpu_src_pull_window(uint64_t pos_frame, uint32_t pos_frac, uint64_t step, uint32_t n_frames, uint32_t taps_per_phase,
                          uint64_t* first, uint64_t* frames)
{
    uint64_t last = 0;
    if (!first || !frames || taps_per_phase == 0 || !pull_last_frame(pos_frame, pos_frac, step, n_frames, &last))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_window: no frames, a step outside 1 .. OHGPU_SRC_PULL_MAX_STEP, or n_frames * step overflows");
    *first = pos_frame >= taps_per_phase - 1 ? pos_frame - (taps_per_phase - 1) : 0;
    *frames = last - *first + 1;
    return OHGPU_OK;
}

int ohgpu_src_pull_create(ohgpu_ctx* ctx, uint32_t T, uint32_t phases_log2, const int32_t* coef_q28, ohgpu_src** out)
{
    CTX_GUARD("ohgpu_src_pull_create");
    if (!out || !coef_q28) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_create: null argument");
    *out = nullptr;
    if ((T != 32 && T != 64) || phases_log2 < 1 || phases_log2 > 16)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_create: T = %u, phases_log2 = %u", T, phases_log2);
    if (src_pull_lds_bytes(T, phases_log2) > 80u * 1024u)
        return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_pull_create: a table of 2^%u phases of %u taps does not fit the kernel's LDS "
                         "(up to 2^8 phases, T = 32 or 64)", phases_log2, T);
    const int err = check_src_pull_table(T, phases_log2, coef_q28, "ohgpu_src_pull_create");
    if (err != OHGPU_OK) return err;
    ohgpu_src* s = new (std::nothrow) ohgpu_src();
    if (!s) return set_error(OHGPU_ERR_NOMEM, "ohgpu_src_pull_create: out of host memory");
    s->T = T;
    s->pulled = true;
    s->phases_log2 = phases_log2;
    const size_t bytes = (size_t)((1u << phases_log2) + 1u) * T * sizeof(int32_t);
    hipError_t e = hipMalloc((void**)&s->d_pull_table, bytes);
    if (e == hipSuccess) e = hipMemcpy(s->d_pull_table, coef_q28, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (s->d_pull_table) (void)hipFree(s->d_pull_table);
        delete s;
        return set_error(OHGPU_ERR_DEVICE, "ohgpu_src_pull_create: %s", hipGetErrorString(e));
    }
    *out = s;
    return OHGPU_OK;
}

int ohgpu_src_pull_destroy(ohgpu_ctx* ctx, ohgpu_src* src)
{
    CTX_GUARD("ohgpu_src_pull_destroy");
    if (!src) return OHGPU_OK;
    if (!src->pulled) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_destroy: not a pulled filter");
    (void)hipFree(src->d_pull_table);
    delete src;
    return OHGPU_OK;
}

int ohgpu_src_pull_batch_create(ohgpu_ctx* ctx, const ohgpu_src* src, const ohgpu_src_pull_msg_desc* descs, size_t n,
                                uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_src_pull_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_src_pull_batch_create", kBatchSrcPull, src && (descs || !n), n, 0xffffffffull, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err != OHGPU_OK) return err;
    if (!src->pulled) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_batch_create: not a pulled filter (ohgpu_src_pull_create)");
    b->src = src;
    b->uniform = true;
    const uint32_t T = src->T;
    for (size_t i = 0; i < n; i++) {
        err = check_pull_desc(descs[i], i, T, src_arena_bytes, dst_arena_bytes, b.get());
        if (err != OHGPU_OK) return err;
        if (i == 0) b->channels = descs[0].channels;
        else if (descs[i].channels != b->channels) b->uniform = false;
    }
    // the tiles: up to kPullTile consecutive outputs whose window (T - 1 frames of history and the frames they advance over) fits
    // the LDS window: (count - 1) * step + frac0 < (cap_frames - T + 1) * 2^32
    std::vector<PullTile> tiles;
    for (size_t i = 0; i < n; i++) {
        const ohgpu_src_pull_msg_desc& d = descs[i];
        const uint64_t cap_frames = src_pull_window_cap(T) / d.channels;
        for (uint32_t j0 = 0; j0 < d.n_frames;) {
            const uint64_t u0 = (uint64_t)d.pos_frac + (uint64_t)j0 * d.step;
            const uint64_t frac0 = u0 & 0xffffffffull;
            const uint64_t room = ((cap_frames - T + 1) << 32) - frac0 - 1;
            uint64_t count = room / d.step + 1;
            count = std::min<uint64_t>(std::min<uint64_t>(count, kPullTile), d.n_frames - j0);
            const uint64_t n_first = d.pos_frame + (u0 >> 32);
            const uint64_t n_last = d.pos_frame + (((uint64_t)d.pos_frac + (uint64_t)(j0 + count - 1) * d.step) >> 32);
            PullTile t;
            t.msg = (uint32_t)i;
            t.j0 = j0;
            t.count = (uint32_t)count;
            t.win_first = (int64_t)n_first - (int64_t)(T - 1);
            t.win_frames = (uint32_t)((int64_t)n_last - t.win_first + 1);
            t.reserved = 0;
            tiles.push_back(t);
            j0 += (uint32_t)count;
        }
    }
    if (tiles.size() > 0xffffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_pull_batch_create: too many tiles");
    err = upload_batch(ctx, b.get(), descs, n * sizeof(ohgpu_src_pull_msg_desc));
    if (err == OHGPU_OK && !tiles.empty()) {
        hipError_t e = ctx_dev_alloc(ctx, &b->d_pull_tiles, tiles.size() * sizeof(PullTile));
        if (e == hipSuccess) e = hipMemcpy(b->d_pull_tiles, tiles.data(), tiles.size() * sizeof(PullTile), hipMemcpyHostToDevice);
        if (e != hipSuccess) err = set_error(hip_code(e), "ohgpu_src_pull_batch_create: tile upload: %s", hipGetErrorString(e));
    }
    b->n_pull_tiles = (uint32_t)tiles.size();
    return batch_done(err, b, out);
}

int ohgpu_src_pull_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_src_pull_batch_run", batch, kBatchSrcPull, batch && batch->n_pull_tiles == 0, false, src_base, dst_base);
    if (go <= 0) return go;
    OHGPU_HIP_TRY(launch_src_pull(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_src_pull_process_host(ohgpu_ctx* ctx, const ohgpu_src* src, const ohgpu_src_pull_msg_desc* descs, size_t n,
                                const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes)
{
    CTX_GUARD("ohgpu_src_pull_process_host");
    ohgpu_batch* b = nullptr;
    const int err = ohgpu_src_pull_batch_create(ctx, src, descs, n, src_bytes, dst_bytes, &b);
    if (err != OHGPU_OK) return err;
    ctx->stage.src_calls++;
    return process_host(ctx, b, n, src_host, src_bytes, dst_host, dst_bytes, ohgpu_src_pull_batch_run, [&](size_t i) { return frames_range(descs[i]); });
}

}  // extern "C"
