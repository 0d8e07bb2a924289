// api_dsd_pcm.hip -- the C ABI's DSD -> PCM converter (ohgpu_dsd_pcm_*).
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

extern "C" {

// the chunks output frames [out0, out0 + n) read: bits (out0 + 1) * D - N .. (out0 + n) * D - 1, those below zero left out
static void pcm_window(uint64_t out0, uint32_t n, uint32_t D, uint32_t N, uint64_t* lo, uint64_t* hi)
{
    const int64_t first = (int64_t)((out0 + 1) * D) - (int64_t)N, last = (int64_t)((out0 + n) * D) - 1;
    *lo = first < 0 ? 0 : (uint64_t)first >> 4;
    *hi = ((uint64_t)last >> 4) + 1;
}

// one message against the rules of ohgpu.h (ohgpu_dsd_pcm_msg_desc); on success its share of the batch's totals
static int check_dsd_pcm_desc(const ohgpu_dsd_pcm_msg_desc& d, size_t i, uint32_t D, uint32_t N, uint64_t src_arena, uint64_t dst_arena, ohgpu_batch* b)
{
    const uint32_t W = d.sample_block_words, P = d.pad_bytes_per_chunk;
    if (!valid_dsd_format(W, P))
        return set_error(OHGPU_ERR_INVALID, "dsd pcm desc %zu: sample block of %u words with %u pad bytes per chunk (P == 0, or W == P + 4 with P even)", i, W, P);
    if (!valid_endian(d.dst_endian)) return set_error(OHGPU_ERR_INVALID, "dsd pcm desc %zu: byte order %u", i, d.dst_endian);
    if (d.flags & ~OHGPU_FLAG_RAMP) return set_error(OHGPU_ERR_INVALID, "dsd pcm desc %zu: flag bits 0x%x not valid for a converted message", i, d.flags);
    for (size_t k = 0; k < sizeof(d.reserved); k++)
        if (d.reserved[k]) return set_error(OHGPU_ERR_INVALID, "dsd pcm desc %zu: reserved bytes must be zero", i);
    if (d.ramp_start > OHGPU_RAMP_MAX || d.ramp_end > OHGPU_RAMP_MAX) return set_error(OHGPU_ERR_INVALID, "dsd pcm desc %zu: ramp beyond Ramp::kMax", i);
    if ((d.flags & OHGPU_FLAG_RAMP) && d.n_frames > 131071u) return set_error(OHGPU_ERR_INVALID, "dsd pcm desc %zu: ramped message of %u frames", i, d.n_frames);
    if (d.out_frame0 > (1ull << 40) || d.src_chunk0 > (1ull << 48) || d.src_chunks > (1ull << 40))
        return set_error(OHGPU_ERR_INVALID, "dsd pcm desc %zu: frame or chunk index out of range", i);
    if (d.n_frames == 0) return OHGPU_OK;
    const uint64_t cs = 4u + P, dst_bytes = (uint64_t)d.n_frames * 6u;
    int span = arena_span("dsd pcm desc", i, "input window", d.src_offset, d.src_chunks * cs, src_arena, "source");
    if (span == OHGPU_OK) span = arena_span("dsd pcm desc", i, "writes", d.dst_offset, dst_bytes, dst_arena, "destination");
    if (span != OHGPU_OK) return span;
    uint64_t lo = 0, hi = 0;
    pcm_window(d.out_frame0, d.n_frames, D, N, &lo, &hi);
    if (lo < d.src_chunk0 || hi > d.src_chunk0 + d.src_chunks)
        return set_error(OHGPU_ERR_INVALID, "dsd pcm desc %zu: reads chunks [%llu, %llu) but the buffer holds [%llu, %llu)", i, (unsigned long long)lo,
                         (unsigned long long)hi, (unsigned long long)d.src_chunk0, (unsigned long long)(d.src_chunk0 + d.src_chunks));
    if (!b) return OHGPU_OK;
    b->in_frames += hi - lo;
    b->out_frames += d.n_frames;
    b->src_bytes_touched += (hi - lo) * cs;
    b->dst_bytes_written += dst_bytes;
    if (d.n_frames > b->max_frames) b->max_frames = d.n_frames;
    return OHGPU_OK;
}

int ohgpu_dsd_pcm_design(uint32_t dsd_rate, uint32_t pcm_rate, uint32_t T, double beta, double f_pass_hz, double gain,
                         int32_t* coef_q28, size_t coef_capacity, uint32_t* decimation)
{
    if (!decimation) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_pcm_design: null result");
    std::vector<int32_t> coef;
    const int err = design_dsd_pcm(dsd_rate, pcm_rate, T, beta, f_pass_hz, gain, coef_q28 ? &coef : nullptr, decimation);
    if (err != OHGPU_OK || !coef_q28) return err;
    if (coef.size() > coef_capacity)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_pcm_design: capacity %zu < D * T = %zu", coef_capacity, coef.size());
    memcpy(coef_q28, coef.data(), coef.size() * sizeof(int32_t));
    return OHGPU_OK;
}

int ohgpu_dsd_pcm_window(uint64_t out_frame0, uint32_t n_frames, uint32_t D, uint32_t T, uint64_t* chunk_lo, uint64_t* chunk_hi)
{
    if (!chunk_lo || !chunk_hi || n_frames == 0 || out_frame0 > (1ull << 40))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_pcm_window: null result, no frames or an out_frame0 beyond 2^40");
    const int err = check_dsd_pcm_filter(D, T, nullptr, "ohgpu_dsd_pcm_window");
    if (err != OHGPU_OK) return err;
    pcm_window(out_frame0, n_frames, D, D * T, chunk_lo, chunk_hi);
    return OHGPU_OK;
}

int ohgpu_dsd_pcm_batch_check(uint32_t D, uint32_t T, const ohgpu_dsd_pcm_msg_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (!descs && n) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_pcm_batch_check: null argument");
    int err = check_dsd_pcm_filter(D, T, nullptr, "ohgpu_dsd_pcm_batch_check");
    for (size_t i = 0; i < n && err == OHGPU_OK; i++) err = check_dsd_pcm_desc(descs[i], i, D, D * T, src_arena_bytes, dst_arena_bytes, nullptr);
    return err;
}

int ohgpu_dsd_pcm_create(ohgpu_ctx* ctx, uint32_t D, uint32_t T, const int32_t* coef_q28, ohgpu_dsd_pcm** out)
{
    CTX_GUARD("ohgpu_dsd_pcm_create");
    if (!out || !coef_q28) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_pcm_create: null argument");
    *out = nullptr;
    const int err = check_dsd_pcm_filter(D, T, coef_q28, "ohgpu_dsd_pcm_create");
    if (err != OHGPU_OK) return err;
    ohgpu_dsd_pcm* f = new (std::nothrow) ohgpu_dsd_pcm();
    if (!f) return set_error(OHGPU_ERR_NOMEM, "ohgpu_dsd_pcm_create: out of host memory");
    f->D = D; f->T = T; f->N = D * T;
    hipError_t e = hipMalloc((void**)&f->d_coef, f->N * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(f->d_coef, coef_q28, f->N * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && f->N <= kDsdPcmTableTaps) {
        std::vector<int32_t> tables;
        build_dsd_pcm_tables(coef_q28, f->N, &tables);
        e = hipMalloc((void**)&f->d_tables, tables.size() * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemcpy(f->d_tables, tables.data(), tables.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        if (f->d_coef) (void)hipFree(f->d_coef);
        if (f->d_tables) (void)hipFree(f->d_tables);
        delete f;
        return set_error(hip_code(e), "ohgpu_dsd_pcm_create: %s", hipGetErrorString(e));
    }
    *out = f;
    return OHGPU_OK;
}

int ohgpu_dsd_pcm_destroy(ohgpu_ctx* ctx, ohgpu_dsd_pcm* f)
{
    CTX_GUARD("ohgpu_dsd_pcm_destroy");
    if (!f) return OHGPU_OK;
    (void)hipFree(f->d_coef);
    if (f->d_tables) (void)hipFree(f->d_tables);
    delete f;
    return OHGPU_OK;
}

int ohgpu_dsd_pcm_batch_create(ohgpu_ctx* ctx, const ohgpu_dsd_pcm* filter, const ohgpu_dsd_pcm_msg_desc* descs, size_t n,
                               uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_dsd_pcm_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_dsd_pcm_batch_create", kBatchDsdPcm, filter && (descs || !n), n, 0xffffffffull, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err != OHGPU_OK) return err;
    b->dsdpcm_filter = filter;
    for (size_t i = 0; i < n; i++) {
        err = check_dsd_pcm_desc(descs[i], i, filter->D, filter->N, src_arena_bytes, dst_arena_bytes, b.get());
        if (err != OHGPU_OK) return err;
    }
    err = upload_batch(ctx, b.get(), descs, n * sizeof(ohgpu_dsd_pcm_msg_desc));
    if (err == OHGPU_OK) err = plan_dsd_pcm(ctx, b.get(), descs, n);
    return batch_done(err, b, out);
}

int ohgpu_dsd_pcm_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_dsd_pcm_batch_run", batch, kBatchDsdPcm, batch && batch->dsdpcm.n_tiles == 0, false, src_base, dst_base);
    if (go <= 0) return go;
    if (batch->dsdpcm.fast && ctx->variant != 1) OHGPU_HIP_TRY(launch_dsd_pcm_table(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream)));
    else OHGPU_HIP_TRY(launch_dsd_pcm_v1(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream)));
    return OHGPU_OK;
}

int ohgpu_dsd_pcm_batch_paths(const ohgpu_batch* b, uint32_t* fast_descs, uint32_t* plain_descs, uint32_t* launches)
{
    if (!b || b->kind != kBatchDsdPcm) return set_error(OHGPU_ERR_INVALID, "ohgpu_dsd_pcm_batch_paths: not a DSD to PCM batch");
    if (fast_descs) *fast_descs = b->dsdpcm.n_fast;
    if (plain_descs) *plain_descs = b->dsdpcm.n_plain;
    if (launches) *launches = b->dsdpcm.n_tiles ? 1u : 0u;
    return OHGPU_OK;
}

int ohgpu_dsd_pcm_process_host(ohgpu_ctx* ctx, const ohgpu_dsd_pcm* filter, const ohgpu_dsd_pcm_msg_desc* descs, size_t n,
                               const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes)
{
    CTX_GUARD("ohgpu_dsd_pcm_process_host");
    ohgpu_batch* b = nullptr;
    const int err = ohgpu_dsd_pcm_batch_create(ctx, filter, descs, n, src_bytes, dst_bytes, &b);
    if (err != OHGPU_OK) return err;
    return process_host(ctx, b, n, src_host, src_bytes, dst_host, dst_bytes, ohgpu_dsd_pcm_batch_run,
                        [&](size_t i) { return std::make_pair(descs[i].dst_offset, (uint64_t)descs[i].n_frames * 6u); });
}

}  // extern "C"
