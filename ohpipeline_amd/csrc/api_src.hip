// api_src.hip -- the C ABI's fixed-ratio sample-rate converter (ohgpu_src_*): filters, checks, plans, launches.
#include <cstring>
#include <string>

#include "api_common.h"
#include "src_mfma_common.h"
#include "src_plan.h"

namespace ohgpu {

// What the planner and the dispatch look at in a filter, from its coefficients alone (no device): the exactness bound's figure, the
// half-band structure, and whether the matrix-pipe kernels' tables exist for it (and which).  ohgpu_src_create and
// ohgpu_src_plan_digest both come through here, so that the digest's plan IS the plan.  Returns false with the error set.
struct SrcTables { std::vector<uint8_t> amat; std::vector<MfStep> steps; bool made = false; };
static bool src_describe(uint32_t L, uint32_t M, uint32_t T, const int32_t* coef_q28, ohgpu_src* s, SrcTables* tables, const char* who)
{
    int64_t max_sum_abs = 0;
    for (uint32_t p = 0; p < L; p++) {
        int64_t sabs = 0;
        for (uint32_t k = 0; k < T; k++) {
            const int32_t q = coef_q28[(size_t)p * T + k];
            sabs += q < 0 ? -(int64_t)q : (int64_t)q;
        }
        if (sabs > max_sum_abs) max_sum_abs = sabs;
        if (sabs >= ((int64_t)1 << 30)) {
            set_error(OHGPU_ERR_INVALID, "%s: phase %u has sum|c| = %lld >= 2^30 (exact fp64 accumulation bound)", who, p, (long long)sabs);
            return false;
        }
    }
    s->L = L; s->M = M; s->T = T;
    s->max_sum_abs = max_sum_abs;
    // a half-band 2:1 decimator (what ohgpu_src_design makes for 96 -> 48 kHz): of its odd taps only the centre one is not zero
    s->halfband = L == 1 && M == 2 && T == 64 && coef_q28[T - 1] == 0;
    for (uint32_t k = 1; k < T && s->halfband; k += 2)
        if (k != T / 2 - 1 && coef_q28[k] != 0) s->halfband = false;
    // the matrix-pipe kernels' digit tables, for the block length the planner gives 24-bit stereo output (rows of up to 8 blocks)
    const uint32_t mf_L_blk = (T == 32 || s->halfband) ? src_block_outputs(L, 6) : 0;
    std::vector<uint8_t> adig;
    s->mf_halfband = false;
    s->mf_L_blk = 0;
    if (mf_L_blk != 0 && s->halfband) {
        tables->made = build_mfma_halfband(coef_q28, mf_L_blk, &tables->steps, &tables->amat);
        s->mf_halfband = tables->made;
    } else if (mf_L_blk != 0 && build_mfma_tables(L, M, T, coef_q28, mf_L_blk, 8, &adig, &tables->steps)) {
        build_mfma_images(adig, tables->steps, L, &tables->amat);
        tables->made = true;
    }
    if (tables->made) s->mf_L_blk = mf_L_blk;
    return true;
}

// messages [lo, hi) of a resampled batch: validation (ohgpu.h: ohgpu_src_msg_desc), the batch's totals, whether they come in the
// planner's order (a message against its predecessor: src_msg_before) -- and, where `dev` is given, the generic kernel's form of each
void src_check_range(const ohgpu_src* src, const ohgpu_src_msg_desc* descs, size_t lo_i, size_t hi_i, uint64_t src_arena_bytes,
                     uint64_t dst_arena_bytes, DevSrcDesc* dev, SrcRangeResult* out)
{
    SrcRangeResult& r = *out;
    const uint64_t L = src->L, M = src->M, T = src->T;
    const FastDiv64 by_L(L);
    const ohgpu_src_msg_desc& d0 = descs[0];
    for (size_t i = lo_i; i < hi_i; i++) {
        const ohgpu_src_msg_desc& d = descs[i];
        int err = OHGPU_OK;
        if (d.channels < 1 || d.channels > OHGPU_MAX_CHANNELS) err = set_error(OHGPU_ERR_INVALID, "src desc %zu: channels %u outside 1..8", i, d.channels);
        else if (!valid_bits(d.src_bits) || !valid_bits(d.dst_bits)) err = set_error(OHGPU_ERR_INVALID, "src desc %zu: bit depth %u -> %u", i, d.src_bits, d.dst_bits);
        else if (!valid_endian(d.src_endian) || !valid_endian(d.dst_endian)) err = set_error(OHGPU_ERR_INVALID, "src desc %zu: endian %u -> %u", i, d.src_endian, d.dst_endian);
        else if (d.flags & ~(OHGPU_FLAG_RAMP | OHGPU_FLAG_ZERO_LSB32 | OHGPU_FLAG_SRC_PLANAR32)) err = set_error(OHGPU_ERR_INVALID, "src desc %zu: flag bits 0x%x not valid for a resampled message", i, d.flags);
        else if (!(d.flags & OHGPU_FLAG_SRC_PLANAR32) && d.src_plane_stride != 0) err = set_error(OHGPU_ERR_INVALID, "src desc %zu: src_plane_stride without OHGPU_FLAG_SRC_PLANAR32", i);
        else if ((d.flags & OHGPU_FLAG_SRC_PLANAR32) && (d.src_bits == 32 || (d.src_offset & 3) || (d.src_plane_stride & 3) || (d.src_plane_stride >> 34)))
            err = set_error(OHGPU_ERR_INVALID, "src desc %zu: planar source needs 8/16/24-bit samples, 4-byte aligned planes less than 16 GiB apart", i);
        else if (d.ramp_start > OHGPU_RAMP_MAX || d.ramp_end > OHGPU_RAMP_MAX) err = set_error(OHGPU_ERR_INVALID, "src desc %zu: ramp beyond Ramp::kMax", i);
        else if ((d.flags & OHGPU_FLAG_RAMP) && d.n_frames > 131071u) err = set_error(OHGPU_ERR_INVALID, "src desc %zu: ramped message of %u frames", i, d.n_frames);
        else if (d.attenuation != OHGPU_UNITY_ATTENUATION) err = set_error(OHGPU_ERR_UNSUPPORTED, "src desc %zu: attenuation %u (resampled audio is 24-bit; Msg.cpp:2741 allows 16-bit only)", i, d.attenuation);
        else if (d.out_frame0 > (1ull << 48) || d.src_frame0 > (1ull << 48) || d.src_frames > (1ull << 40)) err = set_error(OHGPU_ERR_INVALID, "src desc %zu: frame index out of range", i);
        if (err != OHGPU_OK) { r.fail(err); return; }
        const uint64_t fb_src = (uint64_t)d.channels * (d.src_bits / 8);
        const uint64_t fb_dst = (uint64_t)d.channels * (d.dst_bits / 8);
        const bool planar = (d.flags & OHGPU_FLAG_SRC_PLANAR32) != 0;
        // (planar: the window is one run of src_frames * 4 bytes per plane; the last plane's run ends furthest out -- span_end
        // is overflow-safe, see the fmt batches)
        const uint64_t src_bytes = planar ? d.src_frames * 4 : d.src_frames * fb_src;
        const uint64_t dst_bytes = (uint64_t)d.n_frames * fb_dst;
        uint64_t planes_end = 0;
        if (planar && (!span_end(d.src_offset, d.src_plane_stride, d.channels - 1u, src_bytes, &planes_end) || planes_end > src_arena_bytes ||
                       (d.channels > 1 && d.src_plane_stride < src_bytes))) {
            r.fail(set_error(OHGPU_ERR_BOUNDS, "src desc %zu: %u planes of %llu bytes, %llu apart from %llu, beyond the %llu-byte source arena (or overlapping)", i,
                             d.channels, (unsigned long long)src_bytes, (unsigned long long)d.src_plane_stride, (unsigned long long)d.src_offset,
                             (unsigned long long)src_arena_bytes));
            return;
        }
        err = arena_span("src desc", i, "input window", d.src_offset, src_bytes, src_arena_bytes, "source");
        if (err == OHGPU_OK) err = arena_span("src desc", i, "writes", d.dst_offset, dst_bytes, dst_arena_bytes, "destination");
        if (err != OHGPU_OK) { r.fail(err); return; }
        if (d.n_frames > 0) {
            const uint64_t t_first = d.out_frame0 * M, t_last = (d.out_frame0 + d.n_frames - 1) * M;
            const int64_t n0_first = (int64_t)by_L.div(t_first), n0_last = (int64_t)by_L.div(t_last);
            const int64_t n_lo = n0_first - (int64_t)(T - 1);
            if (n_lo >= 0 ? (uint64_t)n_lo < d.src_frame0 : d.src_frame0 != 0) {
                r.fail(set_error(OHGPU_ERR_BOUNDS, "src desc %zu: filter history starts at input frame %lld but the buffer starts at %llu", i,
                                 (long long)(n_lo < 0 ? 0 : n_lo), (unsigned long long)d.src_frame0));
                return;
            }
            if ((uint64_t)n0_last >= d.src_frame0 + d.src_frames) {
                r.fail(set_error(OHGPU_ERR_BOUNDS, "src desc %zu: needs input frame %lld but the buffer ends at %llu", i,
                                 (long long)n0_last, (unsigned long long)(d.src_frame0 + d.src_frames)));
                return;
            }
            const int64_t lo = n_lo < 0 ? 0 : n_lo;
            r.in_frames += (uint64_t)(n0_last - n0_first + 1);   // new input frames this message advances over
            r.src_bytes_touched += (uint64_t)(n0_last - lo + 1) * (planar ? 4ull * d.channels : fb_src);
        }
        if (dev) dev[i] = src_convert_desc(d, L, M);
        r.out_frames += d.n_frames;
        r.dst_bytes_written += dst_bytes;
        if (d.n_frames > r.max_frames) r.max_frames = d.n_frames;
        if (d.channels != d0.channels || d.src_bits != d0.src_bits || d.src_endian != d0.src_endian || d.dst_bits != d0.dst_bits ||
            d.dst_endian != d0.dst_endian || planar != ((d0.flags & OHGPU_FLAG_SRC_PLANAR32) != 0)) r.uniform = false;
        // (the planner's order, message against predecessor -- the range's first against the last of the range before it: a caller
        // that lists its streams one after the other, each in time order, spares the planner its own pass and the sort)
        if (i > 0 && r.ordered && src_msg_before(descs[i], descs[i - 1], planar ? 4u : (uint32_t)fb_src, (uint32_t)fb_dst)) r.ordered = false;
    }
}

// A resampled batch's messages checked and -- if they share a layout -- planned (b->fast), by the shorter of two routes; the batch's
// totals, `uniform` and layout fields are set.  `dev`: where to put the generic kernel's form of every message (null: nowhere).
// `digest`: the plan hashed instead of uploaded (ohgpu_src_plan_digest: ctx has no device behind it).
int src_check_and_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const ohgpu_src_msg_desc* descs, size_t n, DevSrcDesc* dev, PlanDigest* digest)
{
    const ohgpu_src* src = b->src;
    auto layout_of_first = [&] {
        const ohgpu_src_msg_desc& d0 = descs[0];
        b->channels = d0.channels; b->src_bits = d0.src_bits; b->src_endian = d0.src_endian;
        b->dst_bits = d0.dst_bits; b->dst_endian = d0.dst_endian;
        b->src_planar = (d0.flags & OHGPU_FLAG_SRC_PLANAR32) != 0;
    };
    // A large batch is 64 bytes a message to read -- 32 MB for the headline's half a million -- and both the checks and the planner's
    // cut into segments are bound by exactly that.  So the planner is let loose on the messages FIRST, on the usual caller's terms
    // (one layout, streams one after the other in time order), and checks each message itself the first time it looks at it; a batch
    // that is not what it assumed -- several layouts, another order, a layout no block kernel has -- goes the two-pass way below.
    if (!dev && n >= 4096) {
        SrcRangeResult first;
        src_check_range(src, descs, 0, 1, b->src_arena_bytes, b->dst_arena_bytes, nullptr, &first);      // (its layout is the batch's: the planner's geometry needs it sane)
        if (first.err != OHGPU_OK) return set_error(first.err, "%s", first.msg);
        layout_of_first();
        PlanFusedCheck fused;
        fused.src = src;
        const int err = plan_src_fast(ctx, b, descs, n, true, digest, &fused);
        if (err != OHGPU_OK) return err;
        if (fused.checked && fused.total.err != OHGPU_OK) return set_error(fused.total.err, "%s", fused.total.msg);
        if (fused.checked && !fused.retry) {
            b->in_frames = fused.total.in_frames; b->out_frames = fused.total.out_frames;
            b->src_bytes_touched = fused.total.src_bytes_touched; b->dst_bytes_written = fused.total.dst_bytes_written;
            b->max_frames = fused.total.max_frames;
            return OHGPU_OK;                                 // (checked and uniform; a plan, or none: no whole block anywhere -- the generic kernel's batch)
        }
    }
    // every message checked on its own: in ranges, on as many threads as the batch is worth (the first error in message order is the
    // one reported); then the plan
    bool ordered = true;
    {
        const unsigned n_thr = plan_threads(n, 16384);
        std::vector<SrcRangeResult> res(n_thr);
        parallel_ranges(n, n_thr, [&](unsigned t, size_t lo, size_t hi) { src_check_range(src, descs, lo, hi, b->src_arena_bytes, b->dst_arena_bytes, dev, &res[t]); });
        b->in_frames = b->out_frames = b->src_bytes_touched = b->dst_bytes_written = 0;
        b->max_frames = 0;
        b->uniform = true;
        for (const SrcRangeResult& r : res) {
            if (r.err != OHGPU_OK) return set_error(r.err, "%s", r.msg);
            b->in_frames += r.in_frames; b->out_frames += r.out_frames;
            b->src_bytes_touched += r.src_bytes_touched; b->dst_bytes_written += r.dst_bytes_written;
            if (r.max_frames > b->max_frames) b->max_frames = r.max_frames;
            b->uniform = b->uniform && r.uniform;
            ordered = ordered && r.ordered;
        }
        if (n > 0) layout_of_first();
    }
    int err = OHGPU_OK;
    if (b->uniform && n > 0) err = plan_src_fast(ctx, b, descs, n, ordered, digest);
    return err;
}

// Which kernel runs a (uniform) resampled batch's whole blocks: ONE decision, taken from the plan (what it serves: made under the
// variant in force at creation) and the variant in force NOW, and used by the launch and by the name a benchmark prints alike.
enum SrcKernel { kSrcGeneric, kSrcWg, kSrcLean, kSrcBlock };
static SrcKernel src_kernel_choice(const ohgpu_ctx* ctx, const ohgpu_batch* b, bool arena_aligned = true)
{
    const int v = ctx->variant;
    // (the block kernels' staging moves aligned 16-byte pieces of the arena; a plan for the workgroup kernel alone has nothing for
    // a variant that asks for another)
    if (v == 1 || !b->fast.enabled || !arena_aligned || (b->fast.wg_only && v != 0)) return kSrcGeneric;
    if (b->fast.mfma_wg && v == 0) return kSrcWg;                                         // the taps on the matrix pipe (round 4), a unit per workgroup
    if (b->fast.lean) return kSrcLean;                                                     // round 2's, under every other variant
    if (b->fast.d_work) return kSrcBlock;                                                  // round 1's: the fallback for a filter beyond the lean kernel's rounding bound
    return kSrcGeneric;
}
static const char* src_kernel_name(SrcKernel k)
{
    switch (k) {
    case kSrcWg: return "src_mfma_wg_kernel";
    case kSrcLean: return "src_lean_kernel";
    case kSrcBlock: return "src_block_kernel";
    default: return "src_kernel_v1";
    }
}
static const char* src_kernel_of(const ohgpu_ctx* ctx, const ohgpu_batch* b) { return src_kernel_name(src_kernel_choice(ctx, b)); }

}  // namespace ohgpu

using namespace ohgpu;

extern "C" {

int ohgpu_src_design(uint32_t rate_in, uint32_t rate_out, uint32_t taps_per_phase, double beta, double f_pass_hz,
                     int32_t* coef_q28, size_t coef_capacity, uint32_t* L, uint32_t* M)
{
    if (!L || !M) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_design: null L/M");
    if (!coef_q28) return design_src(rate_in, rate_out, taps_per_phase, beta, f_pass_hz, nullptr, L, M);
    std::vector<int32_t> coef;
    const int err = design_src(rate_in, rate_out, taps_per_phase, beta, f_pass_hz, &coef, L, M);
    if (err != OHGPU_OK) return err;
    if (coef.size() > coef_capacity)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_src_design: capacity %zu < L*T = %zu", coef_capacity, coef.size());
    memcpy(coef_q28, coef.data(), coef.size() * sizeof(int32_t));
    return OHGPU_OK;
}

uint64_t ohgpu_src_out_frames(uint32_t L, uint32_t M, uint64_t in_frames)
{
    if (in_frames == 0 || M == 0) return 0;
    return (in_frames * L + M - 1) / M;
}

int ohgpu_src_mfma_tables(uint32_t L, uint32_t M, uint32_t T, const int32_t* coef_q28, uint32_t max_blocks_per_row,
                          uint8_t* coef_digits, size_t coef_digits_capacity, void* steps_out, size_t steps_capacity,
                          size_t* coef_digits_bytes, size_t* steps_bytes, uint32_t* block_outputs)
{
    if (!coef_q28 || L == 0 || M == 0 || (uint64_t)L * T > (1u << 22) || max_blocks_per_row == 0 || max_blocks_per_row > 64)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_src_mfma_tables: bad argument");
    std::vector<uint8_t> adig;
    std::vector<MfStep> steps;
    const uint32_t L_blk = T == 32 ? src_block_outputs(L, 6) : 0;
    if (L_blk == 0 || !build_mfma_tables(L, M, T, coef_q28, L_blk, max_blocks_per_row, &adig, &steps))
        return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_mfma_tables: L=%u M=%u T=%u does not fit the 16-output tiling", L, M, T);
    if (coef_digits_bytes) *coef_digits_bytes = adig.size();
    if (steps_bytes) *steps_bytes = steps.size() * sizeof(MfStep);
    if (block_outputs) *block_outputs = L_blk;
    if (coef_digits) {
        if (coef_digits_capacity < adig.size()) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_mfma_tables: coef_digits too small");
        memcpy(coef_digits, adig.data(), adig.size());
    }
    if (steps_out) {
        if (steps_capacity < steps.size() * sizeof(MfStep)) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_mfma_tables: steps too small");
        memcpy(steps_out, steps.data(), steps.size() * sizeof(MfStep));
    }
    return OHGPU_OK;
}

int ohgpu_src_mfma_halfband_tables(const int32_t* coef_q28, uint8_t* image, int64_t* bias, uint32_t* block_outputs)
{
    if (!coef_q28 || !image) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_mfma_halfband_tables: null argument");
    const uint32_t L_blk = src_block_outputs(1, 6);
    std::vector<MfStep> steps;
    std::vector<uint8_t> amat;
    if (L_blk == 0 || !build_mfma_halfband(coef_q28, L_blk, &steps, &amat) || steps.empty())
        return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_mfma_halfband_tables: not a half-band decimator of 64 taps");
    memcpy(image, amat.data(), kMfStepImage);
    // (the steps carry the bias in pieces, the same for every output: bits 0..15 and, signed, bits 16..)
    if (bias) *bias = (int64_t)steps[0].b0[0] + ((int64_t)(int32_t)steps[0].b1[0]) * 65536 + ((int64_t)(int32_t)steps[0].b2[0]) * 4294967296ll;
    if (block_outputs) *block_outputs = L_blk;
    return OHGPU_OK;
}

int ohgpu_src_create(ohgpu_ctx* ctx, uint32_t L, uint32_t M, uint32_t T, const int32_t* coef_q28, ohgpu_src** out)
{
    CTX_GUARD("ohgpu_src_create");
    if (!out || !coef_q28) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_create: null argument");
    *out = nullptr;
    // (M < 2^15: a descriptor's out_frame0 may be 2^48, and out_frame0 * M is computed in 64 bits)
    if (L == 0 || M == 0 || M >= (1u << 15) || T == 0 || (uint64_t)L * T > (1u << 22))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_src_create: bad geometry L=%u M=%u T=%u", L, M, T);
    const size_t n = (size_t)L * T;
    ohgpu_src* s = new (std::nothrow) ohgpu_src();
    if (!s) return set_error(OHGPU_ERR_NOMEM, "ohgpu_src_create: out of host memory");
    SrcTables tables;
    if (!src_describe(L, M, T, coef_q28, s, &tables, "ohgpu_src_create")) { delete s; return OHGPU_ERR_INVALID; }
    std::vector<double> cd(n);
    for (size_t i = 0; i < n; i++) cd[i] = (double)coef_q28[i];
    hipError_t e = hipMalloc((void**)&s->d_coef, n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&s->d_coef_q28, n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(s->d_coef, cd.data(), n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_coef_q28, coef_q28, n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && tables.made) {
        e = hipMalloc((void**)&s->d_mf_amat, tables.amat.size());
        if (e == hipSuccess) e = hipMalloc((void**)&s->d_mf_steps, tables.steps.size() * sizeof(MfStep));
        if (e == hipSuccess) e = hipMemcpy(s->d_mf_amat, tables.amat.data(), tables.amat.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->d_mf_steps, tables.steps.data(), tables.steps.size() * sizeof(MfStep), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        if (s->d_coef) hipFree(s->d_coef);
        if (s->d_coef_q28) hipFree(s->d_coef_q28);
        if (s->d_mf_amat) hipFree(s->d_mf_amat);
        if (s->d_mf_steps) hipFree(s->d_mf_steps);
        delete s;
        return set_error(OHGPU_ERR_DEVICE, "ohgpu_src_create: %s", hipGetErrorString(e));
    }
    *out = s;
    return OHGPU_OK;
}

int ohgpu_src_destroy(ohgpu_ctx* ctx, ohgpu_src* src)
{
    CTX_GUARD("ohgpu_src_destroy");
    if (!src) return OHGPU_OK;
    if (src->pulled) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_destroy: a pulled filter is destroyed with ohgpu_src_pull_destroy");
    hipFree(src->d_coef);
    hipFree(src->d_coef_q28);
    if (src->d_mf_amat) hipFree(src->d_mf_amat);
    if (src->d_mf_steps) hipFree(src->d_mf_steps);
    delete src;
    return OHGPU_OK;
}

int ohgpu_src_batch_create(ohgpu_ctx* ctx, const ohgpu_src* src, const ohgpu_src_msg_desc* descs, size_t n,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_src_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_src_batch_create", kBatchSrc, src && (descs || !n), n, 0xffffffffull, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err != OHGPU_OK) return err;
    if (src->pulled) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_create: a pulled filter (ohgpu_src_pull_create) runs through ohgpu_src_pull_batch_create");
    b->src = src;
    b->uniform = true;
    // The generic kernel's per-message form (56 bytes a message: 28 MB written for the headline's half a million, half of a checking
    // pass's time) is made only where that kernel will run the whole batch: a batch created while variant 1 is in force, or one no
    // block kernel takes (below).  A batch planned for the block kernels keeps nothing per message.
    const bool keep_generic = ctx->variant == 1;
    auto convert_all = [&]() -> bool {
        b->host_descs.reset((DevSrcDesc*)host_alloc_huge((n ? n : 1) * sizeof(DevSrcDesc)));     // (not zeroed here: the ranges' threads touch their own pages)
        return b->host_descs != nullptr;
    };
    if (keep_generic && !convert_all()) return set_error(OHGPU_ERR_NOMEM, "ohgpu_src_batch_create: out of host memory");
    err = src_check_and_plan(ctx, b.get(), descs, n, b->host_descs.get(), nullptr);
    if (err != OHGPU_OK) return err;
    if (!b->uniform) {
        // Mixed layouts (channel counts, depths, byte orders, planar or packed sources): the block kernels are instantiated per
        // layout, so the batch becomes one uniform batch per layout, messages in their given order.  (More than 32 layouts: the
        // generic kernel takes the whole batch, as it did for every mixed batch before.)
        auto key = [](const ohgpu_src_msg_desc& d) -> uint64_t {
            return (uint64_t)d.channels | ((uint64_t)d.src_bits << 8) | ((uint64_t)d.dst_bits << 16) | ((uint64_t)d.src_endian << 24) |
                   ((uint64_t)d.dst_endian << 32) | ((uint64_t)((d.flags & OHGPU_FLAG_SRC_PLANAR32) ? 1 : 0) << 40);
        };
        std::vector<uint64_t> keys;
        std::vector<std::vector<ohgpu_src_msg_desc>> groups;
        for (size_t i = 0; i < n && keys.size() <= 32; i++) {
            const uint64_t k = key(descs[i]);
            size_t g = 0;
            while (g < keys.size() && keys[g] != k) g++;
            if (g == keys.size()) { keys.push_back(k); groups.emplace_back(); }
            groups[g].push_back(descs[i]);
        }
        if (keys.size() <= 32) {
            for (size_t g = 0; g < groups.size() && err == OHGPU_OK; g++) {
                ohgpu_batch* part = nullptr;
                err = ohgpu_src_batch_create(ctx, src, groups[g].data(), groups[g].size(), src_arena_bytes, dst_arena_bytes, &part);
                if (err == OHGPU_OK) b->parts.push_back(part);
            }
        }
    }
    if (err == OHGPU_OK && !b->host_descs && !b->fast.enabled && b->parts.empty() && n > 0) {
        // no block kernel takes this batch (a layout none is instantiated for, more than 32 layouts, nothing block-aligned): the generic
        // kernel will run it whole, from its own form of the messages -- made now, in a second pass over descriptors known to be good
        if (!convert_all()) err = set_error(OHGPU_ERR_NOMEM, "ohgpu_src_batch_create: out of host memory");
        else {
            DevSrcDesc* const dev = b->host_descs.get();
            const uint64_t L = src->L, M = src->M;
            parallel_ranges(n, plan_threads(n, 16384), [&](unsigned, size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) dev[i] = src_convert_desc(descs[i], L, M); });
        }
    }
    return batch_done(err, b, out);
}

int ohgpu_src_batch_plan(const ohgpu_batch* b, uint64_t* block_kernel_out_frames, uint64_t* generic_pieces)
{
    if (!b || b->kind != kBatchSrc) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_plan: not a src batch");
    if (!b->parts.empty()) {
        uint64_t fast = 0, pieces = 0;
        for (const ohgpu_batch* part : b->parts) {
            uint64_t f = 0, p = 0;
            ohgpu_src_batch_plan(part, &f, &p);
            fast += f; pieces += p;
        }
        if (block_kernel_out_frames) *block_kernel_out_frames = fast;
        if (generic_pieces) *generic_pieces = pieces;
        return OHGPU_OK;
    }
    if (block_kernel_out_frames) *block_kernel_out_frames = b->fast.enabled ? b->fast.fast_out_frames : 0;
    if (generic_pieces) *generic_pieces = b->fast.enabled ? b->fast.n_rem : b->n;
    return OHGPU_OK;
}

int ohgpu_src_plan_digest(uint32_t L, uint32_t M, uint32_t taps_per_phase, const ohgpu_src_msg_desc* descs, size_t n,
                          uint64_t src_arena_bytes, uint64_t dst_arena_bytes, int kernel_variant,
                          const int32_t* coef_q28, int num_cus,
                          uint64_t* digest, uint64_t* units, uint64_t* generic_pieces, int* kernel)
{
    if (!descs || n == 0 || L == 0 || M == 0 || taps_per_phase == 0 || (uint64_t)L * taps_per_phase > (1u << 22))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_src_plan_digest: bad argument");
    // a filter and a context as far as the planner looks at them: no device behind either.  With the coefficients the filter is
    // described exactly as ohgpu_src_create describes it (src_describe: the half-band form, the tables, the gain); without them it
    // is "a polyphase filter of sane gain whose tables exist if its geometry allows".
    ohgpu_src flt{};
    SrcTables tables;
    if (coef_q28) {
        if (!src_describe(L, M, taps_per_phase, coef_q28, &flt, &tables, "ohgpu_src_plan_digest")) return OHGPU_ERR_INVALID;
    } else {
        flt.L = L; flt.M = M; flt.T = taps_per_phase;
        flt.max_sum_abs = (int64_t)1 << 28;
        flt.halfband = false;
        flt.mf_L_blk = taps_per_phase == 32 ? src_block_outputs(L, 6) : 0;
        tables.made = flt.mf_L_blk != 0;
    }
    flt.d_mf_amat = tables.made ? (uint8_t*)&flt : nullptr;         // (only its being there is looked at)
    ohgpu_ctx ctx{};
    ctx.variant = kernel_variant_alias(kernel_variant);
    ctx.num_cus = num_cus > 0 ? num_cus : 256;
    ohgpu_batch b;
    b.kind = kBatchSrc; b.n = n; b.src = &flt; b.src_arena_bytes = src_arena_bytes; b.dst_arena_bytes = dst_arena_bytes; b.uniform = true;
    PlanDigest pd{};
    const int err = src_check_and_plan(&ctx, &b, descs, n, nullptr, &pd);
    if (err != OHGPU_OK) return err;
    if (digest) *digest = pd.hash;
    if (units) *units = pd.units;
    if (generic_pieces) *generic_pieces = pd.pieces;
    if (kernel) *kernel = pd.kernel;
    return OHGPU_OK;
}

int ohgpu_src_batch_units(const ohgpu_batch* b, uint64_t* units, uint64_t* long_units)
{
    if (!b || b->kind != kBatchSrc) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_units: not a src batch");
    uint64_t u = 0, l = 0;
    if (!b->parts.empty()) {
        for (const ohgpu_batch* part : b->parts) {
            uint64_t pu = 0, pl = 0;
            ohgpu_src_batch_units(part, &pu, &pl);
            u += pu; l += pl;
        }
    } else if (b->fast.enabled) {
        u = b->fast.lean ? b->fast.n_lean : b->fast.n_work;
        l = b->fast.lean ? b->fast.n_long : 0;
    }
    if (units) *units = u;
    if (long_units) *long_units = l;
    return OHGPU_OK;
}

int ohgpu_src_batch_kernel_name(ohgpu_ctx* ctx, const ohgpu_batch* batch, char* out, size_t cap)
{
    CTX_GUARD("ohgpu_src_batch_kernel_name");
    if (!batch || batch->kind != kBatchSrc || !out || cap == 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_kernel_name: bad argument");
    std::string name;
    if (ctx->variant != 1 && !batch->parts.empty()) {
        for (const ohgpu_batch* part : batch->parts) {
            const char* k = src_kernel_of(ctx, part);
            if (name.find(k) == std::string::npos) name += (name.empty() ? "" : ",") + std::string(k);
        }
    } else {
        name = src_kernel_of(ctx, batch);
    }
    snprintf(out, cap, "%s", name.c_str());
    return OHGPU_OK;
}

int ohgpu_src_batch_occupancy(ohgpu_ctx* ctx, const ohgpu_batch* batch, int* workgroups_per_cu, int* designed_for, uint32_t* lds_bytes)
{
    CTX_GUARD("ohgpu_src_batch_occupancy");
    if (!batch || batch->kind != kBatchSrc || !workgroups_per_cu) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_occupancy: bad argument");
    const ohgpu_batch* one = batch->parts.empty() ? batch : batch->parts.front();
    if (src_kernel_choice(ctx, one) != kSrcWg) return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_batch_occupancy: the batch does not run on the workgroup kernel (%s)", src_kernel_of(ctx, one));
    WgOccupancy q;
    OHGPU_HIP_TRY(launch_src_mfma_wg(ctx, one, nullptr, nullptr, nullptr, &q));
    *workgroups_per_cu = q.groups_per_cu;
    if (designed_for) *designed_for = q.designed_for;
    if (lds_bytes) *lds_bytes = q.lds_bytes;
    return OHGPU_OK;
}

// (ev_start / ev_stop: both or neither.  A batch that is ONE launch of the workgroup matrix kernel carries them on its dispatch; any other
// -- several layouts, block-unaligned pieces on the generic kernel behind the block kernel, another kernel -- gets them recorded in
// front of its first launch and behind its last)
static int src_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    const int go = run_guard(ctx, "ohgpu_src_batch_run", batch, kBatchSrc, batch && batch->n == 0, false, src_base, dst_base);
    if (go < 0) return go;
    hipStream_t s = pick_stream(ctx, stream);
    if (go == 0) {                                                  // (an empty batch still records the caller's two events)
        if (ev_start) { OHGPU_HIP_TRY(hipEventRecord(ev_start, s)); OHGPU_HIP_TRY(hipEventRecord(ev_stop, s)); }
        return OHGPU_OK;
    }
    if (ctx->variant != 1 && !batch->parts.empty()) {               // one uniform batch per layout
        // "nothing is launched" on refusal holds for the whole batch: every part is asked first whether it is free (a part still
        // running on another stream refuses), and only then does the first one launch
        for (const ohgpu_batch* part : batch->parts)
            if (batch_busy_on_another_stream(part, s))
                return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_run: a part of the batch is still running on another stream (its unit counters "
                                 "serve one launch at a time: wait for it, use the same stream, or create a second batch); nothing was launched");
        if (ev_start) OHGPU_HIP_TRY(hipEventRecord(ev_start, s));
        for (const ohgpu_batch* part : batch->parts) {
            const int err = ohgpu_src_batch_run(ctx, part, src_base, dst_base, s);
            if (err != OHGPU_OK) return err;                        // (a device error: the destination may be partly written, as for any failed launch)
        }
        if (ev_stop) OHGPU_HIP_TRY(hipEventRecord(ev_stop, s));
        return OHGPU_OK;
    }
    const SrcKernel which = src_kernel_choice(ctx, batch, ((uintptr_t)src_base & 15u) == 0);
    // (a batch that is ONE launch of the workgroup matrix kernel: its dispatch carries an event -- the caller's two, or the batch's
    // "last launch done" -- instead of a marker packet behind it: back-to-back launches were 10 us apart with the marker)
    const bool one_launch = which == kSrcWg && batch->fast.n_rem == 0;
    const bool on_dispatch = ev_start && one_launch;
    if (ev_start && !on_dispatch) OHGPU_HIP_TRY(hipEventRecord(ev_start, s));
    if (which != kSrcGeneric) {
        const int claim = claim_single_launch(batch, s, "ohgpu_src_batch_run");        // (the block kernels' unit counters are the batch's)
        if (claim != OHGPU_OK) return claim;
        if (batch->fast.planes_ready) OHGPU_HIP_TRY(hipStreamWaitEvent(s, batch->fast.planes_ready, 0));     // (the ramp planes are filled on the context's stream)
        // whole phase-aligned blocks on the chosen block kernel, block-unaligned heads/tails on the generic one
        switch (which) {
        case kSrcWg: {
            WgOccupancy x;
            x.query = false; x.start = on_dispatch ? ev_start : nullptr; x.stop = on_dispatch ? ev_stop : batch->last_done;
            OHGPU_HIP_TRY(launch_src_mfma_wg(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, s, one_launch ? &x : nullptr));
            break;
        }
        case kSrcBlock: OHGPU_HIP_TRY(launch_src_block(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, s)); break;
        default: OHGPU_HIP_TRY(launch_src_lean(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, s)); break;
        }
        OHGPU_HIP_TRY(launch_src_v1(ctx, batch->fast.d_rem, batch->fast.n_rem, batch->src, (const uint8_t*)src_base, (uint8_t*)dst_base, s));
        if (!one_launch) launched(batch, s);
        else batch->last_untracked = on_dispatch;            // (else: last_done rode on the dispatch)
    } else {
        if (!batch->host_descs)
            return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_batch_run: this batch was planned for the block kernels and keeps no per-message descriptors for the "
                             "generic kernel, which %s asks for: create it while ohgpu_set_kernel_variant(1) is in force%s",
                             ctx->variant == 1 ? "kernel variant 1" : (batch->fast.wg_only ? "this kernel variant (the plan is the workgroup matrix kernel's alone)" : "a source arena that is not 16-byte aligned"),
                             ctx->variant == 1 ? "" : ", or run it under the variant / with the alignment it was planned for");
        {   // (the whole batch on the generic kernel: its per-message descriptors go to the device the first time this happens)
            std::lock_guard<std::mutex> hold(batch->lazy);
            if (!batch->d_descs && batch->n) {
                const int err = upload_batch(ctx, const_cast<ohgpu_batch*>(batch), batch->host_descs.get(), batch->n * sizeof(DevSrcDesc));
                if (err != OHGPU_OK) return err;
            }
        }
        OHGPU_HIP_TRY(launch_src_v1(ctx, batch->d_descs, batch->n, batch->src, (const uint8_t*)src_base, (uint8_t*)dst_base, s));
    }
    if (ev_stop && !on_dispatch) OHGPU_HIP_TRY(hipEventRecord(ev_stop, s));
    return OHGPU_OK;
}

int ohgpu_src_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    return src_batch_run(ctx, batch, src_base, dst_base, stream, nullptr, nullptr);
}

int ohgpu_src_batch_run_timed(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream, void* start_event, void* stop_event)
{
    if (!start_event || !stop_event) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_run_timed: null event");
    return src_batch_run(ctx, batch, src_base, dst_base, stream, (hipEvent_t)start_event, (hipEvent_t)stop_event);
}

int ohgpu_src_batch_block(const ohgpu_batch* b, uint32_t* block_outputs, uint32_t* block_inputs)
{
    if (!b || b->kind != kBatchSrc) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_block: not a src batch");
    const ohgpu_batch* p = b->parts.empty() ? b : b->parts[0];
    if (!p->fast.enabled) return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_batch_block: the batch has no block-kernel plan");
    for (const ohgpu_batch* q : b->parts)
        if (!q->fast.enabled || q->fast.params.L_blk != p->fast.params.L_blk) return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_batch_block: the batch's layouts are cut into blocks of different lengths");
    if (block_outputs) *block_outputs = p->fast.params.L_blk;
    if (block_inputs) *block_inputs = p->fast.params.M_blk;
    return OHGPU_OK;
}

int ohgpu_src_batch_advance(ohgpu_ctx* ctx, ohgpu_batch* b, uint64_t blocks)
{
    CTX_GUARD("ohgpu_src_batch_advance");
    if (!b || b->kind != kBatchSrc) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_advance: not a src batch");
    std::vector<ohgpu_batch*> all(b->parts.begin(), b->parts.end());
    if (all.empty()) all.push_back(b);
    for (const ohgpu_batch* p : all) {
        if (!p->fast.enabled)
            return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_batch_advance: the batch (or one of its layouts) has no block-kernel plan: its generic-kernel descriptors hold the positions themselves");
        if (p->fast.stream_start)
            return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_advance: a message of the batch starts its stream (its filter window reaches in front of input frame 0, "
                             "read as zeros): the same window a period later holds real history the batch's source windows do not declare");
    }
    // Nothing of the plan names an absolute position: a unit is where its rows lie in the two arenas, a ramp job where its frames lie in
    // their message, a generic-kernel piece its window relative to the buffer -- and a whole number of blocks later every message has
    // the phase it had.  The plan IS the next period's plan.
    for (ohgpu_batch* p : all) p->fast.advanced_blocks += blocks;
    if (all[0] != b) b->fast.advanced_blocks += blocks;
    return OHGPU_OK;
}

int ohgpu_src_batch_set_ramps(ohgpu_ctx* ctx, ohgpu_batch* b, const uint16_t* ramp_start, const uint16_t* ramp_end, size_t n)
{
    CTX_GUARD("ohgpu_src_batch_set_ramps");
    if (!b || b->kind != kBatchSrc || !ramp_start || !ramp_end) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_set_ramps: bad argument");
    if (n != b->n) return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_set_ramps: %zu endpoints for a batch of %zu messages", n, b->n);
    if (!b->parts.empty()) return set_error(OHGPU_ERR_UNSUPPORTED, "ohgpu_src_batch_set_ramps: a batch of several layouts (create one batch per layout to re-ramp it)");
    SrcFastPlan& f = b->fast;
    // Every form the batch keeps a ramped message in is checked before anything is written: a refused call leaves the endpoints in
    // force as they were.  (Only the messages that carry a ramp are looked at: the flags are the plan's.)
    auto beyond = [&](uint32_t m) { return ramp_start[m] > OHGPU_RAMP_MAX || ramp_end[m] > OHGPU_RAMP_MAX; };
    auto refuse = [&](uint32_t m) { return set_error(OHGPU_ERR_INVALID, "ohgpu_src_batch_set_ramps: message %u: ramp beyond Ramp::kMax (nothing was changed)", m); };
    for (uint32_t m : f.job_msg) if (beyond(m)) return refuse(m);
    for (uint32_t m : f.rem_msg) if (beyond(m)) return refuse(m);
    for (uint32_t m : f.msgs_ramped_msg) if (beyond(m)) return refuse(m);
    if (b->host_descs)
        for (size_t i = 0; i < n; i++) if ((b->host_descs[i].flags & OHGPU_FLAG_RAMP) && beyond((uint32_t)i)) return refuse((uint32_t)i);
    OHGPU_HIP_TRY(batch_wait_last_launch(b));                                    // (the batch's last launch reads what is rewritten here)
    hipStream_t s0 = ctx->stream;
    if (f.enabled) {
        for (size_t k = 0; k < f.host_jobs.size(); k++) { f.host_jobs[k].ramp_start = ramp_start[f.job_msg[k]]; f.host_jobs[k].ramp_end = ramp_end[f.job_msg[k]]; }
        for (size_t k = 0; k < f.host_rem.size(); k++) { f.host_rem[k].ramp_start = ramp_start[f.rem_msg[k]]; f.host_rem[k].ramp_end = ramp_end[f.rem_msg[k]]; }
        if (!f.msgs_ramped.empty()) {       // round 1's plan: its kernel reads the endpoints of whole-block messages from their SegMsg records
            for (size_t k = 0; k < f.msgs_ramped.size(); k++) {
                SegMsg& sm = f.host_msgs[f.msgs_ramped[k]];
                sm.ramp_start = ramp_start[f.msgs_ramped_msg[k]];
                sm.ramp_end = ramp_end[f.msgs_ramped_msg[k]];
            }
            OHGPU_HIP_TRY(hipMemcpyAsync(f.d_msgs, f.host_msgs.data(), f.host_msgs.size() * sizeof(SegMsg), hipMemcpyHostToDevice, s0));
        }
        if (!f.host_jobs.empty()) {
            OHGPU_HIP_TRY(hipMemcpyAsync(f.d_ramp_jobs, f.host_jobs.data(), f.host_jobs.size() * sizeof(RampJob), hipMemcpyHostToDevice, s0));
            OHGPU_HIP_TRY(hipMemsetAsync(f.d_planes, 0xff, (f.plane_entries ? f.plane_entries : 8) * sizeof(uint16_t), s0));
            OHGPU_HIP_TRY(launch_ramp_planes(ctx, f.d_ramp_jobs, (uint32_t)f.host_jobs.size(), f.d_planes, s0));
        }
        if (!f.host_rem.empty()) OHGPU_HIP_TRY(hipMemcpyAsync(f.d_rem, f.host_rem.data(), f.host_rem.size() * sizeof(DevSrcDesc), hipMemcpyHostToDevice, s0));
        if (f.planes_ready) OHGPU_HIP_TRY(hipEventRecord(f.planes_ready, s0));       // (a run on any stream waits for this: the new planes)
        OHGPU_HIP_TRY(hipStreamSynchronize(s0));                                    // (the host copies above are the caller's to change again)
    }
    if (b->host_descs) {                                                           // the generic kernel's form of every message (a batch created under variant 1)
        DevSrcDesc* const dev = b->host_descs.get();
        for (size_t i = 0; i < n; i++) { dev[i].ramp_start = ramp_start[i]; dev[i].ramp_end = ramp_end[i]; }
        std::lock_guard<std::mutex> hold(b->lazy);
        if (b->d_descs) OHGPU_HIP_TRY(hipMemcpy(b->d_descs, dev, n * sizeof(DevSrcDesc), hipMemcpyHostToDevice));
    }
    return OHGPU_OK;
}

int ohgpu_src_process_host(ohgpu_ctx* ctx, const ohgpu_src* src, const ohgpu_src_msg_desc* descs, size_t n,
                           const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes)
{
    CTX_GUARD("ohgpu_src_process_host");
    ohgpu_batch* b = nullptr;
    const int err = ohgpu_src_batch_create(ctx, src, descs, n, src_bytes, dst_bytes, &b);
    if (err != OHGPU_OK) return err;
    ctx->stage.src_calls++;
    return process_host(ctx, b, n, src_host, src_bytes, dst_host, dst_bytes, ohgpu_src_batch_run, [&](size_t i) { return frames_range(descs[i]); });
}

}  // extern "C"
