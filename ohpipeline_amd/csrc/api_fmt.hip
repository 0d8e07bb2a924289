// api_fmt.hip -- the C ABI's layout-changing processors (a11, a13, a14: ohgpu_fmt_*).
#include "api_common.h"

using namespace ohgpu;

// The route plan_fmt_line planned a fmt batch onto: what ohgpu_fmt_batch_run launches (unless kernel variant 1 sends the batch to
// the generic kernel) and what ohgpu_batch_paths_info reports -- one function, so that the two cannot drift apart.
FmtRoute ohgpu::fmt_route(const ohgpu_batch* b)
{
    if (b->line.enabled) return kFmtRoutePcmLine;                       // mono / stereo Songcast packs as PCM messages
    if (b->fmtline.n_wide) return kFmtRouteWide;                        // Songcast packs of wider streams
    if (b->fmtline.enabled) return b->fmtline.group_kind ? kFmtRouteStereo : kFmtRouteStaged;
    return kFmtRouteGeneric;
}

extern "C" {

int ohgpu_fmt_batch_create(ohgpu_ctx* ctx, const ohgpu_fmt_desc* descs, size_t n,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_fmt_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_fmt_batch_create", kBatchFmt, descs || !n, n, 0xffffffffull, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err != OHGPU_OK) return err;
    for (size_t i = 0; i < n; i++) {
        const ohgpu_fmt_desc& d = descs[i];
        const uint64_t ch = d.channels, nf = d.n_frames, sb = d.src_bits / 8;
        uint64_t src_lo = d.src_offset, src_hi = 0, dst_lo = d.dst_offset, dst_hi = 0;
        if (ch < 1 || ch > 10) err = set_error(OHGPU_ERR_INVALID, "fmt desc %zu: channels %u outside 1..10", i, d.channels);
        else if (d.kind == OHGPU_FMT_UNPACK_PLANAR || d.kind == OHGPU_FMT_SENDER_PACK) {
            if (!valid_bits(d.src_bits)) err = set_error(OHGPU_ERR_INVALID, "fmt desc %zu: source depth %u", i, d.src_bits);   // ASSERTS(), StarvationRamper.cpp:178-180
            else {
                if (!span_end(d.src_offset, nf, ch * sb, 0, &src_hi)) src_hi = UINT64_MAX;
                if (d.kind == OHGPU_FMT_UNPACK_PLANAR) {
                    if (ch > 1 && d.dst_plane_stride < nf * 4) err = set_error(OHGPU_ERR_INVALID, "fmt desc %zu: planes overlap (stride %llu < %llu)", i, (unsigned long long)d.dst_plane_stride, (unsigned long long)(nf * 4));
                    if (!span_end(d.dst_offset, ch - 1, d.dst_plane_stride, nf * 4, &dst_hi)) dst_hi = UINT64_MAX;
                } else {
                    if (!span_end(d.dst_offset, nf, (ch < 2 ? ch : 2) * (sb < 3 ? sb : 3), 0, &dst_hi)) dst_hi = UINT64_MAX;
                }
            }
        } else if (d.kind == OHGPU_FMT_FLAC_PACK) {
            if (!(d.dst_bits == 8 || d.dst_bits == 16 || d.dst_bits == 24))       // THROW(CodecStreamFeatureUnsupported), Flac.cpp:404-407
                err = set_error(OHGPU_ERR_UNSUPPORTED, "fmt desc %zu: FLAC bit depth %u (8/16/24 only)", i, d.dst_bits);
            else if (d.src_bits != 32) err = set_error(OHGPU_ERR_INVALID, "fmt desc %zu: FLAC planes are TInt32 (src_bits must be 32)", i);
            else if (d.src_offset % 4 != 0 || d.src_plane_stride % 4 != 0) err = set_error(OHGPU_ERR_INVALID, "fmt desc %zu: TInt32 planes must be 4-byte aligned", i);
            else {
                if (!span_end(d.src_offset, ch - 1, d.src_plane_stride, nf * 4, &src_hi)) src_hi = UINT64_MAX;
                if (!span_end(d.dst_offset, nf, ch * (d.dst_bits / 8), 0, &dst_hi)) dst_hi = UINT64_MAX;
            }
        } else {
            err = set_error(OHGPU_ERR_INVALID, "fmt desc %zu: unknown kind %u", i, d.kind);
        }
        if (err == OHGPU_OK && nf > 0 && (src_lo > src_arena_bytes || src_hi > src_arena_bytes || src_hi < src_lo))
            err = set_error(OHGPU_ERR_BOUNDS, "fmt desc %zu: reads up to %llu beyond the %llu-byte source arena", i, (unsigned long long)src_hi, (unsigned long long)src_arena_bytes);
        if (err == OHGPU_OK && nf > 0 && (dst_lo > dst_arena_bytes || dst_hi > dst_arena_bytes || dst_hi < dst_lo))
            err = set_error(OHGPU_ERR_BOUNDS, "fmt desc %zu: writes up to %llu beyond the %llu-byte destination arena", i, (unsigned long long)dst_hi, (unsigned long long)dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        b->in_frames += nf;
        b->out_frames += nf;
        b->src_bytes_touched += nf ? src_hi - src_lo : 0;
        b->dst_bytes_written += nf ? dst_hi - dst_lo : 0;
    }
    err = upload_batch(ctx, b.get(), descs, n * sizeof(ohgpu_fmt_desc));
    if (err == OHGPU_OK) err = plan_fmt_line(ctx, b.get(), descs, n);
    return batch_done(err, b, out);
}

int ohgpu_fmt_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_fmt_batch_run", batch, kBatchFmt, batch && batch->n == 0, false, src_base, dst_base);
    if (go <= 0) return go;
    const uint8_t* src = (const uint8_t*)src_base;
    uint8_t* dst = (uint8_t*)dst_base;
    switch (ctx->variant == 1 ? kFmtRouteGeneric : fmt_route(batch)) {
    case kFmtRoutePcmLine: OHGPU_HIP_TRY(launch_pcm_line(ctx, batch, src, dst, pick_stream(ctx, stream))); break;
    case kFmtRouteWide: OHGPU_HIP_TRY(launch_ohm_wide(ctx, batch->fmtline.d_wide, batch->fmtline.n_wide, src, dst, nullptr, pick_stream(ctx, stream))); break;
    case kFmtRouteStereo:                                               // (launch_fmt_line picks the instantiation by group_kind / group_bytes)
    case kFmtRouteStaged: OHGPU_HIP_TRY(launch_fmt_line(ctx, batch, src, dst, pick_stream(ctx, stream))); break;
    case kFmtRouteGeneric: OHGPU_HIP_TRY(launch_fmt_v1(ctx, batch, src, dst, pick_stream(ctx, stream))); break;
    }
    return OHGPU_OK;
}

}  // extern "C"
