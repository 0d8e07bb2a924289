// api_common.h -- what the C ABI's files share (ohgpu_api.hip: the core; api_*.hip and ohm_frame_kernel.hip: a family each).  A batch's
// life has one shape: batch_begin, the family's checks and plan, batch_done; run_guard in front of every launch;
// ohgpu_batch_destroy's table (ohgpu_api.hip) at the end.  Nothing here is exported from the library.
#pragma once

#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "ohgpu_internal.h"

#pragma GCC visibility push(hidden)
namespace ohgpu {

#define CTX_GUARD(name)                                                                    \
    if (!ctx) return set_error(OHGPU_ERR_INVALID, "%s: null context", name);              \
    OHGPU_HIP_TRY(hipSetDevice(ctx->device))

inline hipStream_t pick_stream(const ohgpu_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }
inline bool valid_bits(uint32_t bits) { return bits == 8 || bits == 16 || bits == 24 || bits == 32; }
inline bool valid_endian(uint32_t e) { return e == OHGPU_ENDIAN_LITTLE || e == OHGPU_ENDIAN_BIG; }
// The pipeline's DSD format (ohgpu.h's DSD section): ASSERT((W * 4) % (4 + P) == 0) with W - P chunks per block
inline bool valid_dsd_format(uint32_t W, uint32_t P) { return W >= 1 && W <= 255 && (P == 0 || (P % 2 == 0 && W == P + 4)); }
// end = off + a * b + c in 64 bits; false when any step wraps (such a descriptor is out of bounds: a wrapped end can look small)
inline bool span_end(uint64_t off, uint64_t a, uint64_t b, uint64_t c, uint64_t* end)
{
    uint64_t p = 0, q = 0;
    return !(__builtin_mul_overflow(a, b, &p) || __builtin_add_overflow(off, p, &q) || __builtin_add_overflow(q, c, end));
}
// [off, off + bytes) inside an arena?  Else OHGPU_ERR_BOUNDS, "<what> <i>: <verb> [off, +bytes) beyond the <arena>-byte <which> arena".
inline int arena_span(const char* what, size_t i, const char* verb, uint64_t off, uint64_t bytes, uint64_t arena, const char* which)
{
    if (off <= arena && bytes <= arena - off) return OHGPU_OK;
    return set_error(OHGPU_ERR_BOUNDS, "%s %zu: %s [%llu, +%llu) beyond the %llu-byte %s arena", what, i, verb, (unsigned long long)off,
                     (unsigned long long)bytes, (unsigned long long)arena, which);
}
// Variants 2 and 5 named kernels the library no longer has (round 1's block, round 4's unit-per-wave matrix kernel): aliases of 4.
inline int kernel_variant_alias(int variant) { return variant == 2 || variant == 5 ? 4 : variant; }

// ---- creation.  A batch under construction is owned by a BatchPtr, whose deleter is the whole ohgpu_batch_destroy: every failure after
// batch_begin is `return err;`, whatever the batch holds by then (the release functions take a partly built batch); the end is batch_done.
struct BatchDeleter { ohgpu_ctx* ctx; void operator()(ohgpu_batch* b) const { (void)ohgpu_batch_destroy(ctx, b); } };
using BatchPtr = std::unique_ptr<ohgpu_batch, BatchDeleter>;
// "<who>: null argument" unless `out` and `args_ok` (the family's own pointers: descriptors where n > 0, a filter), *out = nullptr,
// "<who>: too many descriptors" for n > n_cap (the family's), then the batch with its kind, n and arenas set and the rest zero.
int batch_begin(ohgpu_ctx* ctx, const char* who, BatchKind kind, bool args_ok, size_t n, uint64_t n_cap,
                uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out, BatchPtr* b);
inline int batch_done(int err, BatchPtr& b, ohgpu_batch** out) { if (err == OHGPU_OK) *out = b.release(); return err; }   // a create's last line
int upload_batch(ohgpu_ctx* ctx, ohgpu_batch* b, const void* host_descs, size_t bytes);      // b->d_descs, from the context's block cache

// ---- launches.  The front of every ohgpu_*_batch_run: the context, the kind ("<who>: not a <noun> batch"), and two rules that differ
// by family on purpose and are the caller's to state: `empty` (n == 0, no pieces, no tiles; FLAC has none) -- nothing to launch, whatever
// the arenas; `null_src_ok` -- a batch that touches no source byte runs without one.  > 0: launch; 0: empty; < 0: refused, error set.
int run_guard(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, BatchKind kind, bool empty, bool null_src_ok,
              const void* src_base, const void* dst_base);
// Batches with per-launch device state (ohgpu_batch::last_done): a launch on another stream while the last one runs is refused.
int claim_single_launch(const ohgpu_batch* b, hipStream_t s, const char* who);
inline void launched(const ohgpu_batch* b, hipStream_t s) { b->last_untracked = false; if (b->last_done) (void)hipEventRecord(b->last_done, s); }

// The route plan_fmt_line planned a fmt batch onto (api_fmt.hip): ohgpu_fmt_batch_run and ohgpu_batch_paths_info both ask it.
enum FmtRoute { kFmtRoutePcmLine, kFmtRouteWide, kFmtRouteStereo, kFmtRouteStaged, kFmtRouteGeneric };
FmtRoute fmt_route(const ohgpu_batch* b);

// ---- host buffers.  host_stage_in: the first half of host_roundtrip (ohgpu_internal.h) -- counts the call, reserves the context's two
// device arenas, sends src_host on the context's stream.  process_host: the body of an ohgpu_*_process_host behind its create --
// range(i) = (dst_offset, bytes) of output i, the round trip through the family's run, and the batch destroyed either way.
int host_stage_in(ohgpu_ctx* ctx, const void* src_host, uint64_t src_bytes, uint64_t dst_bytes);
using BatchRun = int (*)(ohgpu_ctx*, const ohgpu_batch*, const void*, void*, void*);
template <typename Range>
int process_host(ohgpu_ctx* ctx, ohgpu_batch* batch, size_t n, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                 BatchRun run, Range&& range)
{
    const BatchPtr b(batch, BatchDeleter{ctx});
    std::vector<std::pair<uint64_t, uint64_t>> out(n);
    for (size_t i = 0; i < n; i++) out[i] = range(i);
    return host_roundtrip(ctx, src_host, src_bytes, dst_host, dst_bytes, out,
                          [&](const void* d_src, void* d_dst) { return run(ctx, batch, d_src, d_dst, nullptr); });
}
// (dst_offset, bytes) of a message of n_frames interleaved frames: the pcm, src and src_pull descriptors alike
template <typename D>
std::pair<uint64_t, uint64_t> frames_range(const D& d) { return {d.dst_offset, (uint64_t)d.n_frames * d.channels * (d.dst_bits / 8)}; }

// ---- Apple Lossless (api_alac.hip), shared with RAOP (api_raop.hip), whose decoding streams are Apple Lossless streams behind a cipher:
// one descriptor's validation (its packets [next_packet, +n_packets) of the table), its device-side record, the summary of a stream's
// packet results, and the download of what a stream decoded (of process_host; queued on the context's stream, not waited for).
int  alac_check_desc(const ohgpu_alac_stream_desc& d, size_t i, const ohgpu_alac_packet* packets, uint64_t next_packet, size_t n_packets,
                     uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
void alac_add_stream(AlacState& a, size_t i, const ohgpu_alac_stream_desc& d);
void alac_summarise(const ohgpu_alac_packet_result* pres, uint32_t n_packets, ohgpu_alac_stream_result* out);
int  alac_download_decoded(ohgpu_ctx* ctx, const char* who, const ohgpu_alac_stream_desc& d, const ohgpu_alac_packet_result* pres, void* dst_host);

}  // namespace ohgpu
#pragma GCC visibility pop
