// api_common.h -- what the C ABI's files share (ohgpu_api.hip: the core; api_*.hip and ohm_frame_kernel.hip: a family each).  A batch's
// life has one shape: batch_begin, the family's checks and plan, batch_done; run_guard in front of every launch;
// ohgpu_batch_destroy's table (ohgpu_api.hip) at the end.  Nothing here is exported from the library.
#pragma once

#include <algorithm>
#include <cstring>
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
// Where decoded audio goes (`what`: "flac desc", "alac desc"): `samples` samples a channel from dst_offset on, in planes of 4-byte words
// dst_plane_stride apart that do not overlap, or (packed_frame_bytes != 0) interleaved with no stride; inside the destination arena.
inline int decoded_dst_check(const char* what, size_t i, uint32_t channels, uint64_t samples, uint64_t packed_frame_bytes, uint64_t dst_offset,
                             uint64_t dst_plane_stride, uint64_t dst_arena_bytes)
{
    if (dst_offset % 4 != 0 || dst_plane_stride % 4 != 0) return set_error(OHGPU_ERR_INVALID, "%s %zu: dst_offset and dst_plane_stride must be multiples of 4", what, i);
    uint64_t span;
    if (packed_frame_bytes) {
        if (dst_plane_stride != 0) return set_error(OHGPU_ERR_INVALID, "%s %zu: dst_plane_stride with packed output", what, i);
        span = samples * packed_frame_bytes;
    } else {
        const uint64_t plane = samples * 4u;
        if (channels > 1 && dst_plane_stride < plane) return set_error(OHGPU_ERR_INVALID, "%s %zu: planes overlap (stride %llu < %llu)", what, i, (unsigned long long)dst_plane_stride, (unsigned long long)plane);
        if (dst_plane_stride > (1ull << 40)) return set_error(OHGPU_ERR_INVALID, "%s %zu: dst_plane_stride out of range", what, i);
        span = (uint64_t)(channels - 1u) * dst_plane_stride + plane;
    }
    return arena_span(what, i, "writes", dst_offset, span, dst_arena_bytes, "destination");
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
// the arenas; `null_src_ok` -- a batch that touches no source byte runs without one; `needs_dst` -- false where the batch writes to no
// destination arena (MPEG-4 never does, a PCM file batch without room for a frame does not).  > 0: launch; 0: empty; < 0: refused, error set.
int run_guard(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, BatchKind kind, bool empty, bool null_src_ok,
              const void* src_base, const void* dst_base, bool needs_dst = true);
// Batches with per-launch device state (ohgpu_batch::last_done): a launch on another stream while the last one runs is refused.
int claim_single_launch(const ohgpu_batch* b, hipStream_t s, const char* who);
inline void launched(const ohgpu_batch* b, hipStream_t s) { b->last_untracked = false; if (b->last_done) (void)hipEventRecord(b->last_done, s); }
// ---- the batch states (RunState, ohgpu_internal.h: FlacState, AlacState -- RAOP's too --, OhmRxState, OggState, Mp4State, Mp4fState, and
// FileState of the two file layers, whose whole shell is api_file.h).
// In a plan: state_events creates the n events of the family's phases (the last is the end of a run); dev_array is a device block of
// `count` elements from the context's block cache, entered in the state's registry, and filled from `host` (synchronously) where one is
// given -- a zero count allocates nothing and leaves the pointer null; state_own enters a block that a run allocates.
inline int state_events(RunState& st, int n)
{
    if (n < 1 || n > RunState::kMaxEvents) return set_error(OHGPU_ERR_INVALID, "state_events: %d events where a state holds %d", n, RunState::kMaxEvents);
    st.n_events = n;
    for (int k = 0; k < n; k++) OHGPU_HIP_TRY_ALLOC(hipEventCreate(&st.ev[k]));
    return OHGPU_OK;
}
inline void state_own(RunState& st, void** p) { st.blocks.push_back(p); }
template <typename T>
inline int dev_array(ohgpu_ctx* ctx, RunState& st, void** p, size_t count, const T* host = nullptr)
{
    state_own(st, p);
    if (!count) return OHGPU_OK;
    OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, p, count * sizeof(T)));
    if (host) OHGPU_HIP_TRY_ALLOC(hipMemcpy(*p, host, count * sizeof(T), hipMemcpyHostToDevice));
    return OHGPU_OK;
}
// The whole of a family's release but `delete`: the device drained, every registered block that exists freed, every event that exists
// destroyed.  It takes a state at any point of its plan.
inline void state_release(ohgpu_ctx* ctx, RunState& st)
{
    (void)hipDeviceSynchronize();
    for (void** p : st.blocks) if (*p) { ctx_dev_free(ctx, *p); *p = nullptr; }
    for (hipEvent_t& e : st.ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
}
// A family's whole release (ohgpu_batch_destroy's table, csrc/ohgpu_api.hip, calls it on the batch's pointer): nothing for a null
// pointer -- a batch that never got its state, or one released before --, else state_release, delete, and the pointer nulled.
template <class S>
void state_free(ohgpu_ctx* ctx, S*& p)
{
    if (!p) return;
    state_release(ctx, *p);
    delete p;
    p = nullptr;
}
// ... of a family that holds key schedules (CencState, CbcsState).  They do not outlive the batch: the device block is cleared before it
// goes back to the cache, the host copy too.
template <class S>
void protected_free(ohgpu_ctx* ctx, S*& p)
{
    if (p) {
        (void)hipDeviceSynchronize();
        if (p->d_keys) (void)hipMemset(p->d_keys, 0, p->keys_bytes);
        for (uint32_t& w : p->keys) *(volatile uint32_t*)&w = 0;
    }
    state_free(ctx, p);
}
// The front of a results, table or phase call: the context, then "<who>: not <noun> batch" (the noun with its article: "an Ogg") unless
// the batch is of `kind`.
inline int state_guard(ohgpu_ctx* ctx, const char* who, const ohgpu_batch* batch, BatchKind kind, const char* noun)
{
    CTX_GUARD(who);
    if (!batch || batch->kind != kind) return set_error(OHGPU_ERR_INVALID, "%s: not %s batch", who, noun);
    return OHGPU_OK;
}
// The device records serve ONE RUN AT A TIME, and a run never refuses a stream: run_begin is the first line of the family's run, run_end
// its last.  A run on another stream than the last one's first waits, on the host, for the last run -- on the EVENT that run recorded
// at its end, never on its stream, which the caller may have destroyed since; a run that returned an error half way recorded no end,
// and the whole device is waited for instead.  A run on the same stream queues behind the last one by itself.
inline int run_begin(RunState& st, hipStream_t s)
{
    if (st.last_stream && st.last_stream != s) OHGPU_HIP_TRY(st.ended ? hipEventSynchronize(st.end_event()) : hipDeviceSynchronize());
    st.last_stream = s;
    st.ended = false;
    st.ran = true;
    return OHGPU_OK;
}
inline int run_end(RunState& st, hipStream_t s)
{
    OHGPU_HIP_TRY(hipEventRecord(st.end_event(), s));
    st.ended = true;
    return OHGPU_OK;
}
// What the last run left in a device block, home: "<who>: the batch has not run", the wait for the run's end, the copy.  The room for
// it and the batch with nothing to fetch are the caller's to judge first.
inline int fetch_after_run(const char* who, const RunState& st, void* dst, const void* d_src, size_t bytes)
{
    if (!st.ran) return set_error(OHGPU_ERR_INVALID, "%s: the batch has not run", who);
    OHGPU_HIP_TRY(hipEventSynchronize(st.end_event()));
    if (bytes) OHGPU_HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return OHGPU_OK;
}
// A table of the last run, home, behind state_guard: "<who>: room for <n> <wording> <have><tail>" unless n is what the batch has and
// there is somewhere to put it (the families word it differently: `wording` is "rows, the batch's tables have", "records, the batch's
// table has", ...); nothing to fetch from an empty table or for a batch of no streams; then fetch_after_run of n rows of row_bytes.
inline int fetch_table(const char* who, const RunState& st, const char* wording, const char* tail, size_t n, size_t have, size_t n_streams, void* out,
                       const void* d_src, size_t row_bytes)
{
    if (n != have || (n && !out)) return set_error(OHGPU_ERR_INVALID, "%s: room for %zu %s %zu%s", who, n, wording, have, tail);
    if (!n || !n_streams) return OHGPU_OK;
    return fetch_after_run(who, st, out, d_src, n * row_bytes);
}
// ... the stream results: "<who>: room for <n> results, the batch has <n_streams> streams"
inline int fetch_results(const char* who, const RunState& st, size_t n, size_t n_streams, void* out, const void* d_results, size_t row_bytes)
{
    return fetch_table(who, st, "results, the batch has", " streams", n, n_streams, n_streams, out, d_results, row_bytes);
}
// (first, count) ranges of a batch check that must not overlap ("<who>: the <noun> ranges [a, +b) and [c, +d) overlap"); sorts them
inline int ranges_disjoint(const char* who, const char* noun, std::vector<std::pair<uint64_t, uint64_t>>& ranges)
{
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); k++)
        if (ranges[k - 1].first + ranges[k - 1].second > ranges[k].first)
            return set_error(OHGPU_ERR_INVALID, "%s: the %s ranges [%llu, +%llu) and [%llu, +%llu) overlap", who, noun, (unsigned long long)ranges[k - 1].first,
                             (unsigned long long)ranges[k - 1].second, (unsigned long long)ranges[k].first, (unsigned long long)ranges[k].second);
    return OHGPU_OK;
}
// An ohgpu_*_batch_phase_ms behind its argument check: ms[k] = the time from events[k] to events[k + 1], k < count (waits for the last)
inline int phase_ms(const char* who, bool ran, const hipEvent_t* events, int count, float* ms)
{
    if (!ran) return set_error(OHGPU_ERR_INVALID, "%s: the batch has not run", who);
    OHGPU_HIP_TRY(hipEventSynchronize(events[count]));
    for (int k = 0; k < count; k++) OHGPU_HIP_TRY(hipEventElapsedTime(&ms[k], events[k], events[k + 1]));
    return OHGPU_OK;
}

// The route plan_fmt_line planned a fmt batch onto (api_fmt.hip): ohgpu_fmt_batch_run and ohgpu_batch_paths_info both ask it.
enum FmtRoute { kFmtRoutePcmLine, kFmtRouteWide, kFmtRouteStereo, kFmtRouteStaged, kFmtRouteGeneric };
FmtRoute fmt_route(const ohgpu_batch* b);

// ---- host buffers.  host_stage_in: the first half of host_roundtrip (ohgpu_internal.h) and of decoder_process_host -- counts the call,
// reserves the context's two device arenas, sends src_host on the context's stream.  process_host: the body of an ohgpu_*_process_host behind its create --
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
// decoder_process_host: the whole of a decoder's ohgpu_*_process_host (FLAC, Apple Lossless, RAOP), whose outputs are known only after
// the run -- the null-buffer check, create(&batch), the source sent, run(batch, d_src, d_dst) = the family's run and results, then
// download() = the copies of what was decoded, queued on the context's stream, and one wait.  The batch is destroyed either way.
template <typename Create, typename Run, typename Download>
int decoder_process_host(ohgpu_ctx* ctx, const char* who, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                         Create&& create, Run&& run, Download&& download)
{
    CTX_GUARD(who);
    if ((src_bytes && !src_host) || (dst_bytes && !dst_host)) return set_error(OHGPU_ERR_INVALID, "%s: null buffer", who);
    ohgpu_batch* b = nullptr;
    int err = create(&b);
    if (err != OHGPU_OK) return err;
    const BatchPtr own(b, BatchDeleter{ctx});
    err = host_stage_in(ctx, src_host, src_bytes, dst_bytes);
    if (err != OHGPU_OK) return err;
    err = run(b, ctx->stage.d_src, ctx->stage.d_dst);
    if (err != OHGPU_OK) { (void)hipStreamSynchronize(ctx->stream); return err; }
    err = download();
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && err == OHGPU_OK) err = set_error(OHGPU_ERR_DEVICE, "%s: hipStreamSynchronize failed", who);
    return err;
}
// One run of decoded samples home (queued, and counted in d2h_bytes): samples [first, first + samples) of `unit` bytes each, from each
// of `planes` planes plane_stride apart (packed output: one plane) of the context's destination arena to the same place in dst_host.
inline int download_planes(ohgpu_ctx* ctx, const char* who, void* dst_host, uint64_t dst_offset, uint64_t plane_stride, uint32_t planes, uint64_t unit,
                           uint64_t first, uint64_t samples)
{
    for (uint32_t c = 0; c < planes; c++) {
        const uint64_t off = dst_offset + c * plane_stride + first * unit, bytes = samples * unit;
        if (hipMemcpyAsync((uint8_t*)dst_host + off, (const uint8_t*)ctx->stage.d_dst + off, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            return set_error(OHGPU_ERR_DEVICE, "%s: download failed", who);
        ctx->stage.d2h_bytes += bytes;
    }
    return OHGPU_OK;
}

// ---- Apple Lossless (api_alac.hip), shared with RAOP (api_raop.hip), whose decoding streams are Apple Lossless streams behind a cipher:
// one descriptor's validation (its packets [next_packet, +n_packets) of the table), its device-side record, the summary of a stream's
// packet results, the download of what a stream decoded (of process_host; queued on the context's stream, not waited for), and the
// body of both families' process_host: create, run and results are the family's, download(i, packet results) brings stream i home.
int  alac_check_desc(const ohgpu_alac_stream_desc& d, size_t i, const ohgpu_alac_packet* packets, uint64_t next_packet, size_t n_packets,
                     uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
void alac_add_stream(AlacState& a, size_t i, const ohgpu_alac_stream_desc& d);
void alac_summarise(const ohgpu_alac_packet_result* pres, uint32_t n_packets, ohgpu_alac_stream_result* out);
int  alac_download_decoded(ohgpu_ctx* ctx, const char* who, const ohgpu_alac_stream_desc& d, const ohgpu_alac_packet_result* pres, void* dst_host);
// ... and the same for FLAC (api_flac.hip), shared with Ogg FLAC (api_ogg.hip): a chain's frames are consecutive, so one run of samples
int  flac_download_decoded(ohgpu_ctx* ctx, const char* who, const ohgpu_flac_stream_desc& d, const ohgpu_flac_stream_result& r, void* dst_host);
using AlacResults = int (*)(ohgpu_ctx*, const ohgpu_batch*, ohgpu_alac_stream_result*, size_t, ohgpu_alac_packet_result*, size_t);
template <typename Create, typename Download>
int alac_process_host(ohgpu_ctx* ctx, const char* who, size_t n, size_t n_packets, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                      ohgpu_alac_stream_result* stream_results, ohgpu_alac_packet_result* packet_results, Create&& create, BatchRun run, AlacResults results,
                      Download&& download)
{
    std::vector<ohgpu_alac_stream_result> sres;
    std::vector<ohgpu_alac_packet_result> pres;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes, create,
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            sres = std::vector<ohgpu_alac_stream_result>(n);
            pres = std::vector<ohgpu_alac_packet_result>(n_packets);
            if (!n_packets) return (int)OHGPU_OK;
            const int e = run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : results(ctx, b, n ? sres.data() : nullptr, n, pres.data(), n_packets);
        },
        [&] {   // only what was decoded comes back
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++) e = download(i, pres.data());
            return e;
        });
    if (err == OHGPU_OK && stream_results && n) memcpy(stream_results, sres.data(), n * sizeof(sres[0]));
    if (err == OHGPU_OK && packet_results && n_packets) memcpy(packet_results, pres.data(), n_packets * sizeof(pres[0]));
    return err;
}

}  // namespace ohgpu
#pragma GCC visibility pop
