// api_file.h -- the one shell of the two file layers (PCM files: api_iff.hip and iff_pcm_kernel.hip; DSD files:
// api_dsd_file.hip and dsd_file_kernel.hip) over FileState (ohgpu_internal.h).  The host side of the kernel files:
// file_plan and file_run, which take what differs -- the layouts' sizes, how many conversion workgroups a stream's room needs, the
// three launches -- as plain arguments.  The C ABI's bodies: file_batch_check ... file_process_host, which take the family's nouns, its
// check of one descriptor, its plan and run and the bytes a result says were written.  Nothing here is exported from the library.
#pragma once

#include <cstring>

#include "api_common.h"

#pragma GCC visibility push(hidden)
namespace ohgpu {

// ---- the kernel files' host side.  groups_of(stream): the conversion workgroups its room in the destination arena needs, whatever the
// walk finds (0: it has no room, and a batch of such streams needs no destination arena).  `create` names the family's create call in
// "<create>: the destination ranges are more than one batch takes".
template <class Stream, class GroupsOf>
int file_plan(ohgpu_ctx* ctx, FileState& g, const char* create, const Stream* streams, size_t result_bytes, size_t rec_bytes, GroupsOf&& groups_of)
{
    OHGPU_TRY(state_events(g, 3));
    if (!g.n_streams) return OHGPU_OK;
    std::vector<PieceGroup> groups;
    for (size_t i = 0; i < g.n_streams; i++) {
        const uint64_t want = groups_of(streams[i]);
        g.writes = g.writes || want != 0u;
        if (g.plain) continue;
        if (groups.size() + want > 0x7fffffffull) return set_error(OHGPU_ERR_INVALID, "%s: the destination ranges are more than one batch takes", create);
        for (uint64_t k = 0; k < want; k++) groups.push_back(PieceGroup{(uint32_t)i, (uint32_t)k});
    }
    g.n_groups = (uint32_t)groups.size();
    OHGPU_TRY(dev_array(ctx, g, &g.d_streams, g.n_streams, streams));
    OHGPU_TRY(dev_array<uint8_t>(ctx, g, &g.d_results, g.n_streams * result_bytes));
    OHGPU_TRY(dev_array<uint8_t>(ctx, g, &g.d_recs, g.n_streams * rec_bytes));
    OHGPU_TRY(dev_array(ctx, g, &g.d_groups, g.n_groups, groups.data()));
    return OHGPU_OK;
}

// One run: ev[0], the plain kernel or the walk (a lane a stream, workgroups of 64), ev[1], the conversion (a workgroup of
// convert_threads per entry of the list) where there is one, the end.
template <class Stream, class Result, class Rec>
int file_run(FileState& g, const uint8_t* src, uint8_t* dst, hipStream_t s,
             void (*plain)(const Stream*, uint32_t, const uint8_t*, uint8_t*, Result*, Rec*), void (*walk)(const Stream*, uint32_t, const uint8_t*, Result*, Rec*),
             void (*convert)(const Stream*, const Rec*, const PieceGroup*, const uint8_t*, uint8_t*), uint32_t convert_threads)
{
    OHGPU_TRY(run_begin(g, s));      // (the records serve one run at a time)
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u;
    const Stream* const streams = (const Stream*)g.d_streams;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    if (g.plain) hipLaunchKernelGGL(plain, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, dst, (Result*)g.d_results, (Rec*)g.d_recs);
    else hipLaunchKernelGGL(walk, dim3(lane_blocks), dim3(64), 0, s, streams, ns, src, (Result*)g.d_results, (Rec*)g.d_recs);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
    if (!g.plain && g.n_groups) {
        hipLaunchKernelGGL(convert, dim3(g.n_groups), dim3(convert_threads), 0, s, streams, (const Rec*)g.d_recs, (const PieceGroup*)g.d_groups, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(g, s);
}

// ---- the C ABI's bodies.  `who` is the exported function's name; `what` the family's descriptor in a message ("iff desc"), `noun` its
// batch with the article ("a PCM file").
template <class Desc>
int file_batch_check(const char* who, const Desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes,
                     int (*check_desc)(const Desc&, size_t, uint64_t, uint64_t))
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    if (n > 0x00ffffffull) return set_error(OHGPU_ERR_INVALID, "%s: too many descriptors", who);
    std::vector<std::pair<uint64_t, uint64_t>> ranges;                 // (offset, bytes) of the streams that may write
    for (size_t i = 0; i < n; i++) {
        OHGPU_TRY(check_desc(descs[i], i, src_arena_bytes, dst_arena_bytes));
        if (descs[i].dst_bytes_capacity) ranges.emplace_back(descs[i].dst_offset, descs[i].dst_bytes_capacity);
    }
    return ranges_disjoint(who, "destination", ranges);
}

template <class Desc, class Stream>
int file_batch_create(ohgpu_ctx* ctx, const char* who, BatchKind kind, const Desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out,
                      int (*check)(const Desc*, size_t, uint64_t, uint64_t), int (*plan)(ohgpu_ctx*, ohgpu_batch*, const Stream*))
{
    CTX_GUARD(who);
    BatchPtr b;
    int err = batch_begin(ctx, who, kind, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = check(descs, n, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->file = new (std::nothrow) FileState();
    if (!b->file) return set_error(OHGPU_ERR_NOMEM, "%s: out of host memory", who);
    b->file->n_streams = n;
    b->file->plain = ctx->variant == 1;
    for (size_t i = 0; i < n; i++) b->src_bytes_touched += descs[i].src_bytes;
    err = plan(ctx, b.get(), (const Stream*)descs);
    return batch_done(err, b, out);
}

// (src_align: what the family asks of src_base -- DSD files 4, "<who>: src_base must be a multiple of 4"; PCM files 1)
inline int file_batch_run(ohgpu_ctx* ctx, const char* who, BatchKind kind, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream, uintptr_t src_align,
                          int (*run)(ohgpu_ctx*, const ohgpu_batch*, const uint8_t*, uint8_t*, hipStream_t))
{
    const bool mine = batch && batch->kind == kind;
    const int go = run_guard(ctx, who, batch, kind, mine && batch->file->n_streams == 0, true, src_base, dst_base, mine && batch->file->writes);
    if (go <= 0) return go;
    if ((uintptr_t)src_base % src_align) return set_error(OHGPU_ERR_INVALID, "%s: src_base must be a multiple of %u", who, (unsigned)src_align);
    return run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

template <class Result>
int file_batch_results(ohgpu_ctx* ctx, const char* who, BatchKind kind, const char* noun, const ohgpu_batch* batch, Result* results, size_t n)
{
    OHGPU_TRY(state_guard(ctx, who, batch, kind, noun));
    return fetch_results(who, *batch->file, n, batch->file->n_streams, results, batch->file->d_results, sizeof(Result));
}

inline int file_batch_phase_ms(ohgpu_ctx* ctx, const char* who, BatchKind kind, const char* noun, const ohgpu_batch* batch, float ms[2])
{
    OHGPU_TRY(state_guard(ctx, who, batch, kind, noun));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "%s: bad argument", who);
    const int err = phase_ms(who, batch->file->ran, batch->file->ev, 2, ms);
    if (err == OHGPU_OK && batch->file->plain) ms[1] = 0.0f;          // (one launch: what lies between the later events is no phase)
    return err;
}

// written(result): the bytes from the stream's dst_offset on that the result says the run wrote (0: nothing comes back)
template <class Desc, class Result, class Written>
int file_process_host(ohgpu_ctx* ctx, const char* who, const Desc* descs, size_t n, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes, Result* results,
                      int (*create)(ohgpu_ctx*, const Desc*, size_t, uint64_t, uint64_t, ohgpu_batch**), BatchRun run,
                      int (*fetch)(ohgpu_ctx*, const ohgpu_batch*, Result*, size_t), Written&& written)
{
    std::vector<Result> res(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return create(ctx, descs, n, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            const int e = run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : fetch(ctx, b, res.data(), n);
        },
        [&] {   // only what was written comes back
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (const uint64_t bytes = written(res[i])) e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, 1, 0, bytes);
            return e;
        });
    if (err == OHGPU_OK && results && n) memcpy(results, res.data(), n * sizeof(res[0]));
    return err;
}

}  // namespace ohgpu
#pragma GCC visibility pop
