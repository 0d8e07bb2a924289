// flac_frame_kernel.hip -- native FLAC frames on the device (the format text is csrc/flac_frame_core.h).
// One run is four phases:
//   scan     a thread tests four byte positions of a stream for a frame header (sync, legal codes, well-formed number, CRC-8) and
//            appends the hits to a list with an ordinary atomic add; the host sorts the list by (stream, position), so that nothing
//            depends on the order the hits arrived in
//   probe    a thread per candidate: the entropy decode to the frame's end with the CRC-16 on the way; the residuals go to the
//            candidate's rows of scratch (one row of max_blocksize words per channel) and a record per subframe beside them
//   chain    a thread per stream walks from frame end to frame start over the probe results and marks the accepted frames
//   restore  accepted frames only: a thread per row runs the predictor recurrence in place (64-bit sums), then a thread per sample
//            decorrelates the channels and stores, consecutive lanes to consecutive samples
// The plain route (ohgpu_set_kernel_variant(1)) probes without storing and then decodes each accepted frame with ONE thread, straight
// from the bytes.  Every load is bounded by the descriptor's source range (the bit reader never fetches past it), every row store by
// max_blocksize (a larger block fails in the header) and every destination store by the chain's place check.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "api_common.h"

namespace ohgpu {

using namespace flaccore;

constexpr uint32_t kScanThreads = 256, kScanPerThread = 4, kScanTile = kScanThreads * kScanPerThread;
constexpr uint32_t kProbeThreads = 64;

__global__ __launch_bounds__(kScanThreads) void flac_scan_kernel(const Stream* __restrict__ streams, const FlacScanTile* __restrict__ tiles,
                                                                 const uint8_t* __restrict__ src, const Tables* __restrict__ tables,
                                                                 uint2* __restrict__ list, uint32_t cap, uint32_t* __restrict__ counter)
{
    const FlacScanTile tile = tiles[blockIdx.x];
    const Stream s = streams[tile.stream];
    const StreamCfg cfg = cfg_of(s);
    for (uint32_t k = 0; k < kScanPerThread; k++) {
        const uint32_t pos = tile.pos0 + k * kScanThreads + threadIdx.x;
        if (pos >= s.src_bytes) break;
        if (scan_position(src + s.src_offset + pos, s.src_bytes - pos, tables, cfg) == kParseBad) continue;
        const uint32_t at = atomicAdd(counter, 1u);
        if (at < cap) list[at] = make_uint2(tile.stream, pos);
    }
}

template <bool kStore>
__global__ __launch_bounds__(kProbeThreads) void flac_probe_kernel(const Stream* __restrict__ streams, Probe* __restrict__ probes, uint32_t n,
                                                                   const uint8_t* __restrict__ src, const Tables* __restrict__ tables,
                                                                   Sub* __restrict__ subs, int32_t* __restrict__ rows, uint32_t row_words)
{
    const uint32_t i = blockIdx.x * kProbeThreads + threadIdx.x;
    if (i >= n) return;
    Probe c = probes[i];
    const Stream s = streams[c.stream];
    const StreamCfg cfg = cfg_of(s);
    const uint8_t* p = src + s.src_offset + c.pos;
    const uint32_t left = s.src_bytes - c.pos;
    Header h;
    h.number = 0; h.blocksize = 0; h.rate = 0; h.channels = 0; h.bits = 0; h.assignment = 0; h.variable = 0; h.bytes = 0;
    uint32_t len = 0;
    const int st = parse_frame<kStore>(p, left, tables, cfg, &h, kStore ? subs + c.row0 : nullptr,
                                       kStore ? rows + (uint64_t)c.row0 * row_words : nullptr, row_words, &len);
    c.state = (uint32_t)st;
    c.end = st == kParseOk ? c.pos + len : (st == kParseShort && scan_position(p, left, tables, cfg) == kParseOk ? 1u : 0u);
    c.number = h.number; c.blocksize = h.blocksize; c.rate = h.rate;
    c.channels = h.channels; c.bits = h.bits; c.assignment = h.assignment; c.variable = h.variable;
    c.accepted = 0; c.place = 0;
    probes[i] = c;
}

__global__ void flac_chain_kernel(const Stream* __restrict__ streams, uint32_t n, Probe* __restrict__ probes, Result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    chain_stream(s, probes + s.cand_first, s.cand_count, results + i);
}

__global__ __launch_bounds__(kProbeThreads) void flac_predict_kernel(const Probe* __restrict__ probes, const uint32_t* __restrict__ row_cand, uint32_t n_rows,
                                                                     const Sub* __restrict__ subs, int32_t* __restrict__ rows, uint32_t row_words)
{
    const uint32_t r = blockIdx.x * kProbeThreads + threadIdx.x;
    if (r >= n_rows) return;
    const Probe& c = probes[row_cand[r]];
    if (!c.accepted) return;
    restore_channel(subs[r], rows + (uint64_t)r * row_words, c.blocksize);
}

__global__ __launch_bounds__(256) void flac_store_kernel(const Stream* __restrict__ streams, const Probe* __restrict__ probes,
                                                         const int32_t* __restrict__ rows, uint32_t row_words, uint8_t* __restrict__ dst)
{
    const Probe& c = probes[blockIdx.x];
    if (!c.accepted) return;
    const uint32_t i = blockIdx.y * 256u + threadIdx.x;
    if (i >= c.blocksize) return;
    const Stream s = streams[c.stream];
    const int32_t* row = rows + (uint64_t)c.row0 * row_words + i;
    const uint64_t index = (uint64_t)c.place + i;
    if (c.assignment >= 8) {
        int32_t l, r;
        decorrelate(c.assignment, row[0], row[row_words], &l, &r);
        store_sample(s, dst, index, 0, l);
        store_sample(s, dst, index, 1, r);
    } else {
        for (uint32_t ch = 0; ch < s.channels; ch++) store_sample(s, dst, index, ch, row[(uint64_t)ch * row_words]);
    }
}

// The plain route: one thread per accepted frame does everything, straight from the bytes (its rows of scratch are its work space).
__global__ __launch_bounds__(kProbeThreads) void flac_plain_kernel(const Stream* __restrict__ streams, const Probe* __restrict__ probes, uint32_t n,
                                                                   const uint8_t* __restrict__ src, const Tables* __restrict__ tables,
                                                                   Sub* __restrict__ subs, int32_t* __restrict__ rows, uint32_t row_words, uint8_t* __restrict__ dst)
{
    const uint32_t i = blockIdx.x * kProbeThreads + threadIdx.x;
    if (i >= n) return;
    const Probe& c = probes[i];
    if (!c.accepted) return;
    const Stream s = streams[c.stream];
    Header h;
    uint32_t len = 0;
    int32_t* mine = rows + (uint64_t)c.row0 * row_words;
    if (parse_frame<true>(src + s.src_offset + c.pos, s.src_bytes - c.pos, tables, cfg_of(s), &h, subs + c.row0, mine, row_words, &len) != kParseOk) return;
    for (uint32_t ch = 0; ch < s.channels; ch++) restore_channel(subs[c.row0 + ch], mine + (uint64_t)ch * row_words, h.blocksize);
    for (uint32_t k = 0; k < h.blocksize; k++) {
        const uint64_t index = (uint64_t)c.place + k;
        if (h.assignment >= 8) {
            int32_t l, r;
            decorrelate(h.assignment, mine[k], mine[row_words + k], &l, &r);
            store_sample(s, dst, index, 0, l);
            store_sample(s, dst, index, 1, r);
        } else {
            for (uint32_t ch = 0; ch < s.channels; ch++) store_sample(s, dst, index, ch, mine[(uint64_t)ch * row_words + k]);
        }
    }
}

int flac_plan(ohgpu_ctx* ctx, ohgpu_batch* b)
{
    FlacState& f = *b->flac;
    const size_t n = f.streams.size();
    std::vector<FlacScanTile> tiles;
    for (size_t i = 0; i < n; i++) {
        for (uint32_t pos = 0; pos < f.streams[i].src_bytes; pos += kScanTile) tiles.push_back(FlacScanTile{(uint32_t)i, pos});
        f.max_blocksize = std::max(f.max_blocksize, f.streams[i].max_blocksize);
    }
    f.n_tiles = (uint32_t)tiles.size();
    Tables t;
    make_tables(&t);
    OHGPU_TRY(state_events(f, 5));
    OHGPU_TRY(dev_array(ctx, f, &f.d_tables, 1, &t));
    OHGPU_TRY(dev_array<uint32_t>(ctx, f, &f.d_counter, 64));      // (the first word is the counter)
    OHGPU_TRY(dev_array<Stream>(ctx, f, &f.d_streams, n));
    OHGPU_TRY(dev_array<Result>(ctx, f, &f.d_results, n));
    OHGPU_TRY(dev_array(ctx, f, &f.d_tiles, tiles.size(), tiles.data()));
    for (void** p : {&f.d_list, &f.d_probes, &f.d_rowcand, &f.d_subs, &f.d_rows}) state_own(f, p);      // a run's, grown on demand
    return OHGPU_OK;
}

// p holds at least `bytes`: kept when it does, replaced (half as large again) when it does not
static int flac_reserve(ohgpu_ctx* ctx, void** p, size_t* cap, size_t bytes)
{
    if (*p && *cap >= bytes) return OHGPU_OK;
    ctx_dev_free(ctx, *p);
    *p = nullptr; *cap = 0;
    const size_t want = bytes + bytes / 2 + 256;
    OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, p, want));
    *cap = want;
    return OHGPU_OK;
}

int flac_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s, bool plain)
{
    FlacState& f = *b->flac;
    const size_t n = f.streams.size();
    OHGPU_TRY(run_begin(f, s));
    f.n_candidates = 0;
    const Tables* tables = (const Tables*)f.d_tables;
    // ---- scan (again, with a longer list, should the hits not fit) ----
    uint32_t found = 0;
    if (f.list_cap == 0) {
        uint64_t bytes = 0;
        for (const Stream& st : f.streams) bytes += st.src_bytes;
        size_t cap = 0;
        int err = flac_reserve(ctx, &f.d_list, &cap, (size_t)(bytes / 512 + 256) * sizeof(uint2));
        if (err != OHGPU_OK) return err;
        f.list_cap = cap / sizeof(uint2);
    }
    for (int attempt = 0; attempt < 2; attempt++) {
        OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(f.d_counter, 0, sizeof(uint32_t), s));
        OHGPU_HIP_TRY_ALLOC(hipMemcpyAsync(f.d_streams, f.streams.data(), n * sizeof(Stream), hipMemcpyHostToDevice, s));
        OHGPU_HIP_TRY_ALLOC(hipEventRecord(f.ev[0], s));
        if (f.n_tiles)
            hipLaunchKernelGGL(flac_scan_kernel, dim3(f.n_tiles), dim3(kScanThreads), 0, s, (const Stream*)f.d_streams, (const FlacScanTile*)f.d_tiles, src,
                               tables, (uint2*)f.d_list, (uint32_t)f.list_cap, (uint32_t*)f.d_counter);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        OHGPU_HIP_TRY_ALLOC(hipEventRecord(f.ev[1], s));
        OHGPU_HIP_TRY_ALLOC(hipMemcpyAsync(&found, f.d_counter, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        OHGPU_HIP_TRY_ALLOC(hipStreamSynchronize(s));
        if (found <= f.list_cap) break;
        if (attempt == 1) return set_error(OHGPU_ERR_DEVICE, "ohgpu_flac_batch_run: the scan found %u candidates, then more", (uint32_t)f.list_cap);
        size_t cap = 0;
        ctx_dev_free(ctx, f.d_list);
        f.d_list = nullptr;
        int err = flac_reserve(ctx, &f.d_list, &cap, (size_t)found * sizeof(uint2));
        if (err != OHGPU_OK) { f.list_cap = 0; return err; }
        f.list_cap = cap / sizeof(uint2);
    }
    // ---- the host's part: sort, the streams' shares, a row of scratch per (candidate, channel) ----
    f.host_list.resize((size_t)found * 2);
    if (found) OHGPU_HIP_TRY_ALLOC(hipMemcpy(f.host_list.data(), f.d_list, (size_t)found * sizeof(uint2), hipMemcpyDeviceToHost));
    std::vector<uint64_t> keys(found);
    for (uint32_t i = 0; i < found; i++) keys[i] = ((uint64_t)f.host_list[2 * i] << 32) | f.host_list[2 * i + 1];
    std::sort(keys.begin(), keys.end());
    f.host_probes.assign(found, Probe{});
    f.host_rowcand.clear();
    for (Stream& st : f.streams) { st.cand_first = 0; st.cand_count = 0; }
    for (uint32_t i = 0; i < found; i++) {
        Probe& c = f.host_probes[i];
        c.stream = (uint32_t)(keys[i] >> 32);
        c.pos = (uint32_t)keys[i];
        Stream& st = f.streams[c.stream];
        if (st.cand_count++ == 0) st.cand_first = i;
        c.row0 = (uint32_t)f.host_rowcand.size();
        for (uint32_t ch = 0; ch < st.channels; ch++) f.host_rowcand.push_back(i);
    }
    f.n_candidates = found;
    const size_t n_rows = f.host_rowcand.size();
    const uint32_t row_words = f.max_blocksize;
    OHGPU_HIP_TRY_ALLOC(hipMemcpyAsync(f.d_streams, f.streams.data(), n * sizeof(Stream), hipMemcpyHostToDevice, s));
    if (found) {
        int err = flac_reserve(ctx, &f.d_probes, &f.probes_cap, found * sizeof(Probe));
        if (err != OHGPU_OK) return err;
        if (f.rows_cap < n_rows) {
            ctx_dev_free(ctx, f.d_rowcand); ctx_dev_free(ctx, f.d_subs);
            f.d_rowcand = f.d_subs = nullptr; f.rows_cap = 0;
            const size_t want = n_rows + n_rows / 2 + 16;
            OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, &f.d_rowcand, want * sizeof(uint32_t)));
            OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, &f.d_subs, want * sizeof(Sub)));
            f.rows_cap = want;
        }
        const size_t words = n_rows * (size_t)row_words;
        if (f.rows_words < words) {
            ctx_dev_free(ctx, f.d_rows);
            f.d_rows = nullptr; f.rows_words = 0;
            const size_t want = words + words / 2;
            OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, &f.d_rows, want * 4));
            f.rows_words = want;
        }
        OHGPU_HIP_TRY_ALLOC(hipMemcpyAsync(f.d_probes, f.host_probes.data(), found * sizeof(Probe), hipMemcpyHostToDevice, s));
        OHGPU_HIP_TRY_ALLOC(hipMemcpyAsync(f.d_rowcand, f.host_rowcand.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        OHGPU_HIP_TRY_ALLOC(hipStreamSynchronize(s));             // (the host vectors are pageable and change with the next run)
    }
    Probe* probes = (Probe*)f.d_probes;
    Sub* subs = (Sub*)f.d_subs;
    int32_t* rows = (int32_t*)f.d_rows;
    const Stream* streams = (const Stream*)f.d_streams;
    const uint32_t cand_blocks = (found + kProbeThreads - 1) / kProbeThreads;
    // ---- probe ----
    if (found) {
        if (plain) hipLaunchKernelGGL(flac_probe_kernel<false>, dim3(cand_blocks), dim3(kProbeThreads), 0, s, streams, probes, found, src, tables, subs, rows, row_words);
        else hipLaunchKernelGGL(flac_probe_kernel<true>, dim3(cand_blocks), dim3(kProbeThreads), 0, s, streams, probes, found, src, tables, subs, rows, row_words);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(f.ev[2], s));
    // ---- chain ----
    if (n) {
        hipLaunchKernelGGL(flac_chain_kernel, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, s, streams, (uint32_t)n, probes, (Result*)f.d_results);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(f.ev[3], s));
    // ---- restore ----
    if (found) {
        if (plain) {
            hipLaunchKernelGGL(flac_plain_kernel, dim3(cand_blocks), dim3(kProbeThreads), 0, s, streams, (const Probe*)probes, found, src, tables, subs, rows, row_words, dst);
        } else {
            hipLaunchKernelGGL(flac_predict_kernel, dim3((uint32_t)((n_rows + kProbeThreads - 1) / kProbeThreads)), dim3(kProbeThreads), 0, s,
                               (const Probe*)probes, (const uint32_t*)f.d_rowcand, (uint32_t)n_rows, (const Sub*)subs, rows, row_words);
            hipLaunchKernelGGL(flac_store_kernel, dim3(found, (row_words + 255) / 256), dim3(256), 0, s, streams, (const Probe*)probes, (const int32_t*)rows, row_words, dst);
        }
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(f, s);
}

int flac_results(ohgpu_ctx* ctx, const ohgpu_batch* b, ohgpu_flac_stream_result* out)
{
    FlacState& f = *b->flac;
    return fetch_after_run("ohgpu_flac_batch_results", f, out, f.d_results, f.streams.size() * sizeof(Result));
}

int flac_frames(ohgpu_ctx* ctx, const ohgpu_batch* b, ohgpu_flac_frame* out, size_t capacity, size_t* n_frames)
{
    FlacState& f = *b->flac;
    OHGPU_TRY(fetch_after_run("ohgpu_flac_batch_frames", f, f.host_probes.data(), f.d_probes, (size_t)f.n_candidates * sizeof(Probe)));
    size_t k = 0;
    for (uint32_t i = 0; i < f.n_candidates; i++) {               // (sorted by stream, then position: stream order)
        const Probe& c = f.host_probes[i];
        if (!c.accepted) continue;
        if (k < capacity && out) {
            out[k].stream = c.stream; out[k].blocksize = c.blocksize;
            out[k].first_sample = (uint64_t)c.place + f.streams[c.stream].first_sample;
            out[k].src_pos = c.pos; out[k].src_end = c.end;
        }
        k++;
    }
    if (n_frames) *n_frames = k;
    return OHGPU_OK;
}

}  // namespace ohgpu
