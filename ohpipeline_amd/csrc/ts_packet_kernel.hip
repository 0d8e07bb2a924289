// ts_packet_kernel.hip -- the MPEG transport stream demultiplexer and the ADTS frame table on the device (the text of the
// rules is csrc/ts_packet_core.h).
//   parse    a lane per grid packet of the batch (the packet's stream by bisection in the streams' first rows): tspkt::classify.
//   sums     a workgroup per stream.  Three minima over the stream's packets (the corrupt packet, the PAT, the PMT -- the PMT's section
//            is checked by the lane that stands on a candidate), then the packets in tiles of 256, the state carried from tile to tile:
//            a scan of counts (the audio packets, those with the payload bit: the counter of the one in front), the scan of tspkt::Seg
//            (what each packet delivers), a scan of the delivered bytes and the records.  A start writes the tail of the record in front
//            of it and the head of its own.  It leaves run_end and src_at per packet, the PES table and the result.
//   gather   the hot one.  A lane per 16-byte piece of the destination, a wave per tile of 64 pieces; the tile list is made at create
//            from each stream's capacity, the launch is capped at kTsGroupsPerCu workgroups a CU and every wave goes round the list in
//            strides of the launch's waves.  A tile behind the run's end does nothing.  tspkt::gather_piece.
//   plain    ohgpu_set_kernel_variant(1): one launch, a lane per stream runs tspkt::demux.
//   ADTS     map: a workgroup per tile of 1024 byte positions, a lane a position, a wave's 64 verdicts written as two words of the
//            bitmap.  chain: a wave per stream; recognition takes 64 start positions a step, the chain's search reads 64 words of the
//            bitmap a step (2048 positions).  plain: a lane per stream runs adts::walk.
// Loads: fields through csrc/field_bytes.h, inside a stream's grid (or its src_bytes, ADTS); the gather's words each hold a delivered
// byte.  Stores: [dst_offset, + bytes_delivered), which dst_capacity >= packets * 184 bounds; the rows of the stream's own table range.
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

constexpr uint32_t kTsThreads = 256, kTsWaves = kTsThreads / 64;
constexpr uint32_t kTsGroupsPerCu = 8, kTsTilePieces = 64;
constexpr uint32_t kAdtsTile = 1024;

// ---------------------------------------------------------------- transport stream
__global__ __launch_bounds__(kTsThreads) void ts_parse_kernel(const tspkt::Stream* __restrict__ streams, uint32_t n, const uint64_t* __restrict__ first, uint64_t n_grid,
                                                              const uint8_t* __restrict__ src, tspkt::Pkt* __restrict__ pkt)
{
    const uint64_t g = (uint64_t)blockIdx.x * kTsThreads + threadIdx.x;
    if (g >= n_grid) return;
    uint32_t a = 0, b = n;                                            // the last stream with first[i] <= g
    while (b - a > 1u) {
        const uint32_t m = a + (b - a) / 2u;
        if (first[m] <= g) a = m; else b = m;
    }
    const tspkt::Stream& s = streams[a];
    pkt[g] = tspkt::classify(s, src + s.src_offset, (uint32_t)(g - first[a]));
}

// inclusive sums over the workgroup (Hillis and Steele); total = the last lane's.  `cell` is free again when it returns.
__device__ uint32_t block_sums(uint32_t* cell, uint32_t v, uint32_t* total)
{
    const uint32_t t = threadIdx.x;
    cell[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kTsThreads; d <<= 1) {
        const uint32_t x = t >= d ? cell[t - d] : 0u;
        __syncthreads();
        cell[t] += x;
        __syncthreads();
    }
    const uint32_t mine = cell[t];
    *total = cell[kTsThreads - 1u];
    __syncthreads();
    return mine;
}

__global__ __launch_bounds__(kTsThreads) void ts_sums_kernel(const tspkt::Stream* __restrict__ streams, const uint64_t* __restrict__ first, const uint8_t* __restrict__ src,
                                                             const tspkt::Pkt* __restrict__ pkt, uint32_t* __restrict__ run_end_all, uint32_t* __restrict__ src_at_all,
                                                             tspkt::Pes* __restrict__ table, tspkt::Result* __restrict__ results)
{
    using namespace tspkt;
    __shared__ uint32_t s_min[2], s_count[6], s_cell[kTsThreads], s_cc[kTsThreads];
    __shared__ unsigned long long s_pmt;
    __shared__ Seg s_seg[kTsThreads];
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    const Stream s = streams[i];
    const uint8_t* const base = src + s.src_offset;
    const uint32_t np = packets(s);
    const Pkt* const pk = pkt + first[i];
    uint32_t* const run_end = run_end_all + first[i];
    uint32_t* const src_at = src_at_all + first[i];
    if (tid == 0) { s_min[0] = s_min[1] = kNone; s_pmt = ~0ull; }
    if (tid < 6) s_count[tid] = 0;
    __syncthreads();
    for (uint32_t k = tid; k < np; k += kTsThreads) {
        const Pkt p = pk[k];
        if (kind_of(p) == kCorruptField) atomicMin(&s_min[0], k);
        if (pat_here(s, p)) atomicMin(&s_min[1], k);
    }
    __syncthreads();
    Tab t = {s_min[0], s_min[1], kNone, s.pmt_pid, s.audio_pid, 0u};
    if (t.pat != kNone && t.pat >= t.corrupt) t.pat = kNone;
    if (t.pat != kNone) t.pmt_pid = found_pid(pk[t.pat]);
    uint32_t kinds[3] = {0u, 0u, 0u};
    for (uint32_t k = tid; k < np && k < t.corrupt; k += kTsThreads) {
        const Pkt p = pk[k];
        const uint32_t kind = kind_of(p);
        kinds[0] += kind == kBadSync; kinds[1] += kind == kTei; kinds[2] += kind == kScrambled;
        if (!pmt_candidate(s, t, p, k)) continue;
        const Pkt c = with_section(p, base, (uint64_t)k * kPacket, 2u);
        if (section_ok(c)) atomicMin(&s_pmt, ((unsigned long long)k << 16) | found_pid(c));
    }
    for (int c = 0; c < 3; c++) if (kinds[c]) atomicAdd(&s_count[c], kinds[c]);
    __syncthreads();
    if (s_pmt != ~0ull) { t.pmt = (uint32_t)(s_pmt >> 16); t.audio_pid = (uint32_t)(s_pmt & 0xffffu); t.first = t.pmt + 1u; }

    Seg carry = seg_start(s);                                         // (every lane carries the same state from tile to tile)
    uint32_t n_audio = 0, n_rec = 0, deliv = 0, bad = 0, jumps = 0, dropped = 0;
    int last_cc = -1;
    for (uint32_t k0 = 0; k0 < np; k0 += kTsThreads) {
        const uint32_t k = k0 + tid;
        const Pkt p = k < np ? pk[k] : Pkt{0u, 0u};
        const bool aud = k < np && is_audio(t, p, k), pay = aud && paybit_of(p);
        Elem e = {0u, 0u, 0u, 0u, 0u, 0u, kNoPts};
        if (aud) e = audio_elem(base, k, p);
        // the audio packets and those with the payload bit, counted; the counter of the one in front
        uint32_t tile_counts = 0;
        const uint32_t counts = block_sums(s_cell, (aud ? 1u : 0u) | (pay ? 0x10000u : 0u), &tile_counts);
        const bool is_first = aud && n_audio + (counts & 0xffffu) == 1u;
        const uint32_t pay_at = (counts >> 16) - (pay ? 1u : 0u), pays = tile_counts >> 16;
        if (pay) s_cc[pay_at] = cc_of(p);
        __syncthreads();
        const int before_cc = pay_at ? (int)s_cc[pay_at - 1u] : last_cc;
        const bool jump = pay && before_cc >= 0 && cc_of(p) != (((uint32_t)before_cc + 1u) & 15u);
        if (pays) last_cc = (int)s_cc[pays - 1u];
        // the segments' state
        s_seg[tid] = aud ? seg_of(s, e, is_first, jump) : Seg{0u, 0u, 0u};
        __syncthreads();
        for (uint32_t d = 1; d < kTsThreads; d <<= 1) {
            Seg left = {0u, 0u, 0u};
            if (tid >= d) left = s_seg[tid - d];
            __syncthreads();
            if (tid >= d) s_seg[tid] = combine(left, s_seg[tid]);
            __syncthreads();
        }
        const Seg before = tid ? combine(carry, s_seg[tid - 1u]) : carry;
        const Seg tile_end = combine(carry, s_seg[kTsThreads - 1u]);
        const uint32_t d = aud ? delivers(before, e) : 0u;
        const bool makes = aud && makes_record(s, e, is_first);
        // the delivered bytes and the records, counted (256 x 184 bytes < 2^16)
        uint32_t tile_sums = 0;
        const uint32_t sums = block_sums(s_cell, d | (makes ? 0x10000u : 0u), &tile_sums);
        const uint32_t rec_at = n_rec + (sums >> 16) - (makes ? 1u : 0u), run_to = deliv + (sums & 0xffffu);
        if (k < np) {
            run_end[k] = run_to;
            src_at[k] = aud ? k * kPacket + off_of(p) + e.skip : 0u;
        }
        if (aud && e.start && (before.bits & kSegRec)) record_tail(s, table, rec_at - 1u, before, true);
        if (makes) record_head(s, table, rec_at, run_to - d, k, e);
        bad += aud && e.start && !e.good; jumps += jump; dropped += e.c - d;
        carry = tile_end;
        n_audio += tile_counts & 0xffffu; n_rec += tile_sums >> 16; deliv += tile_sums & 0xffffu;
    }
    if (bad) atomicAdd(&s_count[3], bad);
    if (jumps) atomicAdd(&s_count[4], jumps);
    if (dropped) atomicAdd(&s_count[5], dropped);
    __syncthreads();
    if (tid != 0) return;
    if (carry.bits & kSegRec) record_tail(s, table, n_rec - 1u, carry, false);
    Result r = {};
    r.status = (uint8_t)status_of(s, t);
    r.trailing_bytes = (uint8_t)(s.src_bytes % kPacket);
    r.pmt_pid = (uint16_t)t.pmt_pid; r.audio_pid = (uint16_t)t.audio_pid;
    r.packets = np; r.bad_sync = s_count[0]; r.tei_packets = s_count[1]; r.scrambled_packets = s_count[2];
    r.pat_packet = t.pat; r.pmt_packet = t.pmt; r.corrupt_packet = t.corrupt;
    r.audio_packets = n_audio; r.pes_packets = n_rec; r.bad_pes_starts = s_count[3];
    r.bytes_delivered = deliv; r.dropped_bytes = s_count[5]; r.cc_jumps = s_count[4];
    r.pes_open_bytes = open_bytes_at_end(s, carry, n_audio);
    results[i] = r;
}

__global__ __launch_bounds__(kTsThreads) void ts_gather_kernel(const tspkt::Stream* __restrict__ streams, const uint64_t* __restrict__ first, const TsTile* __restrict__ tiles,
                                                               uint32_t n_tiles, const tspkt::Result* __restrict__ results, const uint32_t* __restrict__ run_end,
                                                               const uint32_t* __restrict__ src_at, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
    const uint32_t stride = gridDim.x * kTsWaves;
    for (uint32_t k = blockIdx.x * kTsWaves + wave; k < n_tiles; k += stride) {
        const TsTile tile = tiles[k];
        const tspkt::Stream& s = streams[tile.stream];
        const uint32_t bytes = results[tile.stream].bytes_delivered, q = tile.piece0 + lane;
        uint8_t* const run = dst + s.dst_offset;
        if (q >= tspkt::piece_count(run, bytes)) continue;
        const uint64_t row = first[tile.stream];
        tspkt::gather_piece(src + s.src_offset, run, bytes, run_end + row, src_at + row, tspkt::packets(s), q);
    }
}

__global__ __launch_bounds__(64) void ts_plain_kernel(const tspkt::Stream* __restrict__ streams, uint32_t n, const uint64_t* __restrict__ first, const uint8_t* __restrict__ src,
                                                      uint8_t* __restrict__ dst, tspkt::Pkt* __restrict__ pkt, uint32_t* __restrict__ run_end, uint32_t* __restrict__ src_at,
                                                      tspkt::Pes* __restrict__ table, tspkt::Result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint64_t row = first[i];
    tspkt::demux(streams[i], src, dst, table, pkt + row, run_end + row, src_at + row, &results[i]);
}

// The gather launch: a wave a tile, at most kTsGroupsPerCu workgroups a CU (tests/test_gpu_ts_textbook.py restates it)
uint32_t ts_wave_blocks(uint64_t tiles, uint32_t cus)
{
    const uint64_t want = (tiles + kTsWaves - 1) / kTsWaves, cap = (uint64_t)cus * kTsGroupsPerCu;
    return (uint32_t)(want < cap ? want : cap);
}

int ts_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const tspkt::Stream* streams)
{
    TsState& g = *b->ts;
    OHGPU_TRY(state_events(g, 4));
    if (!g.n_streams) return OHGPU_OK;
    std::vector<uint64_t> first(g.n_streams + 1);
    std::vector<TsTile> tiles;
    uint64_t grid = 0;
    for (size_t i = 0; i < g.n_streams; i++) {
        const uint32_t np = tspkt::packets(streams[i]);
        first[i] = grid;
        grid += np;
        // the lines of the address space a run of np * 184 bytes can touch, whatever its address
        const uint64_t pieces = np ? (uint64_t)np * 184u / 16u + 2u : 0u;
        for (uint64_t q = 0; q < pieces; q += kTsTilePieces) tiles.push_back(TsTile{(uint32_t)i, (uint32_t)q});
    }
    first[g.n_streams] = grid;
    if (grid > 0xffffffffull || tiles.size() > 0xffffffffull)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_ts_batch_create: %llu packets are more than one batch takes", (unsigned long long)grid);
    g.n_grid = grid;
    g.n_tiles = (uint32_t)tiles.size();
    g.wave_blocks = ts_wave_blocks(g.n_tiles, ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256u);
    OHGPU_TRY(dev_array(ctx, g, &g.d_streams, g.n_streams, streams));
    OHGPU_TRY(dev_array<tspkt::Result>(ctx, g, &g.d_results, g.n_streams));
    OHGPU_TRY(dev_array(ctx, g, &g.d_first, g.n_streams + 1, first.data()));
    OHGPU_TRY(dev_array<tspkt::Pkt>(ctx, g, &g.d_pkt, g.n_grid));
    OHGPU_TRY(dev_array<uint32_t>(ctx, g, &g.d_run_end, g.n_grid));
    OHGPU_TRY(dev_array<uint32_t>(ctx, g, &g.d_src_at, g.n_grid));
    OHGPU_TRY(dev_array(ctx, g, &g.d_tiles, g.n_tiles, tiles.data()));
    OHGPU_TRY(dev_array<tspkt::Pes>(ctx, g, &g.d_pes, g.n_pes));
    return OHGPU_OK;                                                  // (the PES table is zeroed at the head of every run)
}

int ts_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    TsState& g = *b->ts;
    OHGPU_TRY(run_begin(g, s));      // (the lists serve one run at a time)
    const uint32_t ns = (uint32_t)g.n_streams;
    const tspkt::Stream* streams = (const tspkt::Stream*)g.d_streams;
    const uint64_t* first = (const uint64_t*)g.d_first;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    // a run writes the records its streams have and no others: a record of the run before, of a stream that now has fewer PES packets,
    // must not stand in the table as if it were this run's
    if (g.n_pes) OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_pes, 0, g.n_pes * sizeof(tspkt::Pes), s));
    if (g.plain) {
        OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
        OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[2], s));
        hipLaunchKernelGGL(ts_plain_kernel, dim3((ns + 63u) / 64u), dim3(64), 0, s, streams, ns, first, src, dst, (tspkt::Pkt*)g.d_pkt, (uint32_t*)g.d_run_end,
                           (uint32_t*)g.d_src_at, (tspkt::Pes*)g.d_pes, (tspkt::Result*)g.d_results);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        return run_end(g, s);
    }
    if (g.n_grid) {
        hipLaunchKernelGGL(ts_parse_kernel, dim3((uint32_t)((g.n_grid + kTsThreads - 1) / kTsThreads)), dim3(kTsThreads), 0, s, streams, ns, first, g.n_grid, src,
                           (tspkt::Pkt*)g.d_pkt);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
    hipLaunchKernelGGL(ts_sums_kernel, dim3(ns), dim3(kTsThreads), 0, s, streams, first, src, (const tspkt::Pkt*)g.d_pkt, (uint32_t*)g.d_run_end, (uint32_t*)g.d_src_at,
                       (tspkt::Pes*)g.d_pes, (tspkt::Result*)g.d_results);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[2], s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(ts_gather_kernel, dim3(g.wave_blocks), dim3(kTsThreads), 0, s, streams, first, (const TsTile*)g.d_tiles, g.n_tiles, (const tspkt::Result*)g.d_results,
                           (const uint32_t*)g.d_run_end, (const uint32_t*)g.d_src_at, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(g, s);
}

// ---------------------------------------------------------------- ADTS
__global__ __launch_bounds__(kTsThreads) void adts_map_kernel(const adts::Stream* __restrict__ streams, const AdtsTile* __restrict__ tiles, const uint64_t* __restrict__ bit_base,
                                                              const uint8_t* __restrict__ src, uint32_t* __restrict__ bits)
{
    const AdtsTile tile = tiles[blockIdx.x];
    const adts::Stream& s = streams[tile.stream];
    const uint32_t n = s.src_bytes;
    const uint8_t* const base = src + s.src_offset;
    for (uint32_t k = 0; k < kAdtsTile / kTsThreads; k++) {
        const uint32_t pos = tile.pos0 + k * kTsThreads + threadIdx.x;
        adts::Hdr h;
        const bool valid = pos < n && adts::header_at(base, n, pos, &h);
        const unsigned long long verdicts = __ballot(valid);
        if (threadIdx.x % 64u == 0u) {                                // (the wave's 64 positions begin at a multiple of 64: two whole words)
            const uint64_t w = (bit_base[tile.stream] + pos) >> 5;
            bits[w] = (uint32_t)verdicts;
            bits[w + 1u] = (uint32_t)(verdicts >> 32);
        }
    }
}

__global__ __launch_bounds__(kTsThreads) void adts_chain_kernel(const adts::Stream* __restrict__ streams, uint32_t n_streams, const uint64_t* __restrict__ bit_base,
                                                                const uint8_t* __restrict__ src, const uint32_t* __restrict__ bits, adts::Frame* __restrict__ table,
                                                                adts::Result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * kTsWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
    if (i >= n_streams) return;
    const adts::Stream s = streams[i];
    const uint8_t* const base = src + s.src_offset;
    const uint32_t n = s.src_bytes;
    adts::Result r = {};
    uint32_t start = 0;
    if (s.flags & adts::kRecognise) {
        bool found = false;
        uint32_t payload = 0;
        for (uint32_t p0 = 0; p0 <= adts::kLastStart && !found; p0 += 64u) {
            uint32_t mine = 0;
            const bool ok = p0 + lane <= adts::kLastStart && adts::five_from(base, n, p0 + lane, &mine);
            const unsigned long long hits = __ballot(ok);
            if (!hits) continue;
            const uint32_t l = (uint32_t)__ffsll((long long)hits) - 1u;
            start = p0 + l;
            payload = __shfl(mine, (int)l);
            found = true;
        }
        if (!found) {
            r.status = adts::kNotAdts;
            if (lane == 0) results[i] = r;
            return;
        }
        adts::Hdr h;
        adts::header_at(base, n, start, &h);
        adts::set_first(&r, start, h);
        r.mean_payload_bytes = payload / adts::kRecogniseFrames;
    }
    const uint32_t* const map = bits + (bit_base[i] >> 5);
    const uint32_t words = (n + kAdtsTile - 1u) / kAdtsTile * (kAdtsTile / 32u);   // what the map phase wrote for this stream
    // the first position >= p with a valid header, or n - 6: the wave looks at 64 words of the map a step (every lane returns the same)
    auto next = [&](uint32_t p) {
        const uint32_t last = n - 6u;
        while (p < last) {
            const uint32_t w = (p >> 5) + lane;
            uint32_t v = w < words ? map[w] : 0u;
            if (lane == 0) v &= ~0u << (p & 31u);
            const unsigned long long hits = __ballot(v != 0u);
            if (hits) {
                const uint32_t l = (uint32_t)__ffsll((long long)hits) - 1u;
                const uint32_t vv = __shfl(v, (int)l);
                return ((p >> 5) + l) * 32u + (uint32_t)__ffs((int)vv) - 1u;
            }
            p = ((p >> 5) + 64u) * 32u;
        }
        return last;
    };
    adts::chain_from(s, base, start, table, next, &r, lane == 0);
    if (lane == 0) results[i] = r;
}

__global__ __launch_bounds__(64) void adts_plain_kernel(const adts::Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, adts::Frame* __restrict__ table,
                                                        adts::Result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    adts::walk(streams[i], src, table, &results[i]);
}

int adts_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const adts::Stream* streams)
{
    AdtsState& g = *b->adts;
    OHGPU_TRY(state_events(g, 3));
    if (!g.n_streams) return OHGPU_OK;
    std::vector<AdtsTile> tiles;
    std::vector<uint64_t> bit_base(g.n_streams);
    uint64_t bits = 0;
    for (size_t i = 0; i < g.n_streams; i++) {
        bit_base[i] = bits;
        for (uint32_t pos = 0; pos < streams[i].src_bytes; pos += kAdtsTile) tiles.push_back(AdtsTile{(uint32_t)i, pos});
        bits += ((uint64_t)streams[i].src_bytes + kAdtsTile - 1u) / kAdtsTile * kAdtsTile;
    }
    if (tiles.size() > 0x7fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_adts_batch_create: %llu source bytes are more than one batch takes", (unsigned long long)bits);
    g.n_tiles = g.plain ? 0u : (uint32_t)tiles.size();
    g.bits_bytes = g.plain ? 0u : (size_t)(bits / 8u);
    OHGPU_TRY(dev_array(ctx, g, &g.d_streams, g.n_streams, streams));
    OHGPU_TRY(dev_array<adts::Result>(ctx, g, &g.d_results, g.n_streams));
    OHGPU_TRY(dev_array(ctx, g, &g.d_bit_base, g.n_streams, bit_base.data()));
    OHGPU_TRY(dev_array(ctx, g, &g.d_tiles, g.n_tiles, tiles.data()));
    OHGPU_TRY(dev_array<uint8_t>(ctx, g, &g.d_bits, g.bits_bytes));
    OHGPU_TRY(dev_array<adts::Frame>(ctx, g, &g.d_frames, g.n_frames));
    return OHGPU_OK;                                                  // (the frame table is zeroed at the head of every run)
}

int adts_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, hipStream_t s)
{
    AdtsState& g = *b->adts;
    OHGPU_TRY(run_begin(g, s));
    const uint32_t ns = (uint32_t)g.n_streams;
    const adts::Stream* streams = (const adts::Stream*)g.d_streams;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    if (g.n_frames) OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_frames, 0, g.n_frames * sizeof(adts::Frame), s));      // (as ts_run zeroes its PES table)
    if (g.plain) {
        OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
        hipLaunchKernelGGL(adts_plain_kernel, dim3((ns + 63u) / 64u), dim3(64), 0, s, streams, ns, src, (adts::Frame*)g.d_frames, (adts::Result*)g.d_results);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
        return run_end(g, s);
    }
    if (g.n_tiles) {
        hipLaunchKernelGGL(adts_map_kernel, dim3(g.n_tiles), dim3(kTsThreads), 0, s, streams, (const AdtsTile*)g.d_tiles, (const uint64_t*)g.d_bit_base, src, (uint32_t*)g.d_bits);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
    hipLaunchKernelGGL(adts_chain_kernel, dim3((ns + kTsWaves - 1u) / kTsWaves), dim3(kTsThreads), 0, s, streams, ns, (const uint64_t*)g.d_bit_base, src,
                       (const uint32_t*)g.d_bits, (adts::Frame*)g.d_frames, (adts::Result*)g.d_results);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    return run_end(g, s);
}

}  // namespace ohgpu
