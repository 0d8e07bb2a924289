// ogg_page_kernel.hip -- the Ogg page layer on the device (the text of all four phases is csrc/ogg_page_core.h).
//   find     a lane per byte position, workgroups over tiles of kFindTile positions of one stream (the tile list is made at create).
//            A position where a whole page image starts is appended to the candidate list through one atomic counter.  The list
//            holds sum(src_bytes / 27 + 1) entries; what a stream of pages can never exceed.  Bytes made to exceed it ("OggS" every
//            few bytes) leave the counter above the capacity, which the walk sees.
//   verify   the wide one.  A wave per candidate, the launch capped at kGroupsPerCu workgroups a CU, every wave going round the list
//            in strides of the launch's waves; the list's length is read from the device-side counter.  The three tables (3 KiB) are
//            copied to LDS once a workgroup.  A lane runs its slice of the page through the byte table, shifts it to the page's end
//            with two multiplications, the wave xors the 64 terms (crc_lane), and lane 0 sets the position's bit when the sum is
//            the stored checksum.  Pages of one stream are verified side by side: nothing here knows which page follows which.
//   chain    a lane per stream: the walk (two instances: with the chained-stream rules for a batch that has a stream asking for them,
//            and without them in its text for every other batch, which so runs what it ran before those rules were written).  Latency-bound by construction; it is there so that the gather needs no host in front of
//            it.  At its end the lane takes its pieces' places in the dense work list with one atomic add.
//   gather   a wave per piece of the work list, persistent like verify, the count read from the device: ohmrx::gather_lane.
// Every load lies inside a stream's range, which ohgpu_ogg_batch_check placed inside the source arena (gather_lane may read back to
// the last multiple of 4 in front of a piece: a piece starts 27 bytes or more into its stream, and the arena's base is 4-byte
// aligned); every store lies inside [dst_offset, + bytes delivered), and dst_capacity >= src_bytes bounds that.
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

using namespace oggpage;

constexpr uint32_t kOggThreads = 256, kOggWaves = kOggThreads / 64;
constexpr uint32_t kFindTile = 1024;
constexpr uint32_t kGroupsPerCu = 8;

__global__ __launch_bounds__(kOggThreads) void ogg_find_kernel(const Stream* __restrict__ streams, const OggTile* __restrict__ tiles, const uint8_t* __restrict__ src,
                                                               Candidate* __restrict__ list, uint32_t cap, uint32_t* __restrict__ counters)
{
    const OggTile tile = tiles[blockIdx.x];
    const Stream& s = streams[tile.stream];
    const uint32_t n = s.src_bytes;
    const uint8_t* const base = src + s.src_offset;
    for (uint32_t k = 0; k < kFindTile / kOggThreads; k++) {
        const uint32_t pos = tile.pos0 + k * kOggThreads + threadIdx.x;
        if (pos >= n) continue;
        Page pg;
        if (parse_page(base + pos, n - pos, &pg) != 1) continue;
        const uint32_t slot = atomicAdd(&counters[0], 1u);
        if (slot < cap) list[slot] = Candidate{tile.stream, pos, pg.bytes, 0u};
    }
}

__global__ __launch_bounds__(kOggThreads) void ogg_verify_kernel(const Stream* __restrict__ streams, const uint64_t* __restrict__ bit_base, const Candidate* __restrict__ list,
                                                                 uint32_t cap, const uint32_t* __restrict__ counters, const Tables* __restrict__ tables,
                                                                 const uint8_t* __restrict__ src, uint32_t* __restrict__ bits)
{
    __shared__ uint32_t t_byte[256], t_shift[256], t_shift256[256];
    static_assert(kOggThreads == 256, "a table entry a thread");
    t_byte[threadIdx.x] = tables->byte[threadIdx.x];
    t_shift[threadIdx.x] = tables->shift[threadIdx.x];
    t_shift256[threadIdx.x] = tables->shift256[threadIdx.x];
    __syncthreads();
    const uint32_t found = counters[0], n = found < cap ? found : cap;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u), lane = threadIdx.x % 64u;
    const uint32_t stride = gridDim.x * kOggWaves;
    for (uint32_t k = blockIdx.x * kOggWaves + wave; k < n; k += stride) {
        const Candidate c = list[k];
        const uint8_t* const page = src + streams[c.stream].src_offset + c.pos;
        uint32_t term = crc_lane(t_byte, t_shift, t_shift256, page, c.bytes, lane);
        for (int o = 32; o; o >>= 1) term ^= __shfl_xor(term, o);
        if (lane == 0 && term == stored_crc(page)) {
            const uint64_t b = bit_base[c.stream] + c.pos;
            atomicOr(&bits[b >> 5], 1u << (b & 31u));
        }
    }
}

template <bool Links>
__global__ __launch_bounds__(64) void ogg_chain_kernel(const Stream* __restrict__ streams, uint32_t n, const uint64_t* __restrict__ bit_base, const uint64_t* __restrict__ piece_first,
                                                       const uint8_t* __restrict__ src, const uint32_t* __restrict__ bits, uint32_t cap, uint32_t* __restrict__ counters,
                                                       const Tables* __restrict__ tables, Packet* __restrict__ packets, Piece* __restrict__ pieces, uint32_t* __restrict__ work,
                                                       Result* __restrict__ results)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    const bool overflowed = counters[0] > cap;
    const uint64_t my_bits = bit_base[i], my_pieces = piece_first[i];
    auto good = [&](uint32_t pos, const uint8_t* page, uint32_t bytes) { return page_good(bits, my_bits, pos, overflowed, tables, page, bytes); };
    uint32_t n_pieces = 0;
    walk<Links>(s, i, src, packets, pieces + my_pieces, good, &results[i], &n_pieces);
    if (!n_pieces) return;
    const uint32_t at = atomicAdd(&counters[1], n_pieces);
    for (uint32_t k = 0; k < n_pieces; k++) work[at + k] = (uint32_t)my_pieces + k;
}

__global__ __launch_bounds__(kOggThreads) void ogg_gather_kernel(const Stream* __restrict__ streams, const Piece* __restrict__ pieces, const uint32_t* __restrict__ work,
                                                                 const uint32_t* __restrict__ counters, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const uint32_t n = counters[1];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u);
    const uint32_t stride = gridDim.x * kOggWaves;
    for (uint32_t k = blockIdx.x * kOggWaves + wave; k < n; k += stride) {
        const Piece g = pieces[work[k]];
        const Stream& s = streams[g.stream];
        ohmrx::gather_lane(src + s.src_offset + g.src_pos, dst + s.dst_offset + g.run_pos, g.bytes, threadIdx.x % 64u, 64u);
    }
}

// The verify and gather launches: a wave an item, at most kGroupsPerCu workgroups a CU (tests/test_gpu_ogg_textbook.py restates it)
uint32_t ogg_wave_blocks(uint64_t items, uint32_t cus)
{
    const uint64_t want = (items + kOggWaves - 1) / kOggWaves, cap = (uint64_t)cus * kGroupsPerCu;
    return (uint32_t)(want < cap ? want : cap);
}

int ogg_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Stream* streams)
{
    OggState& g = *b->ogg;
    OHGPU_TRY(state_events(g, 5));
    if (!g.n_streams) return OHGPU_OK;
    std::vector<OggTile> tiles;
    std::vector<uint64_t> bit_base(g.n_streams), piece_first(g.n_streams);
    uint64_t bits = 0, pieces = 0, cands = 0;
    for (size_t i = 0; i < g.n_streams; i++) {
        const Stream& s = streams[i];
        for (uint32_t pos = 0; pos + kHeaderBytes <= s.src_bytes; pos += kFindTile) tiles.push_back(OggTile{(uint32_t)i, pos});
        bit_base[i] = bits;
        piece_first[i] = pieces;
        g.follow_links = g.follow_links || (s.flags & kFollowLinks) != 0;
        bits += ((uint64_t)s.src_bytes + 31u) & ~(uint64_t)31u;
        pieces += piece_capacity(s);
        cands += s.src_bytes / 27u + 1u;
    }
    if (pieces > 0xffffffffull || cands > 0xffffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_ogg_batch_create: %llu source bytes are more than one batch takes", (unsigned long long)bits);
    g.n_tiles = (uint32_t)tiles.size(); g.cand_cap = (uint32_t)cands; g.piece_cap = (uint32_t)pieces; g.bits_bytes = (size_t)(bits / 8u);
    Tables tables;
    make_tables(&tables);
    OHGPU_TRY(dev_array(ctx, g, &g.d_streams, g.n_streams, streams));
    OHGPU_TRY(dev_array<Result>(ctx, g, &g.d_results, g.n_streams));
    OHGPU_TRY(dev_array(ctx, g, &g.d_bit_base, g.n_streams, bit_base.data()));
    OHGPU_TRY(dev_array(ctx, g, &g.d_piece_first, g.n_streams, piece_first.data()));
    OHGPU_TRY(dev_array(ctx, g, &g.d_tables, 1, &tables));
    OHGPU_TRY(dev_array<uint32_t>(ctx, g, &g.d_counters, 2));
    OHGPU_TRY(dev_array<Candidate>(ctx, g, &g.d_list, g.cand_cap));
    OHGPU_TRY(dev_array<Piece>(ctx, g, &g.d_pieces, g.piece_cap));
    OHGPU_TRY(dev_array<uint32_t>(ctx, g, &g.d_work, g.piece_cap));
    OHGPU_TRY(dev_array(ctx, g, &g.d_tiles, g.n_tiles, tiles.data()));
    OHGPU_TRY(dev_array<uint8_t>(ctx, g, &g.d_bits, g.bits_bytes));
    OHGPU_TRY(dev_array<Packet>(ctx, g, &g.d_packets, g.n_packets));
    if (g.n_packets) OHGPU_HIP_TRY_ALLOC(hipMemset(g.d_packets, 0, g.n_packets * sizeof(Packet)));
    OHGPU_HIP_TRY_ALLOC(hipStreamSynchronize(nullptr));                // (the fill is queued: a run on another stream must not meet it)
    return OHGPU_OK;
}

int ogg_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    OggState& g = *b->ogg;
    OHGPU_TRY(run_begin(g, s));      // (the lists serve one run at a time)
    const uint32_t ns = (uint32_t)g.n_streams;
    const uint32_t cus = ctx->num_cus > 0 ? (uint32_t)ctx->num_cus : 256u;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[0], s));
    OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_counters, 0, 2 * sizeof(uint32_t), s));
    if (g.bits_bytes) OHGPU_HIP_TRY_ALLOC(hipMemsetAsync(g.d_bits, 0, g.bits_bytes, s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(ogg_find_kernel, dim3(g.n_tiles), dim3(kOggThreads), 0, s, (const Stream*)g.d_streams, (const OggTile*)g.d_tiles, src, (Candidate*)g.d_list, g.cand_cap,
                           (uint32_t*)g.d_counters);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[1], s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(ogg_verify_kernel, dim3(ogg_wave_blocks(g.cand_cap, cus)), dim3(kOggThreads), 0, s, (const Stream*)g.d_streams, (const uint64_t*)g.d_bit_base,
                           (const Candidate*)g.d_list, g.cand_cap, (const uint32_t*)g.d_counters, (const Tables*)g.d_tables, src, (uint32_t*)g.d_bits);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[2], s));
    hipLaunchKernelGGL(g.follow_links ? ogg_chain_kernel<true> : ogg_chain_kernel<false>, dim3((ns + 63u) / 64u), dim3(64), 0, s, (const Stream*)g.d_streams, ns, (const uint64_t*)g.d_bit_base, (const uint64_t*)g.d_piece_first, src,
                       (const uint32_t*)g.d_bits, g.cand_cap, (uint32_t*)g.d_counters, (const Tables*)g.d_tables, (Packet*)g.d_packets, (Piece*)g.d_pieces, (uint32_t*)g.d_work,
                       (Result*)g.d_results);
    OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(g.ev[3], s));
    if (g.n_tiles) {
        hipLaunchKernelGGL(ogg_gather_kernel, dim3(ogg_wave_blocks(g.piece_cap, cus)), dim3(kOggThreads), 0, s, (const Stream*)g.d_streams, (const Piece*)g.d_pieces,
                           (const uint32_t*)g.d_work, (const uint32_t*)g.d_counters, src, dst);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(g, s);
}

}  // namespace ohgpu
