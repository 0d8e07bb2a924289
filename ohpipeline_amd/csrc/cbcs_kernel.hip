// cbcs_kernel.hip -- the second protected fragmented MPEG-4 family on the device (the text is csrc/cbcs_core.h over
// csrc/cenc_core.h and csrc/mp4_frag_core.h).  The launches have csrc/cenc_kernel.hip's shape, over work units (a 16-byte piece of a
// part of a sample) where that file counts keystream blocks:
//   walk            a lane per stream: mp4frag's walk under cbcs::Protection.  At every traf's end the lane follows the senc's entries --
//                   a chain, serial inside a traf -- and writes the stream's subsample rows and a record a sample (cbcs_core.h says why
//                   this is the walk's and no launch of its own).  It also writes the rows served into the sibling's descriptor, where
//                   packet_capacity stands, for the shared launches that follow.
//   run sums, carries, expand, finish
//                   csrc/mp4_frag_kernel.hip's own launches (mp4f_tables).
//   decrypt-gather  three launches:
//       rows        a workgroup per tile of the expansion: the public packet row of every sample, the exclusive prefix of the work
//                   units over the tile's gathered rows, the tile's sum, and the stream's cipher blocks (a wave's sum, one atomic).
//       tiles       a lane per stream, serial over its tiles: the units in front of each tile; the stream's units and blocks.
//       crypt       persistent, a wave per chunk of 64 consecutive work units of one stream, a lane a unit.  The chunk slots are laid out
//                   at create from the capacities (a stream has at most dst_capacity / 16 + packet_capacity + 3 subsample_capacity
//                   units).  The stream is the same for the whole wave, so its scheme, its pattern and its schedule -- the cipher's or
//                   the inverse cipher's, 44 words -- are read through wave-uniform indices and stay in scalar registers.  A lane finds
//                   tile, row and entry by three searches and runs cbcs::unit_lane.  Te0, Td0 and the inverse S-box are staged in the
//                   LDS (2304 bytes a workgroup); their reads are data-dependent, so bank conflicts are part of the cost, as the
//                   sibling measured.  A `cenc` part is cut at the keystream's block edges: every piece pays for exactly one
//                   keystream block, and whole-sample `cenc` costs what it costs the sibling.
//   plain           (kernel variant 1) one launch, a lane per stream: all of it in the serial text the CPU driver runs, the tables
//                   read from constant memory.
// Loads: the walk's are mp4_frag_kernel.hip's, the chain's lie inside a senc that was held to its box entry by entry; an IV lies inside
// that senc or inside the tenc; a sample is read only when emit() found it inside the stream, and a part only where the chain found its
// parts to sum to its size.  Stores: the stream's rows, run slots and subsample rows, its own records, or [dst_offset, + bytes_gathered).
// The scan, the tiles' prefix, the persistent loop and its searches, the plan of the slots and the run around the launches are
// csrc/protected_shell.h's (over csrc/frag_units.h), shared with csrc/cenc_kernel.hip: this file has the kernels' own parts.
#include "protected_shell.h"

namespace ohgpu {

constexpr cenc::Forward kCbcsHostForward = cenc::make_forward();
constexpr raopcore::Tables kCbcsHostInverse = raopcore::make_tables();
__constant__ const cenc::Forward kCbcsForward = kCbcsHostForward;
__constant__ const raopcore::Tables kCbcsInverse = kCbcsHostInverse;

__global__ __launch_bounds__(64) void cbcs_walk_kernel(const cbcs::Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, Stream* __restrict__ plain,
                                                       Result* __restrict__ results, cenc::Extra* __restrict__ extras, cbcs::More* __restrict__ more, Rec* __restrict__ recs,
                                                       RunRec* __restrict__ runrecs, cbcs::SubRow* __restrict__ subs, cbcs::SampleRec* __restrict__ samprecs,
                                                       unsigned long long* __restrict__ cipher_blocks)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const cbcs::Stream s = streams[i];
    uint32_t rows_cap;
    cbcs::walk(s, src + s.c.s.src_offset, false, subs + s.sub_first, samprecs + s.c.s.packet_first, &results[i], &extras[i], &more[i], &recs[i], runrecs + s.c.s.run_first,
               &rows_cap);
    plain[i].packet_capacity = rows_cap;       // what the carries, the expansion and finish() take for the stream's rows
    cipher_blocks[i] = 0u;
}

__global__ __launch_bounds__(kProtThreads) void cbcs_rows_kernel(const Stream* __restrict__ streams, const Rec* __restrict__ recs, const RunRec* __restrict__ runrecs,
                                                                 const Mp4fTile* __restrict__ tiles, const Result* __restrict__ results, const cenc::Extra* __restrict__ extras,
                                                                 const cbcs::More* __restrict__ more, const cbcs::SampleRec* __restrict__ samprecs,
                                                                 const Row* __restrict__ src_rows, Row* __restrict__ rows, uint64_t* __restrict__ unit_first,
                                                                 uint64_t* __restrict__ tile_units, unsigned long long* __restrict__ cipher_blocks)
{
    __shared__ uint64_t part[kProtWaves];
    const Mp4fTile tile = tiles[blockIdx.x];
    const Rec rec = recs[tile.stream];
    if (tile.s0 >= rec.rows) return;                                  // (uniform over the workgroup)
    const Stream st = streams[tile.stream];
    const Result& res = results[tile.stream];
    const RunRec* const runs = runrecs + st.run_first;
    const uint32_t kind = cbcs::kind_of(extras[tile.stream]);
    const cbcs::More m = more[tile.stream];
    const uint32_t first = tile.s0 + threadIdx.x * kProtPerThread;
    uint32_t n[kProtPerThread];
    uint64_t blocks = 0;
    for (uint32_t k = 0; k < kProtPerThread; k++) {
        const uint32_t s = first + k;
        n[k] = 0;
        if (s >= rec.rows) continue;
        Row from;
        uint32_t k_run, b;
        if (public_row(st, rec, res, runs, src_rows, rows, s, &from, &k_run)) {
            cbcs::sample_work(kind, m, samprecs + st.packet_first, s, from.bytes, &n[k], &b);
            blocks += b;
        }
    }
    for (uint32_t o = 32u; o; o >>= 1) blocks += (uint64_t)__shfl_down((unsigned long long)blocks, o);
    if (threadIdx.x % 64u == 0u && blocks) atomicAdd(&cipher_blocks[tile.stream], (unsigned long long)blocks);
    uint64_t before, total;
    tile_exclusive_scan(n, part, &before, &total);
    for (uint32_t k = 0; k < kProtPerThread; k++) {
        const uint32_t s = first + k;
        if (s < rec.rows) unit_first[st.packet_first + s] = before;
        before += n[k];
    }
    if (threadIdx.x == kProtThreads - 1u) tile_units[blockIdx.x] = total;
}

__global__ __launch_bounds__(64) void cbcs_tiles_kernel(uint32_t n, const Rec* __restrict__ recs, const uint32_t* __restrict__ tile_first, uint64_t* __restrict__ tile_units,
                                                        uint64_t* __restrict__ nunits, const unsigned long long* __restrict__ cipher_blocks, cenc::Extra* __restrict__ extras)
{
    tiles_body(n, recs, tile_first, tile_units, nunits, extras, [=](uint32_t i, uint64_t) { return (uint64_t)cipher_blocks[i]; });
}

__global__ __launch_bounds__(kProtThreads) void cbcs_crypt_kernel(const Stream* __restrict__ streams, uint32_t n_streams, const Rec* __restrict__ recs,
                                                                  const cenc::Extra* __restrict__ extras, const cbcs::More* __restrict__ more,
                                                                  const uint32_t* __restrict__ tile_first, const uint64_t* __restrict__ tile_units,
                                                                  const uint64_t* __restrict__ chunk_first, uint64_t n_chunks, const uint64_t* __restrict__ nunits,
                                                                  const uint32_t* __restrict__ keys, const Row* __restrict__ src_rows, const Row* __restrict__ rows,
                                                                  const uint64_t* __restrict__ unit_first, const cbcs::SampleRec* __restrict__ samprecs,
                                                                  const cbcs::SubRow* __restrict__ subs, const uint32_t* __restrict__ sub_first,
                                                                  const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    __shared__ uint32_t te0[256];
    __shared__ uint32_t td0[256];
    __shared__ uint32_t isbox[64];
    te0[threadIdx.x] = kCbcsForward.te0[threadIdx.x];
    td0[threadIdx.x] = kCbcsInverse.td0[threadIdx.x];
    if (threadIdx.x < 64u) {
        uint32_t v;
        __builtin_memcpy(&v, kCbcsInverse.isbox + 4u * threadIdx.x, 4);
        isbox[threadIdx.x] = v;
    }
    __syncthreads();
    cbcs::Tables t;
    t.te0 = te0; t.td0 = td0; t.isbox = (const uint8_t*)isbox;
    unit_loop(streams, n_streams, recs, tile_first, tile_units, chunk_first, n_chunks, nunits, [=](uint32_t r) { return unit_first[r]; },
        [=](uint32_t i, const Stream& st, uint32_t r, uint32_t j) {
            const Row from = src_rows[r], to = rows[r];
            const uint32_t kind = __builtin_amdgcn_readfirstlane(cbcs::kind_of(extras[i]));
            const uint32_t pattern = __builtin_amdgcn_readfirstlane((uint32_t)more[i].crypt << 8 | more[i].skip);
            const uint32_t iv_bytes = __builtin_amdgcn_readfirstlane(extras[i].iv_size ? (uint32_t)extras[i].iv_size : (uint32_t)more[i].civ_size);
            cbcs::SubRow e = cbcs::whole_sample(kind, from.bytes);
            uint32_t v = j;
            cbcs::SampleIv iv = {};
            if (kind != cbcs::kCopy) {
                const cbcs::SampleRec sr = samprecs[r];
                iv = cbcs::read_sample_iv(src + st.src_offset, sr.iv_pos, iv_bytes);
                if (sr.n_sub) {
                    const cbcs::SubRow* const mine = subs + sub_first[i] + sr.sub_first;
                    e = mine[cbcs::entry_of(mine, sr.n_sub, j)];
                    v = j - e.unit_first;
                }
            }
            cbcs::unit_lane(src + from.src_offset, dst + to.src_offset, e, v, kind, pattern >> 8, pattern & 0xffu, keys + (size_t)i * cbcs::kKeyWords, iv, t);
        });
}

__global__ __launch_bounds__(64) void cbcs_plain_kernel(const cbcs::Stream* __restrict__ streams, uint32_t n, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                        Result* __restrict__ results, cenc::Extra* __restrict__ extras, cbcs::More* __restrict__ more, Rec* __restrict__ recs,
                                                        RunRec* __restrict__ runrecs, Run* __restrict__ runs, Row* __restrict__ src_rows, Row* __restrict__ rows,
                                                        Sample* __restrict__ samples, cbcs::SubRow* __restrict__ subs, cbcs::SampleRec* __restrict__ samprecs,
                                                        const uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const cbcs::Stream cs = streams[i];
    Stream s = cs.c.s;
    const uint8_t* const base = src + s.src_offset;
    RunRec* const my = runrecs + s.run_first;
    Result r;
    Rec rec;
    cenc::Extra x;
    cbcs::More m;
    uint32_t rows_cap;
    cbcs::walk(cs, base, false, subs + cs.sub_first, samprecs + s.packet_first, &r, &x, &m, &rec, my, &rows_cap);
    s.packet_capacity = rows_cap;
    for (uint32_t k = 0; k < rec.runs_written; k++)
        if (needs_sums(my[k])) totals_serial(base, my[k], my[k].samples, &my[k].bytes, &my[k].frames);
    carries(s, &rec, my, runs + s.run_first, &r);
    expand_serial(s, base, rec, my, src_rows + s.packet_first, samples + s.packet_first, &r);
    finish(s, &rec, my, src_rows + s.packet_first, &r);
    cbcs::Tables t;
    t.te0 = kCbcsForward.te0; t.td0 = kCbcsInverse.td0; t.isbox = kCbcsInverse.isbox;
    cbcs::gather_serial(cs, src, dst, rec, my, src_rows + s.packet_first, r, keys + (size_t)i * cbcs::kKeyWords, t, subs + cs.sub_first, samprecs + s.packet_first, m,
                        rows + s.packet_first, &x);
    results[i] = r;
    extras[i] = x;
    more[i] = m;
    recs[i] = rec;
}

int cbcs_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const cbcs::Stream* streams)
{
    CbcsState& g = *b->cbcs;
    const size_t n = g.n_streams;
    std::vector<Stream> plain(n);
    std::vector<cbcs::Stream> stripped(streams, streams + n);          // the device's copy has no key: the schedules are all it gets
    std::vector<uint32_t> sub_first(n);
    for (size_t i = 0; i < n; i++) {
        plain[i] = streams[i].c.s;
        sub_first[i] = streams[i].sub_first;
        for (uint8_t& k : stripped[i].c.key) k = 0;
    }
    OHGPU_TRY(protected_plan<uint64_t>(ctx, g, plain, stripped, "ohgpu_cbcs_batch_create", [&](size_t i) { return streams[i].sub_capacity; }));
    if (!n) return OHGPU_OK;
    OHGPU_TRY(dev_array<cbcs::More>(ctx, g, &g.d_more, n));
    OHGPU_TRY(dev_array<cbcs::SampleRec>(ctx, g, &g.d_samprecs, g.n_packets));
    OHGPU_TRY(dev_array<cbcs::SubRow>(ctx, g, &g.d_subs, g.n_subsamples));
    OHGPU_TRY(dev_array<uint64_t>(ctx, g, &g.d_cipher_blocks, n));
    OHGPU_TRY(dev_array(ctx, g, &g.d_sub_first, n, sub_first.data()));
    return OHGPU_OK;
}

int cbcs_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s)
{
    CbcsState& g = *b->cbcs;
    const uint32_t ns = (uint32_t)g.n_streams, lane_blocks = (ns + 63u) / 64u;
    const cbcs::Stream* const cstreams = (const cbcs::Stream*)g.d_cstreams;
    Result* const results = (Result*)g.d_results;
    cenc::Extra* const extras = (cenc::Extra*)g.d_extras;
    cbcs::More* const more = (cbcs::More*)g.d_more;
    Rec* const recs = (Rec*)g.d_recs;
    RunRec* const runrecs = (RunRec*)g.d_runrecs;
    cbcs::SubRow* const subs = (cbcs::SubRow*)g.d_subs;
    cbcs::SampleRec* const samprecs = (cbcs::SampleRec*)g.d_samprecs;
    unsigned long long* const cipher_blocks = (unsigned long long*)g.d_cipher_blocks;
    const uint32_t* const keys = (const uint32_t*)g.d_keys;
    return protected_run(g, src, s,
        [&] {
            hipLaunchKernelGGL(cbcs_plain_kernel, dim3(lane_blocks), dim3(64), 0, s, cstreams, ns, src, dst, results, extras, more, recs, runrecs, (Run*)g.d_runs,
                               (Row*)g.d_packets, (Row*)g.d_rows, (Sample*)g.d_samples, subs, samprecs, keys);
        },
        [&] {
            hipLaunchKernelGGL(cbcs_walk_kernel, dim3(lane_blocks), dim3(64), 0, s, cstreams, ns, src, (Stream*)g.d_streams, results, extras, more, recs, runrecs, subs, samprecs,
                               cipher_blocks);
        },
        [&]() -> int {
            if (g.n_tiles) {
                hipLaunchKernelGGL(cbcs_rows_kernel, dim3(g.n_tiles), dim3(kProtThreads), 0, s, (const Stream*)g.d_streams, (const Rec*)recs, (const RunRec*)runrecs,
                                   (const Mp4fTile*)g.d_tiles, (const Result*)results, (const cenc::Extra*)extras, (const cbcs::More*)more, (const cbcs::SampleRec*)samprecs,
                                   (const Row*)g.d_packets, (Row*)g.d_rows, (uint64_t*)g.d_row_first, (uint64_t*)g.d_tile_units, cipher_blocks);
                OHGPU_HIP_TRY_ALLOC(hipGetLastError());
            }
            // (with no tile too: the streams' units and blocks are this launch's to write)
            hipLaunchKernelGGL(cbcs_tiles_kernel, dim3(lane_blocks), dim3(64), 0, s, ns, (const Rec*)recs, (const uint32_t*)g.d_tile_first, (uint64_t*)g.d_tile_units,
                               (uint64_t*)g.d_nunits, (const unsigned long long*)cipher_blocks, extras);
            OHGPU_HIP_TRY_ALLOC(hipGetLastError());
            if (!g.n_tiles || !g.crypt_blocks) return OHGPU_OK;
            hipLaunchKernelGGL(cbcs_crypt_kernel, dim3(g.crypt_blocks), dim3(kProtThreads), 0, s, (const Stream*)g.d_streams, ns, (const Rec*)recs, (const cenc::Extra*)extras,
                               (const cbcs::More*)more, (const uint32_t*)g.d_tile_first, (const uint64_t*)g.d_tile_units, (const uint64_t*)g.d_chunk_first, g.n_chunks,
                               (const uint64_t*)g.d_nunits, keys, (const Row*)g.d_packets, (const Row*)g.d_rows, (const uint64_t*)g.d_row_first,
                               (const cbcs::SampleRec*)samprecs, (const cbcs::SubRow*)subs, (const uint32_t*)g.d_sub_first, src, dst);
            OHGPU_HIP_TRY_ALLOC(hipGetLastError());
            return OHGPU_OK;
        });
}

}  // namespace ohgpu
