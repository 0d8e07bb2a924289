// raop_rx_kernel.hip -- the RAOP receiver on the device (the text of parse, of the serial sequencer and of the table is
// csrc/raop_rx_core.h).
//   parse      a lane per datagram, one launch sized to the table: up to five aligned dword loads, a record of 48 bytes and a key of
//              16 bytes out.  The keys lie side by side, so the 64 lanes of the sequencer read 64 datagrams in one coalesced load.
//   sequence   the wave route: a wave per stream, a workgroup of one wave.  Everything the reference carries from one datagram to the
//              next is wave-uniform (the stream descriptor and the key of the datagram at hand are read through uniform indices, every
//              count comes out of a ballot); the waiting frames of a repair live in the lanes, iRepairFirst in lane 0 and
//              iRepairFrames behind it, as the frame's 16 bits and the datagram's index.
//                fast path   while running, started, no resume pending, no repair and no delay due: the lanes load the next 64 keys,
//                            a ballot of "audio, of the session, seq == frame + 1 + lane" is taken and its leading ones are that
//                            many OUTPUTs at once.  None: the datagram at hand takes the step below.
//                one step    raoprx::Flow::front decides what ProtocolRaop decides; the branches of Repair() are a ballot of signed
//                            16-bit differences (the insertion point, or a duplicate), a shift up by one lane (the insert), a
//                            ballot of "waiting seq == frame + 1 + lane" whose leading ones are the drain and a shift down by that
//                            count, and a comparison of the occupied count with max_frames + 1 (buffer full).
//              No LDS and no scratch memory: the build's resource report says 0 bytes for both.
//              The plain route (ohgpu_set_kernel_variant(1)): a lane per stream runs raoprx::sequence, the waiting list in a
//              workspace of 64 words a stream.
//   table      a lane per datagram: an OUTPUT record's row goes to the stream's rows at its order, a row behind the last output reads
//              zero.
// Every index is a datagram index inside the stream's range [first_datagram, first_datagram + n_datagrams), which
// ohgpu_raop_rx_batch_check placed inside the tables; every load of a datagram lies inside [src_offset, src_offset + bytes), which the
// same check placed inside the source arena.  Nothing is written outside the batch's own arrays.
#include <hip/hip_runtime.h>

#include "api_common.h"

namespace ohgpu {

using namespace raoprx;

constexpr uint32_t kRaopRxThreads = 256;

__global__ __launch_bounds__(kRaopRxThreads) void raop_rx_parse_kernel(const Datagram* __restrict__ grams, uint32_t n, const uint8_t* __restrict__ src,
                                                                       Record* __restrict__ recs, Key* __restrict__ keys)
{
    const uint32_t k = blockIdx.x * kRaopRxThreads + threadIdx.x;
    if (k >= n) return;
    const Datagram g = grams[k];
    parse(src + g.src_offset, g.bytes, g.port, &recs[k], &keys[k]);
}

__global__ __launch_bounds__(64) void raop_rx_sequence_plain_kernel(const Stream* __restrict__ streams, uint32_t n, const Key* __restrict__ keys, Record* __restrict__ recs,
                                                                    uint64_t* __restrict__ slots, StreamResult* __restrict__ results)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Stream s = streams[i];
    sequence(s, keys + s.first_datagram, recs + s.first_datagram, slots + (size_t)i * kSlots, &results[i]);
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }      // (the same in every lane: says so to the compiler)
__device__ __forceinline__ uint32_t leading_ones(uint64_t b) { return ~b ? (uint32_t)__builtin_ctzll(~b) : 64u; }

__global__ __launch_bounds__(64) void raop_rx_sequence_wave_kernel(const Stream* __restrict__ streams, const Key* __restrict__ keys, Record* __restrict__ recs,
                                                                   StreamResult* __restrict__ results)
{
    const uint32_t lane = threadIdx.x;
    const Stream s = streams[blockIdx.x];
    const Key* const ks = keys + s.first_datagram;
    Record* const rs = recs + s.first_datagram;
    const uint32_t n = s.n_datagrams, max_frames = s.max_frames;
    Flow f;
    f.st = s.state_in;
    f.n_output = 0;
    uint32_t count = 0, stop = kStopNone, i = 0;
    uint32_t wseq = 0, widx = 0;                                      // this lane's waiting frame, lane < count
    while (i < n && stop == kStopNone) {
        if (f.st.running && f.st.started && !f.st.resume_pending && count == 0 && !f.delay_due()) {
            const uint32_t at = i + lane;
            Key k = {};
            if (at < n) k = ks[at];
            const bool next = at < n && k.kind == kKindAudio && k.ssrc == f.st.session_id && (uint32_t)k.seq == (uint32_t)(uint16_t)(f.st.frame + 1u + lane);
            const uint32_t m = uniform(leading_ones(__ballot(next)));
            if (lane < m) {
                rs[at].disposition = kOutput;
                rs[at].order = f.n_output + lane;
            }
            f.st.frame = (uint16_t)(f.st.frame + m);
            f.n_output += m;
            i += m;
            if (m) continue;
        }
        const Key k = ks[i];                                          // (a uniform index)
        uint32_t events, order = 0;
        uint32_t disp = f.front(k, &events);
        if (disp == kNone) {
            const int32_t d = diff16(k.seq, f.st.frame);
            if (!f.st.running) {
                f.st.frame = k.seq;
                f.st.running = 1;
                disp = kOutput;
                events |= f.delay_event();
                order = f.n_output++;
            } else if (d < 1) {
                disp = kDuplicate;
                if (!k.resend) stop = kStopRestarted;
            } else if (d == 1) {
                f.st.frame++;
                disp = kOutput;
                events |= f.delay_event();
                order = f.n_output++;
                const bool ready = lane < count && wseq == (uint32_t)(uint16_t)(f.st.frame + 1u + lane);
                const uint32_t m = uniform(leading_ones(__ballot(ready)));
                if (lane < m) {
                    rs[widx].disposition = kOutput;
                    rs[widx].order = f.n_output + lane;
                }
                f.st.frame = (uint16_t)(f.st.frame + m);
                f.n_output += m;
                wseq = __shfl(wseq, (lane + m) & 63u);
                widx = __shfl(widx, (lane + m) & 63u);
                count -= m;
            } else {
                const uint64_t not_below = __ballot(lane < count && diff16(k.seq, wseq) <= 0);
                const uint32_t p = not_below ? (uint32_t)__builtin_ctzll(not_below) : count;
                const bool dup = not_below && uniform(__shfl(wseq, p)) == (uint32_t)k.seq;
                if (dup) disp = kDuplicate;
                else if (count == max_frames + 1u) stop = kStopBufferFull;
                else {
                    const uint32_t up_seq = __shfl_up(wseq, 1), up_idx = __shfl_up(widx, 1);
                    if (lane > p) { wseq = up_seq; widx = up_idx; }
                    if (lane == p) { wseq = k.seq; widx = i; }
                    count++;
                    disp = kPending;
                }
            }
            if (stop != kStopNone) {                                  // RepairReset
                if (lane < count) {
                    rs[widx].disposition = kDroppedByReset;
                    rs[widx].order = 0;
                }
                count = 0;
                f.stop();
                disp = kDroppedByReset;
            }
        }
        if (lane == 0) {
            rs[i].disposition = (uint8_t)disp;
            rs[i].events = (uint8_t)events;
            rs[i].order = order;
        }
        i++;
    }
    for (uint32_t j = i + lane; j < n; j += 64u) {
        rs[j].disposition = kNotReached;
        rs[j].events = 0;
        rs[j].order = 0;
    }
    // TimerRepairExpired's ranges (raoprx::ranges, a lane per waiting frame): range 0 is lane 0's, range r > 0 belongs to the lane of
    // the r-th gap, and slot `lane` of the result is written by that lane alone
    Range mine = {0u, 0u};
    uint32_t n_ranges = 0;
    if (lane < count) rs[widx].order = lane;                          // the replay's order
    if (count) {
        const uint32_t below = __shfl_up(wseq, 1);
        const uint32_t start = lane == 0 ? (uint32_t)(uint16_t)(f.st.frame + 1u) : (uint32_t)(uint16_t)(below + 1u);
        const uint32_t end = (uint32_t)((int32_t)wseq - 1);
        const uint64_t gaps = __ballot(lane >= 1 && lane < count && (int32_t)wseq - (int32_t)start > 0);
        const uint32_t limit = max_ranges(max_frames);
        const uint32_t start0 = uniform(start), end0 = uniform(end);
        if (lane == 0) { mine.start = start0; mine.end = end0; }
        n_ranges = 1;
        for (uint64_t g = gaps; g && n_ranges < limit; g &= g - 1, n_ranges++) {
            const uint32_t from = (uint32_t)__builtin_ctzll(g);
            const uint32_t gs = __shfl(start, from), ge = __shfl(end, from);
            if (lane == n_ranges) { mine.start = gs; mine.end = ge; }
        }
    }
    StreamResult* const out = &results[blockIdx.x];
    if (lane < (uint32_t)kMaxRanges) out->ranges[lane] = mine;
    if (lane == 0) {
        out->state_out = f.st;
        out->n_output = f.n_output;
        out->n_pending = count;
        out->stop_reason = stop;
        out->n_ranges = n_ranges;
    }
}

__global__ __launch_bounds__(kRaopRxThreads) void raop_rx_table_kernel(const Stream* __restrict__ streams, const Datagram* __restrict__ grams, const uint32_t* __restrict__ owner,
                                                                       const Record* __restrict__ recs, const StreamResult* __restrict__ results, uint32_t n,
                                                                       PacketRow* __restrict__ rows)
{
    const uint32_t k = blockIdx.x * kRaopRxThreads + threadIdx.x;
    if (k >= n) return;
    const uint32_t o = owner[k], first = streams[o].first_datagram;
    table_row(grams[k], recs[k], k - first, results[o].n_output, rows + first);
}

int raop_rx_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Stream* streams, const Datagram* datagrams)
{
    RaopRxState& r = *b->raoprx;
    std::vector<uint32_t> owner(r.n_datagrams);
    for (size_t i = 0; i < r.n_streams; i++)
        for (uint32_t k = 0; k < streams[i].n_datagrams; k++) owner[streams[i].first_datagram + k] = (uint32_t)i;
    OHGPU_TRY(state_events(r, 4));
    OHGPU_TRY(dev_array(ctx, r, &r.d_streams, r.n_streams, streams));
    OHGPU_TRY(dev_array<StreamResult>(ctx, r, &r.d_results, r.n_streams));
    if (r.plain) OHGPU_TRY(dev_array<uint64_t>(ctx, r, &r.d_slots, r.n_streams * kSlots));
    OHGPU_TRY(dev_array(ctx, r, &r.d_datagrams, r.n_datagrams, datagrams));
    OHGPU_TRY(dev_array(ctx, r, &r.d_owner, r.n_datagrams, owner.data()));
    OHGPU_TRY(dev_array<Record>(ctx, r, &r.d_records, r.n_datagrams));
    OHGPU_TRY(dev_array<Key>(ctx, r, &r.d_keys, r.n_datagrams));
    OHGPU_TRY(dev_array<PacketRow>(ctx, r, &r.d_rows, r.n_datagrams));
    return OHGPU_OK;
}

int raop_rx_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, hipStream_t s)
{
    RaopRxState& r = *b->raoprx;
    OHGPU_TRY(run_begin(r, s));      // (the records serve one run at a time)
    const uint32_t ng = (uint32_t)r.n_datagrams, ns = (uint32_t)r.n_streams;
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(r.ev[0], s));
    if (ng) {
        hipLaunchKernelGGL(raop_rx_parse_kernel, dim3((ng + kRaopRxThreads - 1) / kRaopRxThreads), dim3(kRaopRxThreads), 0, s, (const Datagram*)r.d_datagrams, ng, src,
                           (Record*)r.d_records, (Key*)r.d_keys);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(r.ev[1], s));
    if (ns && r.plain) {
        hipLaunchKernelGGL(raop_rx_sequence_plain_kernel, dim3((ns + 63u) / 64u), dim3(64), 0, s, (const Stream*)r.d_streams, ns, (const Key*)r.d_keys, (Record*)r.d_records,
                           (uint64_t*)r.d_slots, (StreamResult*)r.d_results);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    } else if (ns) {
        hipLaunchKernelGGL(raop_rx_sequence_wave_kernel, dim3(ns), dim3(64), 0, s, (const Stream*)r.d_streams, (const Key*)r.d_keys, (Record*)r.d_records,
                           (StreamResult*)r.d_results);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    OHGPU_HIP_TRY_ALLOC(hipEventRecord(r.ev[2], s));
    if (ng) {
        hipLaunchKernelGGL(raop_rx_table_kernel, dim3((ng + kRaopRxThreads - 1) / kRaopRxThreads), dim3(kRaopRxThreads), 0, s, (const Stream*)r.d_streams,
                           (const Datagram*)r.d_datagrams, (const uint32_t*)r.d_owner, (const Record*)r.d_records, (const StreamResult*)r.d_results, ng, (PacketRow*)r.d_rows);
        OHGPU_HIP_TRY_ALLOC(hipGetLastError());
    }
    return run_end(r, s);
}

}  // namespace ohgpu
