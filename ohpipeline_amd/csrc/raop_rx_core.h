// raop_rx_core.h -- the receiving end of RAOP: what stands between a received AirPlay datagram and the packet table
// ohgpu_raop_batch_create takes.  Every function is __host__ __device__: csrc/raop_rx_kernel.hip runs this text on the device,
// tests/cpp/raop_rx_core_driver.cpp runs the same text on the CPU under the sanitizers.
//
//   parse      a datagram -> a Record and a Key.  The wire, all integers big-endian, the datagram's start at a multiple of 4:
//                audio port      0 V P X CC | 1 M type | 2 u16 seq | 4 u32 timestamp | 8 u32 ssrc | 12 payload
//                control, 0x54   0..3 the same | 4 u32 rtp timestamp - latency | 8 u32 ntp secs | 12 u32 ntp fraction | 16 u32 rtp timestamp
//                control, 0x56   0..3 the same | 4 a whole audio datagram (its payload at 16)
//              The order of the checks IS the definition of the statuses: more than 1472 bytes OVERSIZE; fewer than 4 TRUNCATED; on the
//              audio port fewer than 8 behind them TRUNCATED; on the control port a type (byte 1 & 0x7f) of 0x54 with fewer than 16
//              bytes behind the header TRUNCATED, of 0x56 whose inner datagram has fewer than 4 bytes or fewer than 8 behind them
//              TRUNCATED, any other type OTHER_TYPE.  The RTP version and the audio payload type are not looked at (the reference
//              has both checks commented out: senders answer resends with version 0 and type 0).
//   sequence   a stream's records in arrival order -> dispositions, event bits, the output order, the state to carry on and the resend
//              ranges.  Flow is what ProtocolRaop and RaopControlServer decide per datagram (the flush window, start and resume, the
//              session, the latency and its 441-sample rule); the repairer is Repairer<MaxFrames>, read as what it is: every frame
//              that waits was at most 32767 ahead of iFrame when it came, iFrame only moves towards the least of them, so the waiting
//              frames are totally ordered by their signed 16-bit distance and ONE sorted list -- iRepairFirst at place 0,
//              iRepairFrames behind it -- holds them.  All of Repair()'s insert branches are then "the first place whose frame is
//              not below the new one: equal, a duplicate; else full, or insert there".  The serial repairer below keeps the list
//              in a workspace of 64 words; the wave kernel keeps it in the lanes of a wave.
//   table      an OUTPUT record -> its row of the packet table.
#pragma once

#include <stdint.h>

#include "field_bytes.h"

#if defined(__HIPCC__)
#define RAOPRX_HD __host__ __device__ __forceinline__
#else
#define RAOPRX_HD inline
#endif

namespace raoprx {

enum { kHeaderBytes = 4, kAudioHeaderBytes = 8, kSyncHeaderBytes = 16, kMaxPacketBytes = 1472 };
enum { kTypeSync = 0x54, kTypeResendResponse = 0x56 };
enum { kMinDelayChangeSamples = 441, kMaxFramesLimit = 63, kMaxRanges = 31, kSlots = 64 };
enum { kPortAudio = 0, kPortControl = 1 };
enum Status : uint8_t { kOk = 0, kTruncated = 1, kOversize = 2, kOtherType = 3 };
enum Disposition : uint8_t { kNone = 0, kOutput = 1, kDuplicate = 2, kPending = 3, kDroppedByReset = 4, kFlushed = 5, kWrongSession = 6, kSync = 7, kIgnored = 8, kNotReached = 9 };
enum { kEventNewStream = 1, kEventDelay = 2 };
enum { kStopNone = 0, kStopBufferFull = 1, kStopRestarted = 2 };
enum { kKindNone = 0, kKindAudio = 1, kKindSync = 2 };

struct Datagram {             // 16 bytes = ohgpu_raop_rx_datagram
    uint64_t src_offset;
    uint32_t bytes;
    uint8_t  port, reserved[3];
};
struct State {                // 32 bytes = ohgpu_raop_rx_state
    uint32_t flush_seq, flush_time, session_id, latency, control_latency;
    uint16_t frame;
    uint8_t  running, started, resume_pending, reserved[7];
};
struct Stream {               // 48 bytes = ohgpu_raop_rx_stream
    uint32_t first_datagram, n_datagrams, max_frames, reserved;
    State    state_in;
};
struct Record {               // 48 bytes = ohgpu_raop_rx_record
    uint8_t  status, disposition, events, resend;
    uint8_t  marker, extension, type, port;
    uint16_t seq, payload_offset;
    uint32_t payload_bytes, timestamp, ssrc;
    uint32_t sync[4];
    uint32_t order, reserved;
};
struct Key {                  // 16 bytes: what the sequencer reads of a datagram
    uint16_t seq;
    uint8_t  kind, resend;
    uint32_t ssrc, timestamp, latency;
};
struct Range { uint32_t start, end; };
struct StreamResult {         // 296 bytes = ohgpu_raop_rx_stream_result
    State    state_out;
    uint32_t n_output, n_pending, stop_reason, n_ranges;
    Range    ranges[kMaxRanges];
};
struct PacketRow {            // 16 bytes = ohgpu_alac_packet
    uint64_t src_offset;
    uint32_t bytes, reserved;
};
static_assert(sizeof(Datagram) == 16 && sizeof(State) == 32 && sizeof(Stream) == 48 && sizeof(Record) == 48 && sizeof(Key) == 16 && sizeof(StreamResult) == 296 &&
              sizeof(PacketRow) == 16, "RAOP receiver layouts");

// ---- phase 1.  `gram` is the datagram's first byte, at a multiple of 4; bytes [0, bytes) of it are read and no other: every field
// below is a whole dword at a multiple of 4 that the checks in front of it have placed inside the datagram.
RAOPRX_HD void parse_audio(const uint8_t* gram, uint32_t bytes, uint32_t at, uint32_t w, Record& r, Key& k)
{
    r.status = kOk;
    r.extension = (uint8_t)((w >> 28) & 1u);
    r.marker = (uint8_t)((w >> 23) & 1u);
    r.type = (uint8_t)((w >> 16) & 0x7fu);
    r.seq = (uint16_t)w;
    r.timestamp = fieldbytes::be32(gram, at + 4u);
    r.ssrc = fieldbytes::be32(gram, at + 8u);
    r.payload_offset = (uint16_t)(at + kHeaderBytes + kAudioHeaderBytes);
    r.payload_bytes = bytes - r.payload_offset;
    k.seq = r.seq;
    k.kind = kKindAudio;
    k.ssrc = r.ssrc;
    k.timestamp = r.timestamp;
}
RAOPRX_HD void parse(const uint8_t* gram, uint32_t bytes, uint32_t port, Record* out, Key* key)
{
    Record r = {};
    Key k = {};
    r.port = (uint8_t)port;
    r.disposition = kIgnored;
    if (bytes > (uint32_t)kMaxPacketBytes) r.status = kOversize;
    else if (bytes < (uint32_t)kHeaderBytes) r.status = kTruncated;
    else {
        const uint32_t w0 = fieldbytes::be32(gram, 0), behind = bytes - kHeaderBytes, type = (w0 >> 16) & 0x7fu;
        r.status = kTruncated;
        if (port == (uint32_t)kPortAudio) {
            if (behind >= (uint32_t)kAudioHeaderBytes) parse_audio(gram, bytes, 0u, w0, r, k);
        } else if (type == (uint32_t)kTypeSync) {
            if (behind >= (uint32_t)kSyncHeaderBytes) {
                r.status = kOk;
                r.extension = (uint8_t)((w0 >> 28) & 1u);
                r.marker = (uint8_t)((w0 >> 23) & 1u);
                r.type = (uint8_t)type;
                r.seq = (uint16_t)w0;
                for (uint32_t j = 0; j < 4u; j++) r.sync[j] = fieldbytes::be32(gram, 4u + 4u * j);
                k.seq = r.seq;
                k.kind = kKindSync;
                k.latency = r.sync[3] - r.sync[0];
            }
        } else if (type == (uint32_t)kTypeResendResponse) {
            if (behind >= (uint32_t)kHeaderBytes && behind - kHeaderBytes >= (uint32_t)kAudioHeaderBytes) {
                parse_audio(gram, bytes, kHeaderBytes, fieldbytes::be32(gram, kHeaderBytes), r, k);
                r.resend = k.resend = 1;
            }
        } else {
            r.status = kOtherType;
            r.type = (uint8_t)type;
        }
    }
    *out = r;
    *key = k;
}

// ---- phase 2, what both sequencers share.  Flow: a stream's scalars between two datagrams.
RAOPRX_HD int32_t diff16(uint32_t a, uint32_t b) { return (int32_t)(int16_t)(uint16_t)(a - b); }      // TInt16 diff = a - b

struct Flow {
    State    st;
    uint32_t n_output;

    // ProtocolRaop::OutputAudio's rule (ProtocolRaop.cpp:705-743): true when the next frame that goes out carries a delay
    RAOPRX_HD bool delay_due() const
    {
        const uint32_t d = st.control_latency > st.latency ? st.control_latency - st.latency : st.latency - st.control_latency;
        return d >= (uint32_t)kMinDelayChangeSamples;
    }
    RAOPRX_HD uint32_t delay_event()
    {
        if (!delay_due()) return 0;
        st.latency = st.control_latency;
        return kEventDelay;
    }
    // What happens to a datagram in front of the repairer (RaopControlServer::Run, ProtocolRaop::ProcessPacket :782-829 and
    // ProcessStreamStartOrResume :882-926).  kNone: it goes on to the repairer.  *events gets NEW_STREAM (and DELAY for a first start).
    RAOPRX_HD uint32_t front(const Key& k, uint32_t* events)
    {
        *events = 0;
        if (k.kind == kKindNone) return kIgnored;
        if (k.kind == kKindSync) { st.control_latency = k.latency; return kSync; }
        if (st.resume_pending && (uint32_t)k.seq <= st.flush_seq && k.timestamp <= st.flush_time) return kFlushed;
        if (!st.started || st.resume_pending) {
            if (st.session_id == 0) st.session_id = k.ssrc;
            *events = kEventNewStream;
            if (!st.started) { st.latency = st.control_latency; *events |= kEventDelay; }
            st.started = 1;
            st.resume_pending = 0;
            st.flush_seq = st.flush_time = 0;
        }
        return st.session_id == k.ssrc ? (uint32_t)kNone : (uint32_t)kWrongSession;
    }
    // RepairReset + OutputDiscontinuity, as far as the state goes
    RAOPRX_HD void stop()
    {
        st.running = 0;
        st.resume_pending = 1;
    }
};

// TimerRepairExpired's ranges (ProtocolRaop.h:740-789) from the sorted waiting frames w(0) .. w(count - 1), count >= 1, as the timer
// would make them now.  TUint16 operands promoted to int: `end - 1` of a first waiting frame 0 is -1, which Set(TUint, TUint) stores as
// 0xffffffff; a gap whose start lies behind the wrap of its end (end - start <= 0 as ints) asks for nothing.
RAOPRX_HD uint32_t max_ranges(uint32_t max_frames) { const uint32_t m = max_frames / 2u; return m ? m : 1u; }     // (max_frames 1: the reference has no slot at all)
template <typename W>
RAOPRX_HD uint32_t ranges(uint32_t frame, uint32_t count, uint32_t max_frames, W&& w, Range* out)
{
    const uint32_t limit = max_ranges(max_frames);
    uint32_t n = 0;
    uint32_t start = (uint16_t)(frame + 1u), end = w(0);
    out[n].start = start;
    out[n].end = (uint32_t)((int32_t)end - 1);
    n++;
    for (uint32_t i = 1; n < limit && i < count; i++) {
        start = (uint16_t)(end + 1u);
        end = w(i);
        if ((int32_t)end - (int32_t)start > 0) {
            out[n].start = start;
            out[n].end = (uint32_t)((int32_t)end - 1);
            n++;
        }
    }
    return n;
}

// The serial sequencer: a stream's keys and records, `slots` kSlots words of workspace (the waiting list: datagram index << 16 | seq).
struct Serial {
    Flow      f;
    uint32_t  count;          // waiting frames: 0 outside a repair
    uint32_t  max_frames;
    uint64_t* slots;
    Record*   recs;

    RAOPRX_HD static uint32_t seq_of(uint64_t slot) { return (uint32_t)(slot & 0xffffu); }
    RAOPRX_HD static uint32_t index_of(uint64_t slot) { return (uint32_t)(slot >> 16); }
    RAOPRX_HD void output(uint32_t i, uint32_t events)
    {
        recs[i].disposition = kOutput;
        recs[i].events = (uint8_t)(events | f.delay_event());
        recs[i].order = f.n_output++;
    }
    RAOPRX_HD void reset()
    {
        for (uint32_t k = 0; k < count; k++) { Record& r = recs[index_of(slots[k])]; r.disposition = kDroppedByReset; r.order = 0; }
        count = 0;
        f.stop();
    }
    // Repairer::OutputAudio and Repair (ProtocolRaop.h:530-583, 619-738) for record i; the stop reason when the stream ends here
    RAOPRX_HD uint32_t take(uint32_t i, const Key& k, uint32_t events)
    {
        Record& r = recs[i];
        r.events = (uint8_t)events;
        if (!f.st.running) {
            f.st.frame = k.seq;
            f.st.running = 1;
            output(i, events);
            return kStopNone;
        }
        const int32_t d = diff16(k.seq, f.st.frame);
        if (d < 1) {
            if (k.resend) { r.disposition = kDuplicate; return kStopNone; }
            reset();
            r.disposition = kDroppedByReset;
            return kStopRestarted;
        }
        if (d == 1) {
            f.st.frame++;
            output(i, events);
            uint32_t m = 0;
            while (m < count && seq_of(slots[m]) == (uint32_t)(uint16_t)(f.st.frame + 1u)) {
                f.st.frame++;
                output(index_of(slots[m]), 0);
                m++;
            }
            for (uint32_t j = m; j < count; j++) slots[j - m] = slots[j];
            count -= m;
            return kStopNone;
        }
        uint32_t p = 0;
        while (p < count && diff16(k.seq, seq_of(slots[p])) > 0) p++;
        if (p < count && seq_of(slots[p]) == (uint32_t)k.seq) { r.disposition = kDuplicate; return kStopNone; }
        if (count == max_frames + 1u) {
            reset();
            r.disposition = kDroppedByReset;
            return kStopBufferFull;
        }
        for (uint32_t j = count; j > p; j--) slots[j] = slots[j - 1];
        slots[p] = ((uint64_t)i << 16) | k.seq;
        count++;
        r.disposition = kPending;
        return kStopNone;
    }
};

// One stream: `keys` and `recs` are ITS keys and records (parsed).  Writes disposition, events and order of every record, and the
// stream's result.
RAOPRX_HD void sequence(const Stream& s, const Key* keys, Record* recs, uint64_t* slots, StreamResult* out)
{
    Serial q;
    q.f.st = s.state_in;
    q.f.n_output = 0;
    q.count = 0;
    q.max_frames = s.max_frames;
    q.slots = slots;
    q.recs = recs;
    uint32_t stop = kStopNone, i = 0;
    for (; i < s.n_datagrams && stop == kStopNone; i++) {
        const Key k = keys[i];
        uint32_t events;
        const uint32_t d = q.f.front(k, &events);
        recs[i].order = 0;
        recs[i].events = (uint8_t)events;
        recs[i].disposition = (uint8_t)d;
        if (d == kNone) stop = q.take(i, k, events);
    }
    for (; i < s.n_datagrams; i++) { recs[i].disposition = kNotReached; recs[i].events = 0; recs[i].order = 0; }
    for (uint32_t k = 0; k < (uint32_t)kMaxRanges; k++) out->ranges[k].start = out->ranges[k].end = 0;
    uint32_t n_ranges = 0;
    if (q.count) {
        auto w = [&](uint32_t j) { return Serial::seq_of(slots[j]); };
        n_ranges = ranges(q.f.st.frame, q.count, s.max_frames, w, out->ranges);
        for (uint32_t j = 0; j < q.count; j++) recs[Serial::index_of(slots[j])].order = j;      // the replay's order
    }
    out->state_out = q.f.st;
    out->n_output = q.f.n_output;
    out->n_pending = q.count;
    out->stop_reason = stop;
    out->n_ranges = n_ranges;
}

// ---- phase 3.  Datagram j of a stream (its index inside the stream): row j of the stream's rows is the payload of the record whose
// order is j, and a row behind the last output reads zero.
RAOPRX_HD void table_row(const Datagram& g, const Record& r, uint32_t j, uint32_t n_output, PacketRow* rows)
{
    if (r.disposition == kOutput) {
        PacketRow row;
        row.src_offset = g.src_offset + r.payload_offset;
        row.bytes = r.payload_bytes;
        row.reserved = 0;
        rows[r.order] = row;
    }
    if (j >= n_output) { PacketRow zero = {}; rows[j] = zero; }
}

}  // namespace raoprx
