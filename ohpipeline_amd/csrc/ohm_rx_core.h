// ohm_rx_core.h -- the receiving end of Songcast: what stands between a received OHM datagram and the big-endian PCM
// the pipeline's CodecPcm takes.  Three phases, each a function of this file, every one __host__ __device__: csrc/ohm_rx_kernel.hip
// runs this text on the device, tests/cpp/ohm_rx_core_driver.cpp runs the same text on the CPU under the sanitizers.
//
//   parse      a datagram -> a Record.  The wire, all integers big-endian, every field naturally aligned from the datagram's start
//              (which the C ABI keeps at a multiple of 4):
//                0 "Ohm " | 4 major 1 | 5 type | 6 u16 total
//                8 u8 50 | 9 flags | 10 u16 samples | 12 u32 frame | 16 u32 network timestamp | 20 u32 media latency |
//                24 u32 media timestamp | 28 u64 sample start | 36 u64 samples total | 44 u32 sample rate | 48 u32 bit rate |
//                52 i16 volume offset | 54 bit depth | 55 channels | 56 reserved 0 | 57 codec bytes | 58 codec | 58 + codec: audio
//              The order of the checks IS the definition of the statuses: fewer than 8 bytes TRUNCATED; magic, major, a type above 7
//              that is not 255 NOT_OHM; total != the table's bytes TRUNCATED; a type other than 3 NOT_AUDIO; fewer than 58 bytes
//              TRUNCATED; byte 8 != 50, byte 56 != 0, byte 57 > 29 BAD_HEADER; total < 58 + codec TRUNCATED; more than 5760 audio
//              bytes OVERSIZE.  msg_type is filled from NOT_AUDIO on, every other field for OK alone.
//   sequence   a stream's OK records in arrival order -> dispositions, event bits, destination offsets, the state to carry on and the
//              resend request.  The state machine is the reference's frame sequencer read as what it is, a set: frames wait while
//              1 < frame - iFrame, differences in 32-bit two's complement, and every waiting frame but one lies in the 200 frames
//              above iFrame -- a window bitmap of four 64-bit words, bit k for frame iFrame + 1 + k, and beside it a ring of
//              datagram indices addressed by frame mod 256.  The one frame that may wait further out is the frame that BEGAN a repair:
//              beginning a repair has no distance test, so a frame any distance ahead is taken (the `far` slot); every later frame
//              more than 200 ahead resets.  The far frame moves into the window when iFrame comes within 200 of it.
//              The resend request keeps the reference's unsigned loops: a gap is walked `for (i = start; i < end; i++)` on 32-bit
//              unsigned numbers, so a gap whose end lies behind the 2^32 wrap of its start requests nothing.
//   gather     an OUTPUT record's audio -> its place in the stream's run.  Both ends are at any byte address.  A group of lanes
//              takes a record; whole 16-byte destination lines go out as one store each, filled from five aligned source dwords
//              through a byte funnel; what is in front of the first line, behind the last, or too close to the datagram's end for
//              a whole-dword read goes byte by byte.  No load leaves [datagram start, datagram end), no store leaves the record's
//              destination bytes, and no destination byte is read.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define OHMRX_HD __host__ __device__ __forceinline__
#else
#define OHMRX_HD inline
#endif

namespace ohmrx {

enum { kHeaderBytes = 8, kAudioHeaderBytes = 50, kFixedBytes = 58, kMaxCodecBytes = 29, kMaxAudioBytes = 5760 };
enum { kTypeAudio = 3, kTypeResend = 7, kTypeAudioBlob = 255 };
enum { kWindow = 200, kMaxMissed = 20, kRing = 256 };          // kMaxRepairBacklogFrames, kMaxRepairMissedFrames
enum { kFlagHalt = 1, kFlagLossless = 2, kFlagTimestamped = 4, kFlagResent = 8, kFlagTimestamped2 = 16 };
enum Status : uint8_t { kOk = 0, kNotOhm = 1, kNotAudio = 2, kTruncated = 3, kBadHeader = 4, kOversize = 5 };
enum Disposition : uint8_t { kNone = 0, kOutput = 1, kDuplicate = 2, kPending = 3, kDroppedByReset = 4, kStale = 5, kNotReached = 6, kIgnored = 7 };
enum { kEventNewStream = 1, kEventDelay = 2, kEventHalt = 4 };
enum { kStopNone = 0, kStopStale = 1, kStopHalt = 2 };

struct Datagram {             // 16 bytes = ohgpu_ohm_rx_datagram
    uint64_t src_offset;
    uint32_t bytes;
    uint32_t reserved;
};
struct State {                // 32 bytes = ohgpu_ohm_rx_state
    uint64_t last_sample_start;
    uint32_t frame, sample_rate, latency;
    uint8_t  running, stream_msg_due, bit_depth, channels;
    uint32_t reserved[2];
};
struct Stream {               // 64 bytes = ohgpu_ohm_rx_stream
    uint32_t first_datagram, n_datagrams;
    uint64_t dst_offset, dst_capacity;
    State    state_in;
    uint32_t reserved[2];
};
struct Record {               // 104 bytes = ohgpu_ohm_rx_record
    uint8_t  status, disposition, events, flags;
    uint8_t  msg_type, bit_depth, channels, codec_bytes;
    uint16_t samples;
    int16_t  volume_offset;
    uint32_t frame, network_timestamp, media_latency, media_timestamp, sample_rate;
    uint64_t sample_start, samples_total;
    uint32_t bit_rate, audio_offset, audio_bytes, order;
    uint64_t dst_offset;
    uint8_t  codec[32];
};
struct StreamResult {         // 136 bytes = ohgpu_ohm_rx_stream_result
    State    state_out;
    uint64_t out_bytes;
    uint32_t n_output, n_pending, stop_reason, n_resend;
    uint32_t resend[kMaxMissed];
};
static_assert(sizeof(Datagram) == 16 && sizeof(State) == 32 && sizeof(Stream) == 64 && sizeof(Record) == 104 && sizeof(StreamResult) == 136, "Songcast receiver layouts");

// ---- loads.  An aligned dword as it lies in memory (little-endian host and device alike), and big-endian fields out of such dwords.
OHMRX_HD uint32_t ld32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4);
    return v;
}
OHMRX_HD uint32_t be32(const uint8_t* p) { return __builtin_bswap32(ld32(p)); }
OHMRX_HD uint64_t be64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }

// ---- phase 1.  `gram` is the datagram's first byte, at a multiple of 4; bytes [0, bytes) of it are read and no other.
OHMRX_HD void parse(const uint8_t* gram, uint32_t bytes, Record* out)
{
    Record r = {};
    r.disposition = kIgnored;
    r.status = kTruncated;
    do {
        if (bytes < kHeaderBytes) break;
        const uint32_t w1 = be32(gram + 4);                           // major | type | total
        r.status = kNotOhm;
        const uint32_t type = (w1 >> 16) & 0xffu, total = w1 & 0xffffu;
        if (be32(gram) != 0x4f686d20u || (w1 >> 24) != 1u || (type > kTypeResend && type != kTypeAudioBlob)) break;
        r.status = kTruncated;
        if (total != bytes) break;
        r.msg_type = (uint8_t)type;
        r.status = kNotAudio;
        if (type != kTypeAudio) break;
        r.status = kTruncated;
        if (bytes < kFixedBytes) break;
        const uint32_t w2 = be32(gram + 8), w13 = be32(gram + 52);    // 50 | flags | samples;  volume offset | depth | channels
        const uint32_t reserved = gram[56], codec = gram[57];
        r.status = kBadHeader;
        if ((w2 >> 24) != kAudioHeaderBytes || reserved != 0 || codec > kMaxCodecBytes) break;
        r.status = kTruncated;
        if (total < kFixedBytes + codec) break;
        r.status = kOversize;
        if (total - kFixedBytes - codec > kMaxAudioBytes) break;
        r.status = kOk;
        r.flags = (uint8_t)(w2 >> 16);
        r.samples = (uint16_t)w2;
        r.frame = be32(gram + 12);
        r.network_timestamp = be32(gram + 16);
        r.media_latency = be32(gram + 20);
        r.media_timestamp = be32(gram + 24);
        r.sample_start = be64(gram + 28);
        r.samples_total = be64(gram + 36);
        r.sample_rate = be32(gram + 44);
        r.bit_rate = be32(gram + 48);
        r.volume_offset = (int16_t)(uint16_t)(w13 >> 16);
        r.bit_depth = (uint8_t)(w13 >> 8);
        r.channels = (uint8_t)w13;
        r.codec_bytes = (uint8_t)codec;
        r.audio_offset = kFixedBytes + codec;
        r.audio_bytes = total - kFixedBytes - codec;
    } while (false);
    *out = r;
    for (uint32_t k = 0; k < r.codec_bytes; k++) out->codec[k] = gram[kFixedBytes + k];      // (straight into memory: `r` stays in registers)
}

// ---- phase 2.  The window: bit k <-> frame iFrame + 1 + k waits (bit 0 is clear between two datagrams: that frame would have gone out).
// Four named words, the word of a bit chosen by selects: an array indexed by k >> 6 would live in scratch memory on the device.
struct Window {
    uint64_t w0, w1, w2, w3;
    OHMRX_HD bool any() const { return (w0 | w1 | w2 | w3) != 0; }
    OHMRX_HD bool test(uint32_t k) const { const uint64_t w = k < 64u ? w0 : k < 128u ? w1 : k < 192u ? w2 : w3; return (w >> (k & 63u)) & 1u; }
    OHMRX_HD void set(uint32_t k)
    {
        const uint64_t bit = (uint64_t)1 << (k & 63u);
        w0 |= k < 64u ? bit : 0u; w1 |= k >= 64u && k < 128u ? bit : 0u; w2 |= k >= 128u && k < 192u ? bit : 0u; w3 |= k >= 192u ? bit : 0u;
    }
    OHMRX_HD void clear() { w0 = w1 = w2 = w3 = 0; }
    // f(k) for every set bit k, ascending: a word at a time, its bits by count-trailing-zeros
    template <typename F>
    static OHMRX_HD void each_of(uint64_t word, uint32_t base, F& f)
    {
        while (word) { f(base + (uint32_t)__builtin_ctzll(word)); word &= word - 1; }
    }
    template <typename F>
    OHMRX_HD void each(F& f) const { each_of(w0, 0u, f); each_of(w1, 64u, f); each_of(w2, 128u, f); each_of(w3, 192u, f); }
    OHMRX_HD void advance() { w0 = (w0 >> 1) | (w1 << 63); w1 = (w1 >> 1) | (w2 << 63); w2 = (w2 >> 1) | (w3 << 63); w3 >>= 1; }   // iFrame went up by one
};

struct Sequencer {
    State    st;
    Window   win;
    bool     far_valid;       // the frame a repair began on, while it is more than kWindow ahead
    uint32_t far_frame, far_index;
    uint32_t* ring;           // kRing datagram indices (within the stream), by frame mod kRing
    Record*  recs;            // the stream's records
    uint64_t dst_next;
    uint32_t n_output;

    OHMRX_HD bool repairing() const { return far_valid || win.any(); }

    // OutputAudio's decisions for record i (ProtocolOhBase.cpp:461-513); true: a halt frame went out
    OHMRX_HD bool output(uint32_t i)
    {
        Record& r = recs[i];
        uint8_t ev = 0;
        if (r.sample_start < st.last_sample_start || st.bit_depth != r.bit_depth || st.sample_rate != r.sample_rate || st.channels != r.channels) st.stream_msg_due = 1;
        st.last_sample_start = r.sample_start;
        if (st.stream_msg_due) {
            ev |= kEventNewStream;
            st.stream_msg_due = 0;
            st.bit_depth = r.bit_depth;
            st.channels = r.channels;
        }
        if (st.sample_rate != r.sample_rate || st.latency != r.media_latency) {
            st.sample_rate = r.sample_rate;
            st.latency = r.media_latency;
            ev |= kEventDelay;
        }
        if (r.flags & kFlagHalt) ev |= kEventHalt;
        r.disposition = kOutput;
        r.events = ev;
        r.order = n_output++;
        r.dst_offset = dst_next;
        dst_next += r.audio_bytes;
        return (ev & kEventHalt) != 0;
    }
    // iFrame goes up by one: the window moves, and the far frame enters it at its upper edge when it is kWindow ahead
    OHMRX_HD void step()
    {
        st.frame++;
        win.advance();
        if (far_valid && far_frame - st.frame == (uint32_t)kWindow) {
            far_valid = false;
            win.set(kWindow - 1);
            ring[far_frame % kRing] = far_index;
        }
    }
    // every waiting frame gets `d` (in replay order for kPending: the far frame first, then ascending); returns how many
    OHMRX_HD uint32_t mark_waiting(uint8_t d)
    {
        uint32_t n = 0;
        const uint32_t ranked = d == kPending ? 1u : 0u;                    // (`order` is the replay's: a dropped frame has none)
        if (far_valid) { recs[far_index].disposition = d; recs[far_index].order = ranked * n; n++; }
        // (bit 0 too: a halt may end a run of waiting frames half way)
        auto mark = [&](uint32_t k) { Record& r = recs[ring[(st.frame + 1 + k) % kRing]]; r.disposition = d; r.order = ranked * n; n++; };
        win.each(mark);
        return n;
    }
    // RepairReset (ProtocolOhBase.cpp:262-281)
    OHMRX_HD void reset()
    {
        mark_waiting(kDroppedByReset);
        win.clear();
        far_valid = false;
        st.running = 0;
        st.stream_msg_due = 1;
    }
    // Process(OhmMsgAudio&) and Repair (:283-405, :515-553) for record i; the stop reason when the receive loop ends here
    OHMRX_HD uint32_t take(uint32_t i)
    {
        Record& r = recs[i];
        const uint32_t f = r.frame;
        const bool resent = (r.flags & kFlagResent) != 0;
        if (!st.running) {
            st.frame = f;
            st.running = 1;
            return output(i) ? kStopHalt : kStopNone;
        }
        const int32_t diff = (int32_t)(f - st.frame);
        if (!repairing()) {
            if (diff == 1) {
                st.frame++;
                return output(i) ? kStopHalt : kStopNone;
            }
            if (diff < 1) {
                r.disposition = resent ? kDuplicate : kStale;
                return resent ? kStopNone : kStopStale;
            }
            if (diff > kWindow) { far_valid = true; far_frame = f; far_index = i; }     // RepairBegin takes any distance
            else { win.set((uint32_t)diff - 1u); ring[f % kRing] = i; }
            return kStopNone;
        }
        if (diff < 1) {
            if (resent) { r.disposition = kDuplicate; return kStopNone; }
            reset();
            r.disposition = kDroppedByReset;
            return kStopNone;
        }
        if (diff > kWindow) {
            reset();
            r.disposition = kDroppedByReset;
            return kStopNone;
        }
        if (diff == 1) {
            step();
            if (output(i)) return kStopHalt;
            while (win.w0 & 1u) {                                                      // the run of waiting frames that are next
                const uint32_t next = ring[(st.frame + 1) % kRing];
                step();
                if (output(next)) return kStopHalt;
            }
            return kStopNone;
        }
        if (win.test((uint32_t)diff - 1u)) { r.disposition = kDuplicate; return kStopNone; }
        win.set((uint32_t)diff - 1u);
        ring[f % kRing] = i;
        return kStopNone;
    }
    // TimerRepairExpired's list (:407-447) as it would be made now
    OHMRX_HD void missed(StreamResult* out) const
    {
        uint32_t count = 0, start = st.frame + 1;
        auto gap = [&](uint32_t end) {                                // the numbers below a waiting frame that nothing has filled
            for (uint32_t f = start; f < end && count < (uint32_t)kMaxMissed; f++) out->resend[count++] = f;      // (unsigned, as there)
            start = end + 1;
        };
        auto below = [&](uint32_t k) { gap(st.frame + 1 + k); };
        win.each(below);
        if (far_valid) gap(far_frame);
        out->n_resend = count;
    }
};

// One stream: `recs` are ITS records (parsed), `ring` kRing words of scratch.  Writes disposition, events, order and dst_offset of
// every record, and the stream's result.
OHMRX_HD void sequence(const Stream& s, Record* recs, uint32_t* ring, StreamResult* out)
{
    Sequencer q;
    q.st = s.state_in;
    q.win.clear();
    q.far_valid = false;
    q.far_frame = q.far_index = 0;
    q.ring = ring;
    q.recs = recs;
    q.dst_next = s.dst_offset;
    q.n_output = 0;
    // (the result goes straight to memory, field by field: a local StreamResult, its resend list indexed at run time, would live in
    // scratch memory on the device)
    for (uint32_t k = 0; k < (uint32_t)kMaxMissed; k++) out->resend[k] = 0;
    out->n_resend = 0;
    uint32_t stop = kStopNone, n_pending = 0, i = 0;
    for (; i < s.n_datagrams && stop == kStopNone; i++) {
        recs[i].order = 0;
        recs[i].dst_offset = 0;
        recs[i].events = 0;
        if (recs[i].status != kOk) { recs[i].disposition = kIgnored; continue; }
        recs[i].disposition = kPending;
        stop = q.take(i);
    }
    for (; i < s.n_datagrams; i++) { recs[i].disposition = kNotReached; recs[i].order = 0; recs[i].dst_offset = 0; recs[i].events = 0; }
    if (stop != kStopNone) q.reset();                                 // WaitForPipelineToEmpty's RepairReset (:157-160)
    else if (q.repairing()) {
        q.missed(out);
        n_pending = q.mark_waiting(kPending);
    }
    out->state_out = q.st;
    out->out_bytes = q.dst_next - s.dst_offset;
    out->n_output = q.n_output;
    out->n_pending = n_pending;
    out->stop_reason = stop;
}

// ---- phase 3.  Lane `lane` of `lanes` of the group that copies n bytes from src (any address; [src - (src % 4), src + n) must be
// readable, which a payload inside a datagram at a multiple of 4 grants) to dst (any address).
OHMRX_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t shift_bytes)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * shift_bytes));
}
OHMRX_HD void st128(uint8_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t v[4] = {a, b, c, d};
    __builtin_memcpy(__builtin_assume_aligned(p, 16), v, 16);
}
struct GatherCut { uint32_t head, lines, edge; };                     // bytes in front of the first line, whole lines, head + tail bytes
OHMRX_HD GatherCut gather_cut(uintptr_t src, uintptr_t dst, uint32_t n)
{
    GatherCut c;
    c.head = (uint32_t)(-dst & 15u);
    if (c.head > n) c.head = n;
    // line j reads the five dwords from (src + head + 16 j) & ~3 on: all of them must end at or before the last whole dword of the source
    const int64_t room = (int64_t)((src + n) & ~(uintptr_t)3) - (int64_t)src - (int64_t)c.head - 4;
    c.lines = room < 16 ? 0u : (uint32_t)(room >> 4);
    c.edge = n - 16u * c.lines;
    return c;
}
OHMRX_HD void gather_lane(const uint8_t* src, uint8_t* dst, uint32_t n, uint32_t lane, uint32_t lanes)
{
    const GatherCut c = gather_cut((uintptr_t)src, (uintptr_t)dst, n);
    const uint32_t shift = (uint32_t)((uintptr_t)(src + c.head) & 3u);
    const uint8_t* const from = src + c.head - shift;                 // a multiple of 4
    uint8_t* const to = dst + c.head;                                 // a multiple of 16 when there are lines
    // whole trips -- a line for every lane of the group -- run with no lane mask, two at a time so that both trips' loads are
    // issued before either is used; the trip that is left over is the only one under a mask
    const uint32_t whole = c.lines / lanes;
    uint32_t t = 0;
    for (; t + 2u <= whole; t += 2u) {
        const uint32_t ja = t * lanes + lane, jb = ja + lanes;
        const uint8_t* pa = from + 16u * ja;
        const uint8_t* pb = from + 16u * jb;
        const uint32_t a0 = ld32(pa), a1 = ld32(pa + 4), a2 = ld32(pa + 8), a3 = ld32(pa + 12), a4 = ld32(pa + 16);
        const uint32_t b0 = ld32(pb), b1 = ld32(pb + 4), b2 = ld32(pb + 8), b3 = ld32(pb + 12), b4 = ld32(pb + 16);
        st128(to + 16u * ja, funnel(a0, a1, shift), funnel(a1, a2, shift), funnel(a2, a3, shift), funnel(a3, a4, shift));
        st128(to + 16u * jb, funnel(b0, b1, shift), funnel(b1, b2, shift), funnel(b2, b3, shift), funnel(b3, b4, shift));
    }
    for (uint32_t j = t * lanes + lane; j < c.lines; j += lanes) {     // at most one whole trip, then the partial one
        const uint8_t* p = from + 16u * j;
        const uint32_t d0 = ld32(p), d1 = ld32(p + 4), d2 = ld32(p + 8), d3 = ld32(p + 12), d4 = ld32(p + 16);
        st128(to + 16u * j, funnel(d0, d1, shift), funnel(d1, d2, shift), funnel(d2, d3, shift), funnel(d3, d4, shift));
    }
    for (uint32_t e = lane; e < c.edge; e += lanes) {
        const uint32_t at = e < c.head ? e : e + 16u * c.lines;
        dst[at] = src[at];
    }
}

}  // namespace ohmrx
