/* ohgpu_raop_rx.h -- the C ABI's RAOP receiver (ohgpu_raop_rx_*), a part of ohgpu.h kept in a file of its own: ohgpu.h includes it at
 * its end, so `#include "ohgpu.h"` gives the whole ABI.  The types it builds on (ohgpu_ctx, ohgpu_batch, ohgpu_alac_packet) are ohgpu.h's. */
#ifndef OHGPU_RAOP_RX_H
#define OHGPU_RAOP_RX_H

#include "ohgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- RAOP receiver: parse, repair and order the audio datagrams (the text is csrc/raop_rx_core.h) ----
 * What stands in front of ohgpu_raop_*: the datagrams of a session's audio and control ports in, as recvfrom returned them, and per
 * stream the audio packets in playing order out, as the ohgpu_alac_packet rows ohgpu_raop_batch_create takes -- what the reference's
 * RaopAudioServer, RaopControlServer (Av/Raop/ProtocolRaop.cpp:1145-1248, 1414-1466), ProtocolRaop::ProcessPacket (:782-880) and
 * Repairer<MaxFrames> (ProtocolRaop.h:466-789) do before RaopAudioDecryptor sees a packet.  Three launches on one stream, nothing waits
 * for the host: parse (a lane per datagram), sequence (a wave per stream: the waiting frames of a repair live in the wave's lanes), table
 * (a lane per datagram).  No payload byte is read or moved.
 *
 * Per datagram, in this order, the first check that fails naming the status: more than 1472 bytes OVERSIZE (RtpPacketRaop::
 * kMaxPacketBytes); fewer than 4 TRUNCATED; on the audio port fewer than 8 bytes behind those 4 TRUNCATED; on the control port a type
 * (byte 1 & 0x7f) of 0x54 with fewer than 16 bytes behind the 4 TRUNCATED, of 0x56 whose inner datagram (everything behind the 4) has
 * fewer than 4 bytes or fewer than 8 behind them TRUNCATED, any other type OTHER_TYPE.  The RTP version and the audio payload type are
 * deliberately not checked: senders answer resend requests with version 0 and type 0, and the reference has both checks commented out.
 *
 * Per stream the datagrams of BOTH ports are one list in arrival order, and the state below is carried from one to the next:
 *   a sync packet (0x54) sets control_latency = rtp timestamp - (rtp timestamp - latency): SYNC;
 *   an audio packet, or the inner packet of a 0x56, with resume_pending set, seq <= flush_seq and timestamp <= flush_time (plain
 *     unsigned comparisons, as ShouldFlush makes them): FLUSHED, and nothing else happens;
 *   else, when the stream has not started or a resume is pending, ProcessStreamStartOrResume: session_id is taken from the packet if it
 *     is 0, started is set, resume_pending and the flush window are cleared, latency = control_latency if the stream had not started:
 *     OHGPU_RAOP_RX_EVENT_NEW_STREAM on this record, and with it OHGPU_RAOP_RX_EVENT_DELAY if the stream had not started;
 *   an ssrc other than session_id: WRONG_SESSION (the start above has happened all the same, as in the reference);
 *   else the repairer, 16-bit frame arithmetic throughout: the first frame of a stream that is not running is OUTPUT and sets `frame`;
 *     frame + 1 is OUTPUT, and behind it every waiting frame that has become next; a frame at or behind `frame` is a DUPLICATE if it is
 *     a resend and else a restart of the sender (stop, below); a frame further ahead waits (PENDING) in a sorted set of at most
 *     max_frames + 1, unless it waits already (DUPLICATE) or the set is full (stop, below);
 *   every OUTPUT frame is in front of the 441-sample rule of ProtocolRaop::OutputAudio: if control_latency differs from latency by 441
 *     samples or more, latency = control_latency and the record carries OHGPU_RAOP_RX_EVENT_DELAY.
 * Events stand on the datagram whose ARRIVAL caused them, whatever became of it (a frame that drains behind another carries none).
 *
 * Stop.  Where the reference throws RepairerBufferFull or RepairerStreamRestarted it sets iDiscontinuity, closes its servers, drains and
 * resumes with iResumePending.  Here the stream stops at that datagram: it and everything that waited are DROPPED_BY_RESET, every later
 * record is NOT_REACHED (the caller decides what to do with those datagrams), and state_out is what RepairReset and
 * OutputDiscontinuity leave: not running, resume pending, the flush window and the session kept.
 *
 * Waiting frames are not state.  The PENDING datagrams of a batch are queued by the caller, by `order`, in front of the next batch's
 * datagrams, with state_out as state_in: the replay rebuilds iRepairFirst and iRepairFrames exactly (DESIGN.md 5.21 has the proof).
 *
 * The resend ranges are what TimerRepairExpired would ask for at the end of the batch, with its arithmetic: TUint16 operands promoted
 * to int, ResendRange::Set(TUint, TUint), kMaxMissedRanges = max_frames / 2.  Quirks that follow from that text, kept:
 *   - the first range is {frame + 1 (16 bits), first waiting frame - 1}: a first waiting frame of 0 gives end = 0xffffffff, and a gap
 *     that straddles 65535 -> 0 gives end < start (65535 -> 0 for frame 65534 and a first waiting frame of 1); RaopResendRangeRequester
 *     then asks for (end - start) + 1 packets in unsigned arithmetic, whatever that comes to;
 *   - a later gap is asked for only if end - start > 0 as ints, start = the frame below + 1 in 16 bits: a gap whose missing frames
 *     straddle the wrap (65534 waits, then 2: start 65535, end 2) is never asked for;
 *   - the first range is made even when the list is full, so at most max(max_frames / 2, 1) ranges come out.
 * THE ONE DEVIATION: with max_frames 1 the reference's list has no slot and its FIFO asserts; here the first range is made. */
#define OHGPU_RAOP_RX_MAX_PACKET_BYTES 1472u
#define OHGPU_RAOP_RX_MAX_FRAMES       63u   /* the largest max_frames: the waiting set fits a wave (ProtocolRaop::kMaxRepairFrames is 50) */
#define OHGPU_RAOP_RX_MAX_RANGES       31u
#define OHGPU_RAOP_RX_PORT_AUDIO    0u
#define OHGPU_RAOP_RX_PORT_CONTROL  1u
#define OHGPU_RAOP_RX_OK          0u
#define OHGPU_RAOP_RX_TRUNCATED   1u
#define OHGPU_RAOP_RX_OVERSIZE    2u
#define OHGPU_RAOP_RX_OTHER_TYPE  3u   /* a control datagram that is neither 0x54 nor 0x56: `type` says which */
#define OHGPU_RAOP_RX_OUTPUT            1u   /* its payload is row `order` of the stream's rows of the packet table */
#define OHGPU_RAOP_RX_DUPLICATE         2u   /* a frame already waiting, or a resent frame at or behind the last one output */
#define OHGPU_RAOP_RX_PENDING           3u   /* still waiting at the end of the batch: `order` is its place in the replay */
#define OHGPU_RAOP_RX_DROPPED_BY_RESET  4u   /* the datagram the stream stopped at, and every frame that waited then */
#define OHGPU_RAOP_RX_FLUSHED           5u   /* inside the flush window while a resume is pending */
#define OHGPU_RAOP_RX_WRONG_SESSION     6u   /* an ssrc that is not the session's */
#define OHGPU_RAOP_RX_SYNC              7u   /* a sync packet: control_latency is taken from it */
#define OHGPU_RAOP_RX_IGNORED           8u   /* status != OK */
#define OHGPU_RAOP_RX_NOT_REACHED       9u   /* behind the datagram the stream stopped at */
#define OHGPU_RAOP_RX_EVENT_NEW_STREAM  1u   /* ProcessStreamStartOrResume ran in front of this datagram */
#define OHGPU_RAOP_RX_EVENT_DELAY       2u   /* a delay of state `latency` goes out in front of this frame */
#define OHGPU_RAOP_RX_STOP_NONE         0u
#define OHGPU_RAOP_RX_STOP_BUFFER_FULL  1u
#define OHGPU_RAOP_RX_STOP_RESTARTED    2u

typedef struct ohgpu_raop_rx_datagram {   /* 16 bytes */
    uint64_t src_offset;            /* a multiple of 4 */
    uint32_t bytes;                 /* as recvfrom returned */
    uint8_t  port;                  /* OHGPU_RAOP_RX_PORT_AUDIO or _CONTROL: the caller knows the socket */
    uint8_t  reserved[3];           /* zero */
} ohgpu_raop_rx_datagram;

typedef struct ohgpu_raop_rx_state {      /* 32 bytes: what ProtocolRaop, RaopControlServer and the Repairer carry from one datagram to the next */
    uint32_t flush_seq, flush_time; /* ProtocolRaop::iFlushSeq, iFlushTime (SendFlush sets them between batches) */
    uint32_t session_id;            /* iSessionId: 0 until the first packet of a session */
    uint32_t latency;               /* ProtocolRaop::iLatency: what the last delay said */
    uint32_t control_latency;       /* RaopControlServer::iLatency: what the last sync packet said */
    uint16_t frame;                 /* Repairer::iFrame: the last frame output */
    uint8_t  running;               /* Repairer::iRunning */
    uint8_t  started;               /* ProtocolRaop::iStarted */
    uint8_t  resume_pending;        /* iResumePending */
    uint8_t  reserved[7];           /* zero */
} ohgpu_raop_rx_state;

typedef struct ohgpu_raop_rx_stream {     /* 48 bytes */
    uint32_t first_datagram;        /* the streams' ranges tile the datagram table in order */
    uint32_t n_datagrams;
    uint32_t max_frames;            /* 1..63: Repairer<MaxFrames> (ProtocolRaop uses 50, the reference's tests 5) */
    uint32_t reserved;              /* zero */
    ohgpu_raop_rx_state state_in;
} ohgpu_raop_rx_stream;

typedef struct ohgpu_raop_rx_record {     /* 48 bytes, one per datagram */
    uint8_t  status;                /* OHGPU_RAOP_RX_OK ... _OTHER_TYPE */
    uint8_t  disposition;           /* OHGPU_RAOP_RX_OUTPUT ... _NOT_REACHED */
    uint8_t  events;                /* OHGPU_RAOP_RX_EVENT_* */
    uint8_t  resend;                /* 1: the inner packet of a 0x56 datagram */
    uint8_t  marker, extension;     /* of the audio packet (the inner one of a resend), or of the sync packet */
    uint8_t  type;                  /* byte 1 & 0x7f: of the audio packet, the sync packet, or of an OTHER_TYPE datagram */
    uint8_t  port;                  /* the table's */
    uint16_t seq;
    uint16_t payload_offset;        /* 12, or 16 for a resend: where the encrypted payload starts in the datagram */
    uint32_t payload_bytes;
    uint32_t timestamp, ssrc;       /* of an audio packet */
    uint32_t sync[4];               /* of a sync packet: rtp timestamp - latency, ntp seconds, ntp fraction, rtp timestamp */
    uint32_t order;                 /* OUTPUT: its place in the output order; PENDING: its place in the replay; else 0 */
    uint32_t reserved;
} ohgpu_raop_rx_record;

typedef struct ohgpu_raop_rx_range { uint32_t start, end; } ohgpu_raop_rx_range;   /* ResendRange: ask for (end - start) + 1 packets from start */

typedef struct ohgpu_raop_rx_stream_result {   /* 296 bytes */
    ohgpu_raop_rx_state state_out;  /* the state to give the next batch */
    uint32_t n_output;              /* rows [first_datagram, first_datagram + n_output) of the packet table are this stream's, in playing order */
    uint32_t n_pending;
    uint32_t stop_reason;           /* OHGPU_RAOP_RX_STOP_* */
    uint32_t n_ranges;              /* 0 unless frames wait */
    ohgpu_raop_rx_range ranges[OHGPU_RAOP_RX_MAX_RANGES];   /* zero behind n_ranges */
} ohgpu_raop_rx_stream_result;

/* Host only, no device needed: the validation ohgpu_raop_rx_batch_create makes.  OHGPU_ERR_INVALID: a src_offset that is no multiple
 * of 4, a port above 1, a max_frames outside 1..63, a flag of the state above 1, a non-zero reserved byte, stream ranges that do not
 * tile the datagram table in order.  OHGPU_ERR_BOUNDS: a datagram that leaves the source arena. */
int ohgpu_raop_rx_batch_check(const ohgpu_raop_rx_stream* streams, size_t n, const ohgpu_raop_rx_datagram* datagrams, size_t n_datagrams,
                              uint64_t src_arena_bytes);
/* Created under ohgpu_set_kernel_variant(1) the batch takes the plain route: the sequencer is a lane per stream running the serial text
 * (ohgpu_batch_paths_info: raop_rx_route).  Both routes give the same records, rows and results.  Freed with ohgpu_batch_destroy. */
int ohgpu_raop_rx_batch_create(ohgpu_ctx* ctx, const ohgpu_raop_rx_stream* streams, size_t n, const ohgpu_raop_rx_datagram* datagrams, size_t n_datagrams,
                               uint64_t src_arena_bytes, ohgpu_batch** batch);
/* src_base MUST BE 4-BYTE ALIGNED.  Parse, sequence, table: queued on the stream, nothing waits for the host.  The batch owns its
 * records: it runs on one stream at a time.  A second run, and a second batch of the same shape, allocate nothing on the device. */
int ohgpu_raop_rx_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* stream);
/* The last run's results and records (waits for that run); either pair may be NULL / 0. */
int ohgpu_raop_rx_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_raop_rx_stream_result* streams, size_t n,
                                ohgpu_raop_rx_record* records, size_t n_datagrams);
/* The last run's packet table, n_datagrams rows: a stream's rows [first_datagram, first_datagram + n_output) hold its OUTPUT payloads in
 * playing order, src_offset absolute in the source arena (a multiple of 4: the datagram's plus 12 or 16), the rest of its rows zero. */
int ohgpu_raop_rx_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_datagrams);
/* The last run's phases in milliseconds from device events: parse, sequence, table (waits for that run). */
int ohgpu_raop_rx_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[3]);
/* Host-buffer convenience: one upload, one run, results, records and packet rows home.  Any result pointer may be NULL. */
int ohgpu_raop_rx_process_host(ohgpu_ctx* ctx, const ohgpu_raop_rx_stream* streams, size_t n, const ohgpu_raop_rx_datagram* datagrams, size_t n_datagrams,
                               const void* src_host, uint64_t src_bytes, ohgpu_raop_rx_stream_result* stream_results, ohgpu_raop_rx_record* records,
                               ohgpu_alac_packet* packets);
/* Datagrams from host buffers to PCM (or plaintext): the receiver batch runs, its rows and counts come home, and a RAOP batch
 * (ohgpu_raop_batch_create) decrypts and decodes stream i's rows [first_datagram, first_datagram + n_output) -- the table crosses the
 * host between the two, no payload byte does.  descs[i] gives the configuration, key, IV, destination and flags of stream i; its
 * alac.first_packet and alac.n_packets are not read.  packet_results has a row per datagram row: a stream's first n_output are its
 * packets' results, the rest zero.  Any result pointer may be NULL. */
int ohgpu_raop_rx_alac_process_host(ohgpu_ctx* ctx, const ohgpu_raop_rx_stream* streams, const ohgpu_raop_stream_desc* descs, size_t n,
                                    const ohgpu_raop_rx_datagram* datagrams, size_t n_datagrams, const void* src_host, uint64_t src_bytes,
                                    void* dst_host, uint64_t dst_bytes, ohgpu_raop_rx_stream_result* stream_results, ohgpu_raop_rx_record* records,
                                    ohgpu_alac_packet* packets, ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results);

#ifdef __cplusplus
}
#endif
#endif /* OHGPU_RAOP_RX_H */
