/* ohgpu_ts.h -- the C ABI's MPEG transport stream demultiplexer (ohgpu_ts_*) and ADTS frame table (ohgpu_adts_*), a part of ohgpu.h kept
 * in a file of its own: ohgpu.h includes it at its end, so `#include "ohgpu.h"` gives the whole ABI.  The types it builds on (ohgpu_ctx,
 * ohgpu_batch) are ohgpu.h's. */
#ifndef OHGPU_TS_H
#define OHGPU_TS_H

#include "ohgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Layer 1: transport stream -> elementary stream (the text is csrc/ts_packet_core.h) ----
 * What stands where the reference's MpegTsContainer does (OpenHome/Media/Codec/MpegTs.cpp: MpegTs, MpegPes): 188-byte transport packets in,
 * the audio elementary stream as one contiguous run out, with a record per PES packet.  A stream's src_bytes at src_offset (any address)
 * are read as a grid of src_bytes / 188 packets from its first byte; there is no resynchronising search, and the src_bytes % 188 bytes
 * left over are not read (trailing_bytes).  The rules follow the reference wherever a conformant stream cannot tell the difference;
 * where the reference ignores a field ISO 13818-1 defines, they follow the standard (marked +; DESIGN.md 5.22 lists them).
 *
 * T1  A packet is skipped and counted when byte 0 is not 0x47 (bad_sync), when transport_error_indicator is set (+ tei_packets), when
 *     transport_scrambling_control is not 0 (+ scrambled_packets); the first of the three that applies counts.
 * T2  With the adaptation flag (byte 3 & 0x20) byte 4 is the field's length L.  L > 183 ends the stream at that packet for every PID:
 *     status CORRUPT, corrupt_packet its grid index, everything in front of it still delivered, nothing at or behind it looked at (the
 *     three counts of T1 stop there too).  The payload is what follows the header and the field; it may be empty.  + A packet without
 *     the payload bit (byte 3 & 0x10) has no payload.
 * T3  The PAT is the first packet in grid order on PID 0 with payload_unit_start whose section -- behind pointer_field bytes -- lies
 *     wholly inside the packet's payload, has table id 0, passes the header checks (section syntax indicator 1, private bit 0, reserved
 *     bits 11, the two unused length bits 0, section_length <= 1021 and >= 9, reserved bits 11 in front of the version), + whose CRC-32
 *     is right (polynomial 0x04c11db7, start 0xffffffff, nothing reflected or complemented: over the section with its CRC bytes it is 0),
 *     and which has an entry whose program_number is not 0 (+ the first such entry gives pmt_pid; every entry up to it has its three
 *     reserved bits set).  A failing candidate is ignored and the next one tried.  Later PATs are ignored.
 * T4  The PMT is the first packet behind the PAT's on pmt_pid with payload_unit_start that passes the same section checks with table id 2
 *     (section_length >= 13), the CRC, and the reserved and unused bits of the PCR PID, program_info_length and of every elementary
 *     stream entry up to the first of type 0x0f, whose PID is audio_pid.  A valid PMT without such an entry: status NO_AUDIO.
 * T5  Audio packets are the packets on audio_pid behind the PMT's.  A descriptor may give pmt_pid and / or audio_pid (non-zero) for a
 *     stream that continues: with audio_pid every packet of the grid on it is audio and T3 / T4 do not run; with pmt_pid alone the PMT
 *     is the first such packet of the grid.
 * P1  A payload_unit_start audio packet starts a PES packet when its payload has at least 9 bytes, begins 00 00 01, + has a stream id
 *     0xC0..0xDF, byte 6 & 0xC0 is 0x80, 9 + h (h = PES_header_data_length) does not exceed the payload, and PES_packet_length N is 0 or
 *     >= 3 + h.  Otherwise it is a bad start (bad_pes_starts): its payload and that of the audio packets up to the next
 *     payload_unit_start are dropped.
 * P2  A PES packet's elementary bytes are what follows its header through the audio packets up to the next payload_unit_start or the
 *     end: A bytes.  With N != 0 it expects E = N - 3 - h: min(E, A) are delivered, A > E flags the record EXCESS, A < E in front of a
 *     next start TRUNCATED, A < E at the end of the input gives the result's pes_open_bytes = E - A.  With N = 0 all A are delivered
 *     and at the end of the input pes_open_bytes is 0xffffffff.  (pes_open_bytes is 0 when no PES packet is open at the end.)
 * P3  pts: the 33 bits of bytes 9..13 when byte 7 & 0x80 is set and h >= 5, else OHGPU_TS_NO_PTS.
 * P4  With OHGPU_TS_PES_OPEN the audio payload in front of the first start continues an earlier PES packet: at most the descriptor's
 *     pes_open_bytes of it are delivered (0xffffffff: all), described by record 0, flagged CONTINUATION (stream_id 0, no pts), under the
 *     rules of P2 with E = pes_open_bytes.  The record exists when the first audio packet is not a start.  Without the flag that payload
 *     is dropped.
 * P5  + Among the audio packets with the payload bit the continuity counter goes up by one mod 16; a packet that breaks this adds one to
 *     cc_jumps and flags the PES record its payload falls in CC_JUMP.  Nothing is dropped for it.
 * dropped_bytes counts every audio payload byte that is neither delivered nor part of a good PES header.
 *
 * The delivered bytes are concatenated into [dst_offset, dst_offset + bytes_delivered), at any address; not one byte outside that range
 * is written.  A stream's records are [pes_first, pes_first + min(pes_packets, pes_capacity)) of the batch's table; the count goes on
 * past the capacity, as ohgpu_ogg_batch_packets documents.  Every other record of the table is zero after a run, whatever the run before
 * it left there (the ADTS frame table likewise). */
#define OHGPU_TS_PACKET_BYTES  188u
#define OHGPU_TS_NONE          0xffffffffu            /* pat_packet, pmt_packet, corrupt_packet: there is none */
#define OHGPU_TS_NO_PTS        0xffffffffffffffffull
#define OHGPU_TS_OK        0u
#define OHGPU_TS_NO_PAT    1u
#define OHGPU_TS_NO_PMT    2u
#define OHGPU_TS_NO_AUDIO  3u
#define OHGPU_TS_CORRUPT   4u                         /* whatever else holds: pat_packet, pmt_packet and audio_pid say how far the tables got */
#define OHGPU_TS_PES_OPEN  1u                         /* descriptor flag */
#define OHGPU_TS_PES_CONTINUATION  1u                 /* record flags */
#define OHGPU_TS_PES_EXCESS        2u
#define OHGPU_TS_PES_TRUNCATED     4u
#define OHGPU_TS_PES_CC_JUMP       8u

typedef struct ohgpu_ts_stream_desc {     /* 64 bytes */
    uint64_t src_offset;            /* any address */
    uint64_t dst_offset;            /* any address */
    uint64_t dst_capacity;          /* >= (src_bytes / 188) * 184 */
    uint32_t src_bytes;             /* < 2^31 */
    uint32_t flags;                 /* OHGPU_TS_PES_OPEN */
    uint32_t pmt_pid, audio_pid;    /* 0: to be found; else 1..0x1fff, from an earlier result */
    uint32_t pes_open_bytes;        /* with OHGPU_TS_PES_OPEN: an earlier result's */
    uint32_t pes_first, pes_capacity;   /* the stream's range of the batch's PES table */
    uint32_t reserved[3];           /* zero */
} ohgpu_ts_stream_desc;

typedef struct ohgpu_ts_stream_result {   /* 64 bytes */
    uint8_t  status;                /* OHGPU_TS_OK ... _CORRUPT */
    uint8_t  trailing_bytes;        /* src_bytes % 188 */
    uint16_t reserved;
    uint16_t pmt_pid, audio_pid;    /* 0: not found */
    uint32_t packets;               /* src_bytes / 188 */
    uint32_t bad_sync, tei_packets, scrambled_packets;
    uint32_t pat_packet, pmt_packet;    /* grid indices, OHGPU_TS_NONE where none was looked for or found */
    uint32_t audio_packets, pes_packets, bad_pes_starts;
    uint32_t bytes_delivered, dropped_bytes, cc_jumps;
    uint32_t pes_open_bytes;
    uint32_t corrupt_packet;
} ohgpu_ts_stream_result;

typedef struct ohgpu_ts_pes {             /* 32 bytes, one per PES packet */
    uint64_t es_offset;             /* of its first delivered byte, from the run's start */
    uint64_t pts;                   /* 33 bits, or OHGPU_TS_NO_PTS */
    uint32_t bytes;                 /* delivered */
    uint32_t packet;                /* grid index of its first packet */
    uint32_t flags;                 /* OHGPU_TS_PES_* */
    uint8_t  stream_id;
    uint8_t  reserved[3];
} ohgpu_ts_pes;

/* Host only, no device needed: the validation ohgpu_ts_batch_create makes.  OHGPU_ERR_INVALID: a non-zero reserved word, an unknown flag,
 * src_bytes of 2^31 or more, a PID above 0x1fff, a PES range outside the table, overlapping PES ranges.  OHGPU_ERR_BOUNDS: a range
 * outside its arena, dst_capacity below (src_bytes / 188) * 184.  The empty batch is legal. */
int ohgpu_ts_batch_check(const ohgpu_ts_stream_desc* descs, size_t n, size_t n_pes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* Created under ohgpu_set_kernel_variant(1) the batch takes the plain route: one launch, a lane per stream runs the serial text
 * (ohgpu_ts_batch_paths).  Both routes write the same bytes.  Freed with ohgpu_batch_destroy. */
int ohgpu_ts_batch_create(ohgpu_ctx* ctx, const ohgpu_ts_stream_desc* descs, size_t n, size_t n_pes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes,
                          ohgpu_batch** batch);
/* Parse (a lane per grid packet), tables and sums (a workgroup per stream), gather (a lane per 16-byte piece of the destination;
 * persistent): queued on the stream, nothing waits for the host.  The source arena must reach to the end of the aligned 4-byte word
 * that holds a stream's last packet byte (ohgpu.h: the container layers' requirement).  The batch owns its lists: it runs on one stream
 * at a time.  A second run allocates nothing on the device. */
int ohgpu_ts_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
int ohgpu_ts_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ts_stream_result* results, size_t n);   /* waits for the last run */
int ohgpu_ts_batch_pes(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ts_pes* pes, size_t n_pes);                 /* the whole table, n_pes records */
/* The last run's phases in milliseconds from device events: parse, tables and sums, gather (the plain route: 0, 0, everything). */
int ohgpu_ts_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[3]);
/* route: 1 the three launches, 2 the plain route.  tiles: the gather's work list (64 destination pieces each).  wave_blocks: the
 * workgroups of the persistent gather launch (a wave a tile, four waves a workgroup, at most eight workgroups a CU). */
int ohgpu_ts_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks);
/* Host-buffer convenience: one upload, one run, the results and the table home, and of dst_host only what was delivered. */
int ohgpu_ts_process_host(ohgpu_ctx* ctx, const ohgpu_ts_stream_desc* descs, size_t n, size_t n_pes, const void* src_host, uint64_t src_bytes,
                          void* dst_host, uint64_t dst_bytes, ohgpu_ts_stream_result* results, ohgpu_ts_pes* pes);
/* The section CRC-32 of any bytes (host only): 0x04c11db7, start 0xffffffff, nothing reflected or complemented. */
uint32_t ohgpu_ts_crc(const void* bytes, size_t n);

/* ---- Layer 2: elementary stream -> ADTS frame table (the framing half of CodecAacFdkAdts, AacFdkAdts.cpp) ----
 * Reads src_bytes at src_offset of an arena -- layer 1's run where it lies, or any .aac bytes -- moves no payload byte and writes one
 * record per frame.
 * A1  A header at p needs 7 bytes present and is valid when it begins 0xFFF, its layer bits are 0, its frequency index is <= 12, its
 *     frame length is >= its header bytes (7, or 9 when the protection bit is 0) and its number_of_raw_data_blocks_in_frame is 0.
 * A2  The chain: at p with a valid header and the whole frame present, record it and go to p + length; with a valid header whose frame
 *     runs past the bytes, stop; with no valid header go to p + 1 (skipped_bytes) and flag the next recorded frame INTERRUPTED
 *     (interruptions counts those frames); with fewer than 7 bytes left, stop.  bytes_consumed is the p at which it stopped: the caller
 *     keeps the rest for the next run.
 * A3  With OHGPU_ADTS_RECOGNISE the chain starts at the smallest p in [0, 1001] from which five headers in a row are valid, each at the
 *     previous one's p + length, each with 10 bytes present.  If there is none: status NOT_ADTS, no frames, bytes_consumed 0.  Else
 *     first_frame_offset is that p, profile / sf_index / channel_config are its header's and mean_payload_bytes is the five frames'
 *     payload bytes (length - header bytes) / 5.  Without the flag first_frame_offset and the three fields are the first recorded
 *     frame's (0 where there is none) and mean_payload_bytes is 0. */
#define OHGPU_ADTS_OK         0u
#define OHGPU_ADTS_NOT_ADTS   1u
#define OHGPU_ADTS_RECOGNISE  1u                      /* descriptor flag */
#define OHGPU_ADTS_INTERRUPTED  1u                    /* frame flag */
#define OHGPU_ADTS_RECOGNISE_LAST_START  1001u
#define OHGPU_ADTS_RECOGNISE_FRAMES      5u

typedef struct ohgpu_adts_stream_desc {   /* 32 bytes */
    uint64_t src_offset;            /* any address */
    uint32_t src_bytes;             /* < 2^31 */
    uint32_t flags;                 /* OHGPU_ADTS_RECOGNISE */
    uint32_t frame_first, frame_capacity;   /* the stream's range of the batch's frame table */
    uint32_t reserved[2];           /* zero */
} ohgpu_adts_stream_desc;

typedef struct ohgpu_adts_stream_result { /* 64 bytes */
    uint32_t status;                /* OHGPU_ADTS_OK, _NOT_ADTS */
    uint32_t frames;                /* goes on past frame_capacity */
    uint32_t bytes_consumed;
    uint32_t first_frame_offset;
    uint32_t interruptions, skipped_bytes;
    uint32_t mean_payload_bytes;
    uint8_t  profile, sf_index, channel_config, reserved;
    uint32_t reserved2[8];
} ohgpu_adts_stream_result;

typedef struct ohgpu_adts_frame {         /* 32 bytes */
    uint64_t offset;                /* of its header, from src_offset */
    uint32_t bytes;                 /* header and payload */
    uint32_t flags;                 /* OHGPU_ADTS_INTERRUPTED */
    uint8_t  header_bytes;          /* 7 or 9 */
    uint8_t  profile, sf_index, channel_config;
    uint32_t reserved[3];
} ohgpu_adts_frame;

/* As ohgpu_ts_batch_check, for the frame table's ranges and the source arena. */
int ohgpu_adts_batch_check(const ohgpu_adts_stream_desc* descs, size_t n, size_t n_frames, uint64_t src_arena_bytes);
/* Under ohgpu_set_kernel_variant(1): the plain route, a lane per stream runs the serial text (ohgpu_adts_batch_paths: route 2). */
int ohgpu_adts_batch_create(ohgpu_ctx* ctx, const ohgpu_adts_stream_desc* descs, size_t n, size_t n_frames, uint64_t src_arena_bytes, ohgpu_batch** batch);
/* Map (a lane per byte position decides A1 into a bit), chain (a wave per stream: 64 lanes look at 2048 positions of the map for the
 * next valid header while it searches; recognition takes 64 start positions a step).  The source arena as for ohgpu_ts_batch_run. */
int ohgpu_adts_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* stream);
int ohgpu_adts_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_adts_stream_result* results, size_t n);
int ohgpu_adts_batch_frames(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_adts_frame* frames, size_t n_frames);
int ohgpu_adts_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[2]);   /* map, chain (the plain route: 0, everything) */
int ohgpu_adts_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles);   /* tiles: the map's workgroups, 1024 positions each */
int ohgpu_adts_process_host(ohgpu_ctx* ctx, const ohgpu_adts_stream_desc* descs, size_t n, size_t n_frames, const void* src_host, uint64_t src_bytes,
                            ohgpu_adts_stream_result* results, ohgpu_adts_frame* frames);
/* Host only.  One header by A1: OHGPU_OK and the record (offset 0, flags 0) or OHGPU_ERR_INVALID. */
int ohgpu_adts_header(const void* bytes, size_t n, ohgpu_adts_frame* out);
/* Host only.  The bytes of the ID3v2 tags at the head of a buffer: "ID3", two version bytes that are not 0xff, flags, four sync-safe size
 * bytes below 0x80, plus 10, plus 10 more with the footer flag (0x10); consecutive tags are summed; 0 means no tag. */
uint64_t ohgpu_id3v2_skip(const void* bytes, size_t n);

/* ---- both together: transport bytes in; the elementary run, the PES table and the frame table out.  One upload and both batches on one
 * stream, with one small read of layer 1's results between them.  adts_descs[i].src_offset is ts_descs[i].dst_offset, or lies up to
 * 2^24 - 1 bytes in front of it: dst_host's bytes between the two -- what the last call's chain left unconsumed -- go to the device in
 * front of the run, so that the elementary stream stays one contiguous run from call to call.  Its src_bytes is replaced by those bytes
 * plus the stream's bytes_delivered.  dst_host receives the delivered runs.  Any result pointer may be NULL. */
int ohgpu_ts_adts_process_host(ohgpu_ctx* ctx, const ohgpu_ts_stream_desc* ts_descs, const ohgpu_adts_stream_desc* adts_descs, size_t n, size_t n_pes,
                               size_t n_frames, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                               ohgpu_ts_stream_result* ts_results, ohgpu_ts_pes* pes, ohgpu_adts_stream_result* adts_results, ohgpu_adts_frame* frames);

#ifdef __cplusplus
}
#endif
#endif /* OHGPU_TS_H */
