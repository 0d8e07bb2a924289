/* ohgpu_cenc.h -- the C ABI's protected fragmented MPEG-4 family (ohgpu_cenc_*), a part of ohgpu.h kept in a file of its own: ohgpu.h
 * includes it at its end, so `#include "ohgpu.h"` gives the whole ABI.  The types it builds on (ohgpu_ctx, ohgpu_batch, the fragmented
 * family's descriptor fields, result, run, packet and sample rows, the FLAC and Apple Lossless descriptors) are ohgpu.h's. */
#ifndef OHGPU_CENC_H
#define OHGPU_CENC_H

#include "ohgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Protected fragmented MPEG-4: Common Encryption (`cenc`, AES-128 in counter mode) in front of the FLAC and Apple Lossless decoders
 * (the text is csrc/cenc_core.h over csrc/mp4_frag_core.h) ----
 * ohgpu_cenc_* reads what ohgpu_mp4f_* reads, plus the protection boxes.  It always gathers: the taken track's samples are written in
 * the clear as one contiguous run, a clear stream's copied, a protected one's decrypted on the way, and the packet rows point at the
 * clear bytes.  Everything this section does not name follows the fragmented section of ohgpu.h unchanged (ohgpu_mp4f_* itself keeps
 * answering an `enca` entry UNSUPPORTED).  These rules are the specification; ISO/IEC 23001-7 was not at hand.
 *
 * The sample entry.  An `enca` entry has the audio entry's 28-byte head; its child boxes are walked in order, counted with the entry
 * against OHGPU_MP4_MAX_BOXES (one more: INVALID, the box), unknown ones skipped, and all of them before anything is judged:
 *   - the first `sinf` holds the first `frma` (4 bytes: the original format -- the entry's codec for `codecs`, NOT_CODEC and the
 *     result's `codec`), the first `schm` (4 bytes version and flags, 4 scheme type, 4 scheme version, an optional URI) and the first
 *     `schi`, which holds the first `tenc`; beside `sinf` stand the codec's own children with the clear entry's rules (`dfLa` for fLaC,
 *     the inner `alac` box for alac);
 *   - no `sinf`, or a `sinf` missing `frma`, `schm` or `schi` > `tenc`: INVALID (the entry); a `frma` of fewer than 4 bytes or a `schm`
 *     of fewer than 12: INVALID (that box); a scheme type other than `cenc` (cbcs, cbc1, cens, anything): UNSUPPORTED (the `schm`);
 *   - `tenc`: 1 byte version, 3 flags, 1 reserved, 1 reserved, 1 isProtected, 1 per-sample IV size, 16 KID.  Shorter than 24 bytes:
 *     INVALID.  A version (the first byte) other than 0: UNSUPPORTED.  isProtected above 1: INVALID; 0: the track is clear and the IV
 *     size is ignored (iv_size reads 0); 1: an IV size of 8 or 16, anything else -- 0, a constant IV, included -- UNSUPPORTED;
 *   - then the codec's own children: what a clear entry of that codec would be refused for is refused here, at the same box.
 * A plain `fLaC` or `alac` entry is a clear track and is served: `entry` is the codec, `scheme` 0.
 *
 * The key.  A protected track (isProtected 1) whose descriptor lacks OHGPU_CENC_HAVE_KEY, or whose `kid` is not `tenc`'s, ends the walk
 * behind `moov` with OHGPU_CENC_NO_KEY: error_offset is the `tenc`, everything `moov` gives is kept (codec, configuration, track,
 * duration, entry, scheme, kid, iv_size), everything a `moof` gives reads 0, and nothing is written.
 *
 * A traf of the taken track.  Its boxes besides tfhd, tfdt and trun are judged at its end, a `seig` grouping first, then the senc:
 *   - an `sbgp` or `sgpd` of 8 payload bytes or more whose grouping type is `seig`: UNSUPPORTED (that box: per-sample keys);
 *   - on a clear track `senc` is skipped;
 *   - the traf's first `senc`, wherever it stands among tfhd, tfdt and the truns, covers the traf's samples in run order; later ones
 *     are skipped.  Payload: 1 byte version, 3 flags, u32 sample_count, then sample_count x IV size bytes.  Fewer than 8 bytes: INVALID.
 *     A version other than 0, flag 0x1 (overridden parameters) or flag 0x2 (subsamples): UNSUPPORTED.  Entries that leave the box, or a
 *     sample_count other than the sum of the traf's trun samples: INVALID (the senc);
 *   - a protected track's traf that has samples and no `senc`: UNSUPPORTED (the traf) -- its IVs may lie in saiz / saio, which are
 *     skipped by size and not read.
 *
 * The keystream.  A sample of S bytes with IV v; counter block j, j = 0 .. ceil(S / 16) - 1: bytes 0..7 are v[0..7], bytes 8..15 the
 * big-endian value (L + j) mod 2^64, L = 0 for an 8-byte IV, else the big-endian value of v[8..15].  The low half wraps without carrying
 * into the high half.  clear[o] = cipher[o] ^ AES128_Encrypt(key, block[o / 16])[o % 16].  Every sample starts again at j = 0, a last
 * partial block uses the keystream's leading bytes, a sample of 0 bytes writes nothing.
 *
 * The tables.  Row i of [gather_first_row, samples_available) of the packet table is {dst_offset + the sizes of the rows from
 * gather_first_row up to i, its size}: offsets into the DESTINATION arena, what the FLAC batch (the whole run) and the Apple Lossless
 * batch (the rows) take.  Every other row the stream has -- and every row when bytes_gathered is 0 -- is {dst_offset, 0}.  The sample
 * rows and the run rows are ohgpu_mp4f_*'s (a run row's data_offset stays a place in the source arena).  No byte outside
 * [dst_offset, dst_offset + bytes_gathered) is touched.
 *
 * Where this differs from the reference (tests/cenc_textbook.py carries the same list):
 *   - the reference reads the version of tenc and senc as (x & 0xF000) >> 24, which is always 0 (Mpeg4.cpp:2346, :2469); here the
 *     version is the payload's first byte;
 *   - the reference protects `mp4a` only; here fLaC and alac are served;
 *   - the reference holds an IV in Mpeg4ProtectionDetails without checking its size; here the IV is 8 or 16 bytes;
 *   - the reference hands the cipher to a provider (IMpegDRMProvider::Decrypt); here the key comes with the descriptor;
 *   - a library's CTR mode increments all 128 bits of the counter block; here only the low eight bytes count, and they wrap. */
#define OHGPU_CENC_NO_KEY    7u      /* statuses 0..6 are OHGPU_MP4F_OK ... OHGPU_MP4F_NOT_FRAGMENTED, with the same meaning */
#define OHGPU_CENC_HAVE_KEY  1u
#define OHGPU_CENC_SCHEME    0x63656e63u   /* 'cenc' */

typedef struct ohgpu_cenc_stream_desc {   /* 112 bytes */
    uint64_t src_offset;            /* the first twelve fields are ohgpu_mp4f_stream_desc's, with the same meaning */
    uint32_t src_bytes;
    uint32_t codecs;
    uint32_t flags;                 /* must be OHGPU_MP4F_GATHER */
    uint32_t packet_first;
    uint32_t packet_capacity;
    uint32_t run_first;
    uint32_t run_capacity;
    uint32_t gather_first_row;
    uint64_t dst_offset;
    uint64_t dst_capacity;
    uint32_t reserved[2];           /* zero */
    uint32_t key_flags;             /* OHGPU_CENC_HAVE_KEY: kid and key are given */
    uint32_t reserved2[3];          /* zero */
    uint8_t  kid[16];               /* the key identifier the key belongs to: tenc's, or the stream answers NO_KEY */
    uint8_t  key[16];               /* AES-128; expanded on the host at batch creation, never sent to the device as it is */
} ohgpu_cenc_stream_desc;

typedef struct ohgpu_cenc_stream_result {   /* 208 bytes */
    ohgpu_mp4f_stream_result mp4f;  /* status: OHGPU_MP4F_OK ... _NOT_FRAGMENTED, OHGPU_CENC_NO_KEY */
    uint32_t entry;                 /* the stsd entry's fourcc as written ('enca', 'fLaC', 'alac') */
    uint32_t scheme;                /* an `enca` entry's scheme type ('cenc'); 0 for a plain entry */
    uint8_t  is_protected, iv_size; /* tenc's; 0, 0 for a clear track */
    uint8_t  pad[2];
    uint32_t reserved;
    uint8_t  kid[16];               /* tenc's: the key to ask for */
    uint64_t blocks;                /* keystream blocks computed: the sum of ceil(size / 16) over the gathered rows of a protected stream */
} ohgpu_cenc_stream_result;

/* Host only, no device needed: the validation ohgpu_cenc_batch_create makes -- ohgpu_mp4f_batch_check's, and OHGPU_ERR_INVALID for
 * flags other than OHGPU_MP4F_GATHER, unknown key_flags or a non-zero reserved word. */
int ohgpu_cenc_batch_check(const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* As ohgpu_mp4f_batch_create.  The keys are expanded here, on the host (44 words a stream); the device gets the schedules and the
 * descriptors without their keys, and ohgpu_batch_destroy overwrites the schedules' block with zeros before it returns to the
 * context's cache.  Created under ohgpu_set_kernel_variant(1) the batch takes the plain route: one launch, a lane a stream, the
 * cipher included.  Both routes write the same bytes. */
int ohgpu_cenc_batch_create(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* Walk, run sums, carries, expand, finish, decrypt-gather: queued on the stream, nothing waits for the host.  The arenas' rules are
 * ohgpu_mp4f_batch_run's.  A second run, and a second batch of the same shape, allocate nothing on the device. */
int ohgpu_cenc_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's results and tables, as ohgpu_mp4f_batch_*'s. */
int ohgpu_cenc_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_cenc_stream_result* results, size_t n);
int ohgpu_cenc_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs);
int ohgpu_cenc_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets);
int ohgpu_cenc_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets);
/* The last run's phases in milliseconds: walk, run sums, carries, expand, finish, decrypt-gather.  The plain route is one phase. */
int ohgpu_cenc_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6]);
/* The route (OHGPU_MP4F_ROUTE_*), the expansion's tiles and the workgroups of the persistent decrypt-gather launch (0 on the plain route,
 * and for a batch with no room to gather into); the last two may be NULL. */
int ohgpu_cenc_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks);
/* Host only, no device and no key needed: the walk up to the end of `moov`, with both codecs asked for.  It never answers NO_KEY: the
 * result's is_protected and kid say which key to ask for. */
int ohgpu_cenc_head(const void* bytes, size_t n, ohgpu_cenc_stream_result* result);
/* Host-buffer convenience, as ohgpu_mp4f_process_host: of dst_host the clear bytes that were gathered come back. */
int ohgpu_cenc_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, const void* src_host, uint64_t src_bytes,
                            void* dst_host, uint64_t dst_bytes, ohgpu_cenc_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples);
/* Protected fLaC from host buffers to PCM, as ohgpu_mp4f_flac_process_host: the clear runs lie in a middle arena of mid_bytes that
 * lives on the device only, and a FLAC batch decodes them (flac_descs[i].src_offset must be cenc_descs[i].dst_offset). */
int ohgpu_cenc_flac_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* cenc_descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cenc_stream_result* cenc_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames);
/* Protected alac from host buffers to PCM: the clear packets lie in the middle arena, which is the Apple Lossless batch's source arena,
 * and its packets are the rows above; stream i's are its rows [gather_first_row, samples_available), none for a stream that is not OK,
 * not alac or gathered nothing.  packet_results has a row a packet row (zero where nothing was decoded). */
int ohgpu_cenc_alac_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* cenc_descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cenc_stream_result* cenc_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results);

#ifdef __cplusplus
}
#endif
#endif /* OHGPU_CENC_H */
