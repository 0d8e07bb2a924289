/* ohgpu_cbcs.h -- the C ABI's second protected fragmented MPEG-4 family (ohgpu_cbcs_*), a part of ohgpu.h kept in a file of its own:
 * ohgpu.h includes it at its end, so `#include "ohgpu.h"` gives the whole ABI.  The types it builds on (ohgpu_ctx, ohgpu_batch, the
 * fragmented family's result, run, packet and sample rows, the FLAC and Apple Lossless descriptors) are ohgpu.h's and ohgpu_cenc.h's. */
#ifndef OHGPU_CBCS_H
#define OHGPU_CBCS_H

#include "ohgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Protected fragmented MPEG-4, the rest of Common Encryption: scheme `cbcs` (AES-128 in CBC mode under a crypt:skip pattern), tenc
 * version 1 with its constant IV, and subsample entries under both schemes (the text is csrc/cbcs_core.h over
 * csrc/cenc_core.h) ----
 * ohgpu_cbcs_* is ohgpu_cenc_* with wider rules; ohgpu_cenc_* itself keeps answering as it does.  Everything this section does not name
 * follows ohgpu_cenc.h unchanged: the sample entry and its children, the key and NO_KEY, `seig`, the tables, the statuses.  These rules
 * are the specification; ISO/IEC 23001-7 was not at hand.
 *
 * `schm`.  Scheme types `cenc` and `cbcs` are served; `cbc1`, `cens` and anything else: UNSUPPORTED (the `schm`).
 *
 * `tenc`.  1 byte version, 3 flags, 1 reserved, 1 pattern, 1 isProtected, 1 per-sample IV size, 16 KID; shorter than 24 bytes: INVALID.
 * Version 0 or 1, a higher one: UNSUPPORTED.  In version 1 the pattern byte is crypt_blocks << 4 | skip_blocks; in version 0 it is
 * ignored and the pattern is 0:0.  isProtected above 1: INVALID; 0: the track is clear, and iv_size, the pattern and the constant IV
 * read 0.  With isProtected 1, in this order, all at the `tenc`:
 *   - a per-sample IV size of 0 is followed by one byte constant_iv_size and that many bytes: a box too short for them is INVALID, a
 *     constant-IV size other than 8 or 16 UNSUPPORTED;
 *   - `cenc`: a pattern other than 0:0 (that is `cens`), or a per-sample IV size other than 8 or 16: UNSUPPORTED;
 *   - `cbcs`: a per-sample IV size other than 0, 8 or 16: UNSUPPORTED; crypt 0 with skip above 0: UNSUPPORTED.
 *
 * `senc` (a traf's first, judged at the traf's end behind `seig`, skipped on a clear track).  Payload: 1 byte version, 3 flags, u32
 * sample_count, the entries.  Fewer than 8 bytes: INVALID.  A version other than 0, or flag 0x1: UNSUPPORTED.  A sample_count other
 * than the traf's trun samples: INVALID.  An entry is the sample's IV (per-sample IV size bytes, none under a constant IV) and, under
 * flag 0x2, u16 count and count x {u16 clear_bytes, u32 protected_bytes}: the sample's parts in order, clear, protected, clear, ...
 * An entry that leaves the box: INVALID.  A sample with count > 0 whose parts do not sum to its trun size: INVALID, whatever the
 * descriptor's capacities.  All at the `senc`.  count 0 under flag 0x2, and every sample of a
 * senc without the flag: the whole sample is one protected part.  A protected traf that has samples and no `senc` is served when the
 * per-sample IV size is 0 -- every sample one protected part under the constant IV -- and stays UNSUPPORTED (the traf) otherwise.
 * `saiz` / `saio` are skipped and not read.
 *
 * The subsample table.  The entries of the samples a stream serves are kept in its share [subsample_first, + subsample_capacity) of a
 * batch-wide table of n_subsamples rows, in sample order from the stream's first sample on (a gather_first_row inside a traf changes
 * nothing: the chain is followed from the traf's start); a sample without entries takes none.  The first sample whose entries do not fit
 * what is left of the share ends the rows served, exactly as a sample beyond packet_capacity does: with R that sample's index,
 * everything behaves as if packet_capacity were min(packet_capacity, R) -- samples_available, bytes_gathered and the tables show it,
 * `samples` and `runs` still count the whole stream, and the packet and sample rows from R on are not written.  `subsamples` is the
 * count of entries kept.
 *
 * The cipher, `cenc`.  A sample's protected parts, concatenated, are one byte string under one keystream: byte o of that string is
 * xored with byte o % 16 of counter block o / 16 (the counter rule is ohgpu_cenc.h's), so a part may begin in the middle of a
 * keystream block.  Clear parts are copied.  `blocks` counts a keystream block for every piece a protected part is cut into at the
 * keystream's block edges: ceil((o % 16 + B) / 16) for a part of B > 0 bytes at keystream offset o (a block two parts share counts
 * twice; for whole samples this is ohgpu_cenc_*'s count).
 *
 * The cipher, `cbcs`.  Every protected part stands alone.  Of its W = protected_bytes / 16 whole blocks, block b is encrypted if and
 * only if crypt == 0 || skip == 0 || b % (crypt + skip) < crypt.  With the encrypted cipher blocks in order e_0, e_1, ...:
 * clear(e_k) = AES128_Decrypt(key, e_k) ^ (k == 0 ? IV : e_(k-1)) -- the chain links the encrypted blocks across the skipped ones, and
 * starts again from the IV at every part.  The IV is the sample's own or the constant one; one of 8 bytes is the IV's first half, the
 * second half zero.  Skipped blocks, the protected_bytes % 16 tail and clear parts are copied.  `blocks` counts the encrypted blocks.
 *
 * Where this differs from the reference (tests/cbcs_textbook.py carries the same list), beyond ohgpu_cenc.h's list:
 *   - the reference serves scheme `cenc` only (Mpeg4.cpp:2266); here `cbcs` is served too, and tenc version 1;
 *   - the reference reads the subsample flag of a senc (Mpeg4.cpp:2478) and hands the entries to its provider; here they are applied. */
#define OHGPU_CBCS_SCHEME_CENC  0x63656e63u   /* 'cenc' */
#define OHGPU_CBCS_SCHEME_CBCS  0x63626373u   /* 'cbcs' */

typedef struct ohgpu_cbcs_stream_desc {   /* 120 bytes */
    uint64_t src_offset;            /* the first eighteen fields are ohgpu_cenc_stream_desc's, with the same meaning */
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
    uint8_t  kid[16];
    uint8_t  key[16];               /* AES-128; expanded on the host at batch creation, never sent to the device as it is */
    uint32_t subsample_first;       /* the stream's share of the batch's subsample table, as run_first / run_capacity name its runs */
    uint32_t subsample_capacity;
} ohgpu_cbcs_stream_desc;

typedef struct ohgpu_cbcs_stream_result {   /* 232 bytes */
    ohgpu_cenc_stream_result cenc;  /* scheme: 'cenc' or 'cbcs'; iv_size: the per-sample IV's, 0 under a constant IV; blocks: cipher blocks computed */
    uint8_t  crypt_blocks, skip_blocks;     /* tenc's pattern; 0, 0 for version 0 and for a clear track */
    uint8_t  constant_iv_size;      /* 0, 8 or 16 */
    uint8_t  pad;
    uint32_t subsamples;            /* the senc entries kept in the stream's share of the subsample table */
    uint8_t  constant_iv[16];       /* the first constant_iv_size bytes; the rest zero */
} ohgpu_cbcs_stream_result;

/* Host only, no device needed: the validation ohgpu_cbcs_batch_create makes -- ohgpu_cenc_batch_check's, and OHGPU_ERR_INVALID for a
 * share of the subsample table that leaves it or overlaps another stream's. */
int ohgpu_cbcs_batch_check(const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, uint64_t src_arena_bytes,
                           uint64_t dst_arena_bytes);
/* As ohgpu_cenc_batch_create.  The scheme is the stream's to say, so both schedules are expanded here, on the host (the cipher's and
 * the inverse cipher's, 88 words a stream); the device gets them and the descriptors without their keys, and ohgpu_batch_destroy
 * overwrites the schedules' block with zeros.  Created under ohgpu_set_kernel_variant(1) the batch takes the plain route: one launch, a
 * lane a stream, the ciphers included.  Both routes write the same bytes. */
int ohgpu_cbcs_batch_create(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* Walk (with the subsample chain), run sums, carries, expand, finish, decrypt-gather: queued on the stream, nothing waits for the host.
 * A second run, and a second batch of the same shape, allocate nothing on the device. */
int ohgpu_cbcs_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's results and tables, as ohgpu_cenc_batch_*'s. */
int ohgpu_cbcs_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_cbcs_stream_result* results, size_t n);
int ohgpu_cbcs_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs);
int ohgpu_cbcs_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets);
int ohgpu_cbcs_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets);
/* The last run's phases in milliseconds: walk, run sums, carries, expand, finish, decrypt-gather.  The plain route is one phase. */
int ohgpu_cbcs_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6]);
/* The route (OHGPU_MP4F_ROUTE_*), the expansion's tiles and the workgroups of the persistent decrypt-gather launch (0 on the plain route,
 * and for a batch with no room to gather into); the last two may be NULL.  The launch's chunk slots are laid out at create: a stream has
 * room for dst_capacity / 16 + packet_capacity + 3 subsample_capacity work units (none if dst_capacity or packet_capacity is 0), 64 a slot. */
int ohgpu_cbcs_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks);
/* Host only, no device and no key needed: the walk up to the end of `moov`, with both codecs asked for.  It never answers NO_KEY. */
int ohgpu_cbcs_head(const void* bytes, size_t n, ohgpu_cbcs_stream_result* result);
/* Host-buffer convenience, as ohgpu_cenc_process_host: of dst_host the clear bytes that were gathered come back. */
int ohgpu_cbcs_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, const void* src_host,
                            uint64_t src_bytes, void* dst_host, uint64_t dst_bytes, ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets,
                            ohgpu_mp4_sample* samples);
/* Protected fLaC from host buffers to PCM, as ohgpu_cenc_flac_process_host: the clear runs lie in a middle arena of mid_bytes that
 * lives on the device only (flac_descs[i].src_offset must be descs[i].dst_offset). */
int ohgpu_cbcs_flac_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 size_t n_subsamples, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames);
/* Protected alac from host buffers to PCM, as ohgpu_cenc_alac_process_host. */
int ohgpu_cbcs_alac_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 size_t n_subsamples, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results);

#ifdef __cplusplus
}
#endif
#endif /* OHGPU_CBCS_H */
