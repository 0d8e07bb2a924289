/* ohgpu_vorbis.h -- the C ABI's Vorbis I decoder (ohgpu_vorbis_*), a part of ohgpu.h kept in a file of its own: ohgpu.h includes it at its
 * end, so `#include "ohgpu.h"` gives the whole ABI.  The types it builds on (ohgpu_ctx, ohgpu_batch, ohgpu_alac_packet) are ohgpu.h's.
 *
 * What stands where the reference's CodecVorbis does (OpenHome/Media/Codec/Vorbis.cpp, which plays through Tremor): the audio packets of a
 * Vorbis I stream in -- the rows of a packet table, as the Ogg layer (ohgpu_ogg_* without OHGPU_OGG_FLAC_MAPPING) delivers them --, 16-bit
 * PCM out.  DESIGN.md 5.23 has the whole; the format text is csrc/vorbis_core.h.
 *
 * V1  The stream's identification and setup headers are parsed once, on the host, into a SETUP IMAGE (ohgpu_vorbis_setup_parse): a
 *     position-independent blob of 32-bit words that a batch uploads as it is.  Floor type 1, residue types 0 / 1 / 2, mapping type 0;
 *     codebook lookup types 0 / 1 / 2.  Floor type 0 is OHGPU_ERR_UNSUPPORTED, and so is a stream beyond the limits below.
 * V2  A packet whose first bit is 1 is a header packet: status HEADER, passed over.  A packet of no bytes, or whose mode number is not one
 *     of the setup's: status CORRUPT, passed over.  Every other packet is OK: the end of the packet inside the floor or the residue is the
 *     specification's nominal case (a floor it ends in is unused -- what Tremor does --, a residue it ends in keeps what it has), and
 *     so is a codeword an under-specified codebook does not hold.
 * V3  The first OK packet of a stream's range primes the overlap and delivers nothing.  Every later OK packet delivers
 *     previous_block / 4 + block / 4 samples a channel (the previous OK packet's block), at the stream's running sum.  A caller continues a
 *     stream by sending the last packet of the previous call again: the batch keeps nothing between runs.
 * V4  Only the first max_samples samples a channel of a stream are written; the packet records count what was written.
 * V5  sample = clamp(floor(x * 32768 + 0.5), -32768, 32767), written as interleaved big-endian 16-bit frames at dst_offset, or with
 *     OHGPU_VORBIS_OUT_PLANAR32 as 32-bit words, channel c at dst_offset + c * dst_plane_stride (what OHGPU_FLAG_SRC_PLANAR32 reads).
 * V6  A setup whose codebooks hold a value vector entry that is not finite is OHGPU_ERR_INVALID, and a sample that is not a number is
 *     stored as 0.  (The packed floats reach 2^256, so a header valid by its syntax can say infinity, and finite but huge entries can
 *     still sum past float32 in the residue, the coupling or the transform: infinities clamp by V5, inf - inf is not a number.  No
 *     float reaches an integer conversion unclamped.) */
#ifndef OHGPU_VORBIS_H
#define OHGPU_VORBIS_H

#include "ohgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OHGPU_VORBIS_OK       0u
#define OHGPU_VORBIS_HEADER   1u                    /* packet status: a header packet among the audio */
#define OHGPU_VORBIS_CORRUPT  2u                    /* packet status: no bytes, or a mode number the setup does not have */
#define OHGPU_VORBIS_OUT_PLANAR32  1u               /* descriptor flag */
/* The limits of V1: the specification's own (256 codebooks, 64 floors / residues / mappings / modes, 65 floor values) and these. */
#define OHGPU_VORBIS_MAX_COUPLING_STEPS  32u
#define OHGPU_VORBIS_MAX_IMAGE_BYTES     (16u << 20)   /* the cap on a setup image */
#define OHGPU_VORBIS_MAX_CLASS_BYTES     (1u << 20)    /* ... and on a packet's residue classification bytes */

typedef struct ohgpu_vorbis_info {          /* 32 bytes: what the identification header says, and the image's size */
    uint32_t channels;                      /* 1 .. 8 */
    uint32_t sample_rate;
    uint32_t blocksize_short, blocksize_long;   /* 64 .. 8192 */
    uint32_t image_bytes;
    uint32_t codebooks, modes;
    uint32_t reserved;
} ohgpu_vorbis_info;

typedef struct ohgpu_vorbis_stream_desc {   /* 64 bytes */
    uint64_t image_offset;                  /* of the stream's setup image in the batch's image blob; a multiple of 4 */
    uint64_t dst_offset;                    /* a multiple of 4 */
    uint64_t dst_plane_stride;              /* planes only, a multiple of 4; else 0 */
    uint64_t max_samples;                   /* a channel; the destination holds that many */
    uint32_t image_bytes;
    uint32_t first_packet, n_packets;       /* the stream's range of the packet table: the ranges follow each other and take the whole table */
    uint32_t flags;                         /* OHGPU_VORBIS_OUT_PLANAR32 */
    uint32_t reserved[4];                   /* zero */
} ohgpu_vorbis_stream_desc;

typedef struct ohgpu_vorbis_packet_result { /* 24 bytes */
    uint8_t  status;                        /* OHGPU_VORBIS_OK, _HEADER, _CORRUPT */
    uint8_t  mode;
    uint16_t blocksize;                     /* 0 unless OK */
    uint32_t samples;                       /* a channel, written */
    uint64_t position;                      /* of its first sample in the stream's output, before max_samples cuts */
    uint64_t reserved;
} ohgpu_vorbis_packet_result;

typedef struct ohgpu_vorbis_stream_result { /* 24 bytes */
    uint32_t packets_ok;                    /* leading packets that are OK */
    uint32_t first_bad_status;              /* of the packet that ends them, 0 when all are */
    uint64_t samples;                       /* a channel, written by the whole range */
    uint64_t reserved;
} ohgpu_vorbis_stream_result;

/* Host only, no device needed.  Reads the identification header packet and the setup header packet and writes the setup image: with
 * image == NULL or image_capacity too small only info is filled (info->image_bytes says how much room it takes) and, for a too small
 * capacity, OHGPU_ERR_BOUNDS is returned.  OHGPU_ERR_INVALID: a malformed header, an over-specified codebook tree, an index out of range, a value that is not finite (V6).
 * OHGPU_ERR_UNSUPPORTED: floor type 0, more than 8 channels, more than OHGPU_VORBIS_MAX_COUPLING_STEPS coupling steps, an image or a
 * classification area beyond the caps above. */
int ohgpu_vorbis_setup_parse(const void* id_packet, size_t id_bytes, const void* setup_packet, size_t setup_bytes,
                             void* image, size_t image_capacity, ohgpu_vorbis_info* info);
/* Host only.  The codewords the specification's section 3.2.1 assigns to a list of lengths (0: an unused entry, whose codeword is left
 * 0), each right-justified in its word, first bit most significant.  OHGPU_ERR_INVALID for an over-specified tree or a length above 32. */
int ohgpu_vorbis_codewords(const uint8_t* lengths, size_t n, uint32_t* codewords);
/* Host only: the validation ohgpu_vorbis_batch_create makes.  OHGPU_ERR_INVALID: a non-zero reserved word, an unknown flag, an image
 * range outside the blob or not an image (every table of the image is walked: each codebook's tree and value vectors inside the image, each
 * tree's children inside the tree, every book, floor, residue and mapping index in range), packet ranges that do not follow each other, misaligned offsets, overlapping planes.
 * OHGPU_ERR_BOUNDS: a packet outside the source arena, max_samples beyond the destination arena.  The empty batch is legal. */
int ohgpu_vorbis_batch_check(const ohgpu_vorbis_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                             const void* images, uint64_t images_bytes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* The batch copies the images.  Created under ohgpu_set_kernel_variant(1) it takes the plain route: the same head and entropy launches
 * and a direct-form transform (ohgpu_batch_paths_info: vorbis_route 2).  Freed with ohgpu_batch_destroy. */
int ohgpu_vorbis_batch_create(ohgpu_ctx* ctx, const ohgpu_vorbis_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                              const void* images, uint64_t images_bytes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* Head (a lane per packet, then a lane per stream sums the blocks into positions), entropy (a lane per packet: floor values, residue,
 * inverse coupling), synthesis (a workgroup per packet and channel: floor curve, spectrum, IMDCT in the LDS, window), store (overlap-add,
 * round, clip): queued on the stream, nothing waits for the host.  A second run allocates nothing on the device. */
int ohgpu_vorbis_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
int ohgpu_vorbis_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_vorbis_stream_result* streams, size_t n,
                               ohgpu_vorbis_packet_result* packets, size_t n_packets);   /* waits for the last run */
/* The last run's phases in milliseconds from device events: head, entropy, synthesis, store. */
int ohgpu_vorbis_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4]);
/* route: ohgpu_batch_paths_info's vorbis_route.  blocks: the workgroups of the synthesis launch (packets x channels). */
int ohgpu_vorbis_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* blocks);
/* For tests: the float32 spectrum (floor curve times residue, blocksize / 2 values) the last run transformed for one packet and channel. */
int ohgpu_vorbis_batch_spectrum(ohgpu_ctx* ctx, const ohgpu_batch* batch, size_t packet, uint32_t channel, float* out, size_t n_values);
/* Host-buffer convenience: one upload, one run, the results home, and of dst_host what each stream wrote. */
int ohgpu_vorbis_process_host(ohgpu_ctx* ctx, const ohgpu_vorbis_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                              const void* images, uint64_t images_bytes, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                              ohgpu_vorbis_stream_result* stream_results, ohgpu_vorbis_packet_result* packet_results);
/* Host only: the head of an Ogg Vorbis stream, as ohgpu_ogg_flac_head is Ogg FLAC's.  Walks the leading pages of `bytes` (any serial, any
 * first page number, every page's checksum run), takes the first three packets -- identification, comment, setup: types 1, 3, 5, each
 * "vorbis" -- parses the first and the third as ohgpu_vorbis_setup_parse does (image, image_capacity and info as there), and answers the
 * serial and where the first audio packet begins: the page's offset, the segment in it, that page's number -- the (src_offset,
 * first_page_segment, expect_seq) of the stream's first ohgpu_ogg_stream_desc.  OHGPU_ERR_INVALID: not Ogg Vorbis, or the bytes end
 * inside the headers; otherwise ohgpu_vorbis_setup_parse's codes. */
int ohgpu_vorbis_head(const void* bytes, size_t n, void* image, size_t image_capacity, ohgpu_vorbis_info* info, uint32_t* serial,
                      uint64_t* audio_page_offset, uint32_t* audio_segment, uint32_t* audio_seq);
/* Ogg Vorbis from host buffers, built as ohgpu_ogg_flac_process_host is: one upload of the Ogg bytes, the demux (ogg_descs without
 * OHGPU_OGG_FLAC_MAPPING) into a middle arena of mid_bytes that lives on the device only, one small read of the Ogg results and packet
 * records, a Vorbis batch whose packet rows are those records -- stream i's rows are its recorded packets in order, at
 * ogg_descs[i].dst_offset + run_pos; vorbis_descs[i].first_packet and n_packets are replaced by that range --, and of dst_host the samples
 * that were written.  The demuxed bytes never visit the host.  A stream fed from its first page has its three header packets passed
 * over (status HEADER); by V3 the first audio packet of the range primes.  packet_results has n_packets rows, indexed as the Ogg packet
 * table is (rows no packet took stay zero).  Any result pointer may be NULL. */
int ohgpu_ogg_vorbis_process_host(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* ogg_descs, const ohgpu_vorbis_stream_desc* vorbis_descs, size_t n, size_t n_packets,
                                  const void* images, uint64_t images_bytes, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes,
                                  void* dst_host, uint64_t dst_bytes, ohgpu_ogg_stream_result* ogg_results, ohgpu_ogg_packet* packets,
                                  ohgpu_vorbis_stream_result* stream_results, ohgpu_vorbis_packet_result* packet_results);

/* ---- chained Ogg Vorbis (an Icecast mount: every track a link with its own serial, headers, channel count, rate and granule positions).
 * One row per link of a stream that ohgpu_ogg_vorbis_links_process_host met, in stream order and then link order. */
#define OHGPU_VORBIS_LINK_CONTINUED  0xffffffffffffffffull   /* page_offset of the link the call began in */
#define OHGPU_VORBIS_LINK_HEAD_OPEN  1                        /* head: the range ends inside the link's three header packets */
typedef struct ohgpu_vorbis_link {          /* 64 bytes */
    uint32_t stream;                        /* the descriptor's index */
    uint32_t serial;                        /* the link's (the continued link's: of the page its first packet began on, else the descriptor's) */
    uint64_t page_offset;                   /* of the link's first page, from the stream's src_offset; OHGPU_VORBIS_LINK_CONTINUED */
    uint32_t first_packet, n_packets;       /* the link's rows in the Ogg packet table, its header packets included */
    int32_t  head;                          /* OHGPU_OK; ohgpu_vorbis_head's error code; OHGPU_VORBIS_LINK_HEAD_OPEN.  Not OK: nothing of the link is decoded */
    uint32_t channels, sample_rate;         /* what the link's identification header says (the continued link's: its image) */
    uint32_t blocksize_short, blocksize_long;
    uint32_t reserved;
    uint64_t dst_offset;                    /* where the link's samples lie */
    uint64_t samples;                       /* a channel, written */
} ohgpu_vorbis_link;
/* Chained Ogg Vorbis from host buffers, shaped as ohgpu_ogg_vorbis_process_host: one upload, the Ogg batch with OHGPU_OGG_FOLLOW_LINKS
 * and the magic "\x01vorbis" (set here on a copy of ogg_descs[i] unless the descriptor has the flag already), the one small read.  Then,
 * on the host, a stream's packet records are cut at OHGPU_OGG_PACKET_LINK; each new link's head is parsed from the source bytes
 * (ohgpu_vorbis_head at the record's page_offset) into an image in the call's own blob; every link becomes one Vorbis descriptor, and ONE
 * Vorbis batch runs over all of them.
 *   vorbis_descs[i] describes the link the call begins in (its image, dst_offset, flags, and max_samples as a further bound on that link);
 *   first_packet, n_packets and dst_plane_stride are replaced.  dst_capacity_bytes[i] bounds the stream's whole region
 *   [dst_offset, + dst_capacity_bytes[i]), which lies inside the destination.
 *   Links lie in link order in the region, without overlap, each at a multiple of 4.  A link is sized before the run as n_packets x
 *   blocksize_long / 2 samples a channel; one that no longer fits gets what is left, in whole frames, as its max_samples, and every later
 *   link 0 -- the rows' samples say so.  With OHGPU_VORBIS_OUT_PLANAR32 a link's plane stride is its bound x 4.
 *   By V3 the first OK packet of each link primes and delivers nothing: nothing overlaps across links, which is the specification's rule.
 *   A link whose range ends inside its headers (fewer than three packets, the stream's status OK, no link behind it) has head
 *   OHGPU_VORBIS_LINK_HEAD_OPEN: the caller sends it again from its page_offset when more bytes are there.  Give a stream a packet_capacity
 *   for all its packets: a link is seen by its record.  A link NONE of whose packets is whole -- its first page has come, or a part of
 *   it, and the identification packet does not end in the range -- has no row at all, by the Ogg layer's rule L4: the stream's
 *   bytes_consumed stops at that page, its serial and links are those in front of it, and the later call finds the link.
 * links has room for links_capacity rows; *n_links is the true count (n rows at least: every stream has its continued link, with no
 * packets when the range begins at a link's first page).  packet_results as ohgpu_ogg_vorbis_process_host's.  Any result pointer may be NULL. */
int ohgpu_ogg_vorbis_links_process_host(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* ogg_descs, const ohgpu_vorbis_stream_desc* vorbis_descs, const uint64_t* dst_capacity_bytes,
                                        size_t n, size_t n_packets, const void* images, uint64_t images_bytes, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes,
                                        void* dst_host, uint64_t dst_bytes, ohgpu_ogg_stream_result* ogg_results, ohgpu_ogg_packet* packets,
                                        ohgpu_vorbis_link* links, size_t links_capacity, size_t* n_links, ohgpu_vorbis_packet_result* packet_results);

#ifdef __cplusplus
}
#endif
#endif /* OHGPU_VORBIS_H */
