/*
 * ohgpu.h -- C ABI of the MI355X-native PCM hot path of ohPipeline.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ types, no torch types, never
 * throws.  Every entry point returns OHGPU_OK (0) or a negative OHGPU_ERR_* code; the message
 * for the most recent failure on the calling thread is available from ohgpu_last_error().
 *
 * What it stands in for (file:line relative to the reference tree, openhome/ohPipeline):
 *
 *   reference call chain (per message, on the animator thread)          replaced by
 *   ------------------------------------------------------------------  ---------------------------
 *   MsgFactory::CreateMsgAudioPcm -> DecodedAudio::ConstructPcm          src_endian in the descriptor
 *       (OpenHome/Media/Pipeline/Msg.cpp:3961-3965, 347-408)             (LE->BE fused into the load)
 *   MsgAudioPcm::CreatePlayable (Msg.cpp:2234-2262)                      host fills src_offset/n_frames
 *   MsgPlayable::Read(IPcmProcessor&) (Msg.cpp:2646-2653)                ohgpu_pcm_batch_run()
 *     MsgPlayablePcm::ApplyAttenuation (Msg.cpp:2736-2751)                 attenuation field
 *     RampApplicator::GetNextSample    (Msg.cpp:832-899)                   OHGPU_FLAG_RAMP + ramp_start/end
 *     MsgPlayableSilence::ReadBlock    (Msg.cpp:2874-2893)                 OHGPU_FLAG_SILENCE
 *   IPcmProcessor::ProcessFragment doing depth conversion                dst_bits / dst_endian
 *     FlywheelInput::AppendSubsample8/16/24/32 (StarvationRamper.cpp:117-186)
 *     RampGenerator::ProcessFragment           (StarvationRamper.cpp:281-327)
 *   CodecDsdDsf::Process (Codec/DsdDsf.cpp:169-247, ReverseBits8 :460-465)   OHGPU_DSD_DSF  } ohgpu_dsd_batch_run()
 *   CodecDsdDff::TransferToOutputBuffer (Codec/DsdDff.cpp:305-327, 350-369)  OHGPU_DSD_DFF  }
 *   CodecDsdRaw / DsdFiller (Codec/DsdRaw.cpp:119-134, DsdFiller.cpp:73-99)  OHGPU_DSD_RAW  }
 *   MsgPlayableDsd::ReadBlock (Msg.cpp:2834-2839)                        OHGPU_DSD_PASS
 *   MsgPlayableSilenceDsd::ReadBlock (Msg.cpp:2916-2932), muted DSD       OHGPU_DSD_FLAG_SILENCE
 *       (Msg.cpp:2360-2373)
 *   CodecFlac + libFLAC: frames found, entropy-decoded, restored            ohgpu_flac_batch_run()
 *       (Codec/Flac.cpp:355-443; thirdparty/flac-1.2.1 by its format document)   -> TInt32 planes or CallbackWrite's packed bytes
 *   CodecAlacApple + apple_alac: packets entropy-decoded, predicted, unmixed   ohgpu_alac_batch_run()
 *       (Codec/AlacApple.cpp, AlacAppleBase.cpp:20-115; thirdparty/apple_alac by its behaviour)   -> TInt32 planes or the decoder's packed bytes
 *   RaopAudioDecryptor::Decrypt + CodecRaopApple: AES-128-CBC per packet, then as above   ohgpu_raop_batch_run()
 *       (Av/Raop/ProtocolRaop.cpp:1477-1502, Av/Raop/CodecRaopApple.cpp:61-214)          -> the same, or the plaintext alone
 *   RaopAudioServer, RaopControlServer, ProtocolRaop::ProcessPacket + Repairer<MaxFrames>   ohgpu_raop_rx_batch_run() (ohgpu_raop_rx.h)
 *   MpegTsContainer (MpegTs, MpegPes), the framing of CodecAacFdkAdts, Id3v2   ohgpu_ts_batch_run(), ohgpu_adts_batch_run() (ohgpu_ts.h)
 *   CodecVorbis + Tremor: Vorbis I packets to 16-bit PCM (Codec/Vorbis.cpp; by the specification)   ohgpu_vorbis_batch_run() (ohgpu_vorbis.h)
 *       (Av/Raop/ProtocolRaop.cpp:285-378, 662-926, 1145-1466, ProtocolRaop.h:466-789)       -> the packet table ohgpu_raop_* takes, in playing order
 *   OhmHeader::Internalise + OhmMsgAudio::Create(IReader&) + ProtocolOhBase's frame sequencer   ohgpu_ohm_rx_batch_run()
 *       (Av/Songcast/Ohm.cpp:22-42, OhmMsg.cpp:101-175, ProtocolOhBase.cpp:254-553)            -> CodecPcm's big-endian bytes
 *   CodecFlac's Ogg FLAC streams: libogg's page reader and libFLAC's Ogg aspect in front of the frames   ohgpu_ogg_batch_run()
 *       (Codec/Flac.cpp:155-213; thirdparty/libogg and flac-1.2.1's Ogg aspect by their behaviour)        -> the run ohgpu_flac_* reads
 *   Mpeg4Container in front of CodecAlacApple: boxes walked, sample tables expanded into packet rows   ohgpu_mp4_batch_run()
 *       (Codec/Mpeg4.cpp by its behaviour and ISO/IEC 14496-12; AlacApple.cpp:92-186)                 -> the table ohgpu_alac_* takes
 *   CodecWav, CodecAiff, CodecAifc: the chunks walked, the audio run made big-endian (and 32 -> 24 bit)   ohgpu_iff_batch_run()
 *       (Codec/Wav.cpp, AiffBase.cpp, Aiff.cpp, Aifc.cpp by their behaviour)                             -> CodecPcm's big-endian bytes
 *   "SampleRateConverter" -- NOT PRESENT in the reference  ohgpu_src_* (own spec)
 *
 * The reference binds nothing through FFI today (it is one C++ static library); INTEGRATION.md
 * shows the adapter a maintainer would add: an IPcmProcessor-shaped C++ shim over this ABI.
 *
 * Threading: an ohgpu_ctx may be used from one thread at a time (the reference's element
 * contract is the same: one puller thread per element, Msg.h:1844-1849).  Different contexts
 * are independent.  All *_run calls are asynchronous on the given stream.
 */
#ifndef OHGPU_H
#define OHGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHGPU_ABI_VERSION 1

/* ---- error codes ---- */
#define OHGPU_OK                0
#define OHGPU_ERR_INVALID      (-1)  /* bad argument / descriptor fails validation (reference: ASSERT) */
#define OHGPU_ERR_DEVICE       (-2)  /* HIP runtime error (message holds hipGetErrorString)            */
#define OHGPU_ERR_NO_DEVICE    (-3)  /* no GPU visible; the product path never falls back to the CPU   */
#define OHGPU_ERR_NOMEM        (-4)
#define OHGPU_ERR_BOUNDS       (-5)  /* descriptor addresses bytes outside the declared arenas         */
#define OHGPU_ERR_UNSUPPORTED  (-6)  /* e.g. attenuation on non-16-bit audio (Msg.cpp:2741)            */

/* ---- enums mirroring the reference ---- */
#define OHGPU_ENDIAN_LITTLE 1   /* AudioDataEndian::Little  Msg.h:107-112 */
#define OHGPU_ENDIAN_BIG    2   /* AudioDataEndian::Big */

#define OHGPU_RAMP_MAX 16384u          /* Ramp::kMax  Msg.h:258 */
#define OHGPU_UNITY_ATTENUATION 256u   /* MsgAudioPcm::kUnityAttenuation  Msg.cpp:2219 */
#define OHGPU_MAX_CHANNELS 8u          /* DecodedAudio::kMaxNumChannels   Msg.h:170 (Sender maps 10 -> handled on host) */

/* ---- descriptor flags ---- */
#define OHGPU_FLAG_RAMP       0x01u  /* Ramp::IsEnabled(): apply RampApplicator semantics (16-bit, low bytes zeroed) */
#define OHGPU_FLAG_SILENCE    0x02u  /* MsgPlayableSilence: emit zeros (+ the 6-channel id bytes of Msg.cpp:2877);
                                        src is not read */
#define OHGPU_FLAG_SRC_PLANAR32 0x08u /* resampled messages only: the source is what CodecFlac::CallbackWrite is handed (Codec/Flac.cpp:
                                         379-417) -- one plane of host-endian TInt32 per channel, sample values at src_bits depth,
                                         sign-extended -- instead of the packed bytes that callback makes of it: channel c's plane
                                         starts at src_offset + c * src_plane_stride, a frame is 4 bytes.  a14 -> a1 -> a-R in one pass;
                                         as in that callback, bits above the depth are ignored */
#define OHGPU_FLAG_ZERO_LSB32 0x04u  /* RampGenerator::ProcessFragment "case 32" (StarvationRamper.cpp:311-320):
                                        when dst_bits == 32 write a zero least-significant byte */

/*
 * One MsgPlayable (Msg.cpp:2684-2696, 2722-2734) flattened for the device.  32 bytes.
 * Audio is packed, interleaved; src_offset already includes MsgPlayable::iOffset.
 * Output is packed interleaved at dst_bits, big endian unless dst_endian says otherwise.
 */
typedef struct ohgpu_msg_desc {
    uint64_t src_offset;    /* bytes from src_base to the first frame                               */
    uint64_t dst_offset;    /* bytes from dst_base to the first output frame                        */
    uint32_t n_frames;      /* sample instants ("samples" in the reference, Msg.cpp:826)            */
    uint16_t ramp_start;    /* Ramp::Start()  [0, 16384]                                            */
    uint16_t ramp_end;      /* Ramp::End()                                                          */
    uint16_t attenuation;   /* 256 = unity; other values only with src_bits == 16 (Msg.cpp:2741)    */
    uint8_t  channels;      /* 1..8                                                                 */
    uint8_t  src_bits;      /* 8, 16, 24, 32                                                        */
    uint8_t  src_endian;    /* OHGPU_ENDIAN_*                                                       */
    uint8_t  dst_bits;      /* 8, 16, 24, 32                                                        */
    uint8_t  dst_endian;    /* OHGPU_ENDIAN_*                                                       */
    uint8_t  flags;         /* OHGPU_FLAG_*                                                         */
} ohgpu_msg_desc;

/*
 * One OUTPUT message of a sample-rate-converted stream.  64 bytes.
 * The input buffer holds frames [src_frame0, src_frame0 + src_frames) of the stream starting at
 * src_offset; frames with a negative absolute index are zeros (stream start); every other frame the
 * filter needs, n0(out_frame0) - T + 1 .. n0(out_frame0 + n_frames - 1), must be present.
 * The resampler runs in the S24 domain (sources are left-justified to 24 bits first), so ramping
 * follows RampApplicator's 24-bit case and attenuation must be unity.
 */
typedef struct ohgpu_src_msg_desc {
    uint64_t src_offset;    /* bytes from src_base to input frame src_frame0                        */
    uint64_t src_frame0;    /* absolute index of the first input frame held in the buffer           */
    uint64_t src_frames;    /* number of input frames held                                          */
    uint64_t out_frame0;    /* absolute index of this message's first output frame                  */
    uint64_t dst_offset;    /* bytes from dst_base                                                  */
    uint32_t n_frames;      /* output frames in this message                                        */
    uint16_t ramp_start;
    uint16_t ramp_end;
    uint16_t attenuation;   /* must be 256                                                          */
    uint8_t  channels;
    uint8_t  src_bits;
    uint8_t  src_endian;
    uint8_t  dst_bits;
    uint8_t  dst_endian;
    uint8_t  flags;         /* OHGPU_FLAG_RAMP | OHGPU_FLAG_ZERO_LSB32 | OHGPU_FLAG_SRC_PLANAR32    */
    uint64_t src_plane_stride; /* OHGPU_FLAG_SRC_PLANAR32: bytes between the channels' planes, multiple of 4 (else 0) */
} ohgpu_src_msg_desc;

typedef struct ohgpu_ctx   ohgpu_ctx;     /* one per GPU / per pipeline thread            */
typedef struct ohgpu_batch ohgpu_batch;   /* validated, device-resident descriptor batch  */
typedef struct ohgpu_src   ohgpu_src;     /* a designed polyphase filter on the device    */

/* ---- library / device ---- */
int         ohgpu_abi_version(void);
const char* ohgpu_last_error(void);
int         ohgpu_device_count(void);                       /* >= 0, or OHGPU_ERR_DEVICE */
int         ohgpu_init(int device, ohgpu_ctx** ctx);         /* OHGPU_ERR_NO_DEVICE when there is no GPU */
int         ohgpu_shutdown(ohgpu_ctx* ctx);
int         ohgpu_device_name(ohgpu_ctx* ctx, char* buf, size_t buf_bytes);
/* The device's PCI address, "0000:c1:00.0", lower case: a host that runs one rank per GPU finds the CPUs nearest the device under
 * /sys/bus/pci/devices/<address>/local_cpulist (bench.py pins each rank's planner and feeder threads there). */
int         ohgpu_device_pci_bus_id(ohgpu_ctx* ctx, char* buf, size_t buf_bytes);

/* ---- plumbing: device memory, streams, events (thin wrappers, so hosts need no HIP headers) ---- */
int ohgpu_malloc(ohgpu_ctx* ctx, size_t bytes, void** dptr);
int ohgpu_free(ohgpu_ctx* ctx, void* dptr);
int ohgpu_malloc_host(ohgpu_ctx* ctx, size_t bytes, void** hptr);   /* pinned */
int ohgpu_free_host(ohgpu_ctx* ctx, void* hptr);
int ohgpu_memcpy_h2d(ohgpu_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream);
int ohgpu_memcpy_d2h(ohgpu_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream);
int ohgpu_memset(ohgpu_ctx* ctx, void* dptr, int value, size_t bytes, void* stream);
int ohgpu_stream_create(ohgpu_ctx* ctx, void** stream);
int ohgpu_stream_destroy(ohgpu_ctx* ctx, void* stream);
int ohgpu_stream_sync(ohgpu_ctx* ctx, void* stream);                /* NULL = the context's own stream */
int ohgpu_event_create(ohgpu_ctx* ctx, void** event);
int ohgpu_event_destroy(ohgpu_ctx* ctx, void* event);
int ohgpu_event_record(ohgpu_ctx* ctx, void* event, void* stream);
int ohgpu_stream_wait_event(ohgpu_ctx* ctx, void* stream, void* event);          /* work queued on stream after this waits for event */
int ohgpu_event_elapsed_ms(ohgpu_ctx* ctx, void* start, void* stop, float* ms);  /* synchronises on stop */

/* ---- RampArray.h:7-74: the 512 Q15 multipliers the device uses (generated) ---- */
int ohgpu_ramp_table(uint16_t out[512]);

/* ---- unpack -> attenuate -> ramp -> pack over a batch of playables ---- */
/* Validates every descriptor against the arena sizes (OHGPU_ERR_BOUNDS / _INVALID / _UNSUPPORTED),
 * then keeps a device-resident copy.  descs is host memory and may be freed after the call. */
int ohgpu_pcm_batch_create(ohgpu_ctx* ctx, const ohgpu_msg_desc* descs, size_t n,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* Launches the batch: src_base / dst_base are DEVICE pointers to arenas at least as large as declared. */
int ohgpu_pcm_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
int ohgpu_batch_destroy(ohgpu_ctx* ctx, ohgpu_batch* batch);
/* Totals recorded at creation (for throughput accounting). */
int ohgpu_batch_info(const ohgpu_batch* batch, uint64_t* n_msgs, uint64_t* in_frames, uint64_t* out_frames,
                     uint64_t* src_bytes_touched, uint64_t* dst_bytes_written);
/* Which kernels a PCM batch (ohgpu_pcm_batch_create), a Songcast frame batch (ohgpu_ohm_batch_create) or a batch of the layout-
 * changing processors (ohgpu_fmt_batch_create) was planned onto at its creation -- read-only, for tests and tools that must know
 * that the path they mean to exercise is the one that ran.  A chunk is one wave's unit of work of the line kernel
 * (csrc/pcm_line_kernel.hip); under ohgpu_set_kernel_variant(1) a batch runs the generic kernel message by message whatever its
 * plan says.  A fmt batch takes exactly one of five routes: mono / stereo Songcast packs of >= 16 bits as plain PCM messages
 * (line_planned, group_chunks), Songcast packs of wider streams (fmt_wide_records), a uniform stereo batch on a register-only
 * kernel (fmt_stereo_*), the staged layout kernel (fmt_staged_chunks), or, with every count zero, the generic kernel only.
 * An Apple Lossless batch (ohgpu_alac_batch_create) answers with alac_route alone, and so does a RAOP batch; an MPEG-4 batch
 * (ohgpu_mp4_batch_create) answers with mp4_route alone, a PCM file batch (ohgpu_iff_batch_create) with iff_route alone, a DSD file
 * batch (ohgpu_dsd_file_batch_create) with dsd_file_route alone, a Vorbis batch (ohgpu_vorbis_batch_create) with vorbis_route alone.
 * OHGPU_ERR_INVALID for any other kind of batch. */
typedef struct ohgpu_batch_paths {       /* 64 bytes */
    uint32_t line_planned;          /* 1: the line kernel has a plan for the batch (0: only the generic kernel can run it) */
    uint32_t launches;              /* line-kernel launches per run: one per layout present (8-bit / silence, and each 16/24/32-bit depth pair) */
    uint32_t staged_chunks;         /* staged path: 8-bit audio on either side and silence, <= 512 subsamples each */
    uint32_t group_chunks;          /* register path, plain: runs of a stream's consecutive plain messages, merged and re-cut */
    uint32_t heavy_chunks;          /* register path, ramped or attenuated: one per message */
    uint32_t prefixed_chunks;       /* chunks that write a Songcast header in front of their audio */
    uint32_t ohm_wide_fragments;    /* Songcast: audible fragments of streams of more than two channels (the channel-selecting kernel) */
    uint32_t ohm_staged_fragments;  /* Songcast: silent fragments of such streams (through scratch) */
    uint32_t ohm_headers_fused;     /* Songcast: frame headers written by the audio pass itself */
    uint32_t ohm_headers_separate;  /* Songcast: frame headers the header kernel writes (every header under kernel variant 1) */
    uint32_t fmt_wide_records;      /* fmt: Songcast packs of streams of more than two channels on the channel-selecting kernel, one per descriptor with frames */
    uint32_t fmt_stereo_records;    /* fmt: a uniform stereo batch of UNPACK_PLANAR (16/24/32 bit) or FLAC_PACK on its register-only kernel, one per descriptor with frames */
    uint32_t fmt_stereo_kind;       /* ... which of the two: OHGPU_FMT_UNPACK_PLANAR or OHGPU_FMT_FLAC_PACK (0 when fmt_stereo_records is 0) */
    uint32_t fmt_stereo_bytes;      /* ... and the instantiation: source bytes per subsample 2/3/4 (UNPACK_PLANAR), destination bytes 1/2/3 (FLAC_PACK) */
    uint32_t fmt_staged_chunks;     /* fmt: chunks of the staged layout kernel (csrc/fmt_line_kernel.hip), <= 512 destination subsamples each */
    union {                         /* (the last word: named for what took it, `reserved` for older callers) */
        uint32_t reserved[1];
        uint32_t alac_route;        /* Apple Lossless: 1 the three fused phases over the transposed scratch, 2 the plain route (created under kernel variant 1) */
        uint32_t mp4_route;         /* MPEG-4: 1 the four phases (walk, tile sums, carries, expand), 2 the plain route: one launch, a lane per stream (kernel variant 1) */
        uint32_t iff_route;         /* PCM files: 1 the two launches (walk, convert by 16-byte pieces), 2 the plain route: one launch, a lane per stream (kernel variant 1) */
        uint32_t raop_rx_route;     /* RAOP receiver: 1 the sequencer is a wave per stream, 2 the plain route: a lane per stream runs the serial text (kernel variant 1) */
        uint32_t vorbis_route;      /* Vorbis: 1 the transform through the FFT in the LDS, 2 the plain route: the direct-form transform (kernel variant 1) */
        uint32_t dsd_file_route;    /* DSD files: 1 the two launches (walk, convert by lanes of eight chunks), 2 the plain route: one launch, a lane per stream (kernel variant 1) */
    };
} ohgpu_batch_paths;
int ohgpu_batch_paths_info(const ohgpu_batch* batch, ohgpu_batch_paths* out);

/* Convenience for hosts that hold host buffers (a live pipeline's 5 ms cadence: the driver thread's MsgPlayable::Read of a
 * period, Msg.cpp:2646-2653, for as many playables as the caller brings): H2D, run, D2H, sync.  Of dst_host only the bytes the
 * messages' outputs cover are written (in ONE copy when the outputs tile a span of it, whatever their order).  The device arenas
 * the audio passes through belong to the context and are kept from call to call -- a steady caller allocates nothing per period
 * (ohgpu_device_allocations) -- and src_host / dst_host may be pageable or pinned (ohgpu_malloc_host: no staging copy).
 * The same holds for the three *_process_host calls below. */
int ohgpu_pcm_process_host(ohgpu_ctx* ctx, const ohgpu_msg_desc* descs, size_t n,
                           const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes);

/* ---- the in-tree IPcmProcessor conversions that are not plain interleaved -> interleaved ---- */
#define OHGPU_FMT_UNPACK_PLANAR 1  /* FlywheelInput::DoProcessFragment + AppendSubsample8/16/24/32 (Pipeline/StarvationRamper.cpp:
                                      117-186): packed BE interleaved -> PLANAR 4-byte BE, left-justified, low bytes zero;
                                      channel c's plane starts at dst_offset + c * dst_plane_stride */
#define OHGPU_FMT_SENDER_PACK   2  /* Sender::DoProcessFragment (Av/Songcast/Sender.cpp:351-377): first two channels (from
                                      channel 8 when there are >= 10), min(bytes, 3) most significant bytes each */
#define OHGPU_FMT_FLAC_PACK     3  /* CodecFlac::CallbackWrite (Codec/Flac.cpp:379-417): planar host-endian TInt32 (channel c at
                                      src_offset + c * src_plane_stride) -> packed BE interleaved 8/16/24 bit */

typedef struct ohgpu_fmt_desc {     /* 48 bytes */
    uint64_t src_offset;
    uint64_t dst_offset;
    uint64_t src_plane_stride;      /* FLAC_PACK only   */
    uint64_t dst_plane_stride;      /* UNPACK_PLANAR only */
    uint32_t n_frames;
    uint8_t  kind;                  /* OHGPU_FMT_* */
    uint8_t  channels;              /* 1..10 (Sender is told about up to 10) */
    uint8_t  src_bits;              /* packed depth of the source (UNPACK/SENDER); 32 for FLAC_PACK's TInt32 planes */
    uint8_t  dst_bits;              /* FLAC_PACK: 8/16/24; ignored otherwise (UNPACK -> 32, SENDER -> min(src,24)) */
    uint8_t  reserved[8];
} ohgpu_fmt_desc;

int ohgpu_fmt_batch_create(ohgpu_ctx* ctx, const ohgpu_fmt_desc* descs, size_t n,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
int ohgpu_fmt_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);

/* ---- DSD: the codec-side packers, the playable pass-through, silence ----
 * The pipeline's DSD format (Pipeline/Msg.cpp:2379-2393) is a run of SAMPLE BLOCKS of W = sample_block_words 32-bit words; a block
 * holds W * 4 / (4 + P) CHUNKS, P = pad_bytes_per_chunk, and a chunk is
 *     [P/2 x 00] L L [P/2 x 00] R R
 * -- sixteen one-bit samples per channel, most significant bit first, the padding in front of each channel's two bytes.  The
 * reference asserts (W * 4) % (4 + P) == 0 and takes W - P for the chunks of a block (Codec/DsdDsf.cpp:108,196, DsdDff.cpp:92,334,
 * Msg.cpp:2385); both hold only for P == 0 (any W >= 1) or W == P + 4 with P even -- in practice (1,0), (2,0), (6,2), (8,4).  Any
 * other pair is OHGPU_ERR_INVALID.
 *
 * A descriptor turns n_chunks chunks' worth of source into ceil(n_chunks / chunks per block) * W * 4 bytes at dst_offset: the
 * chunks, back to back, then 0x69 up to the end of the last block (every byte of that tail, pad positions included: DsdDsf.cpp:
 * 218-237, DsdDff.cpp:350-369).  Chunk j is made of
 *   OHGPU_DSD_DSF   bytes 2r, 2r + 1 of the left plane and of the right plane of pair q (j = 2048 q + r): a file is pairs of
 *                   4096-byte planes, left then right, so they lie at src_offset + 8192 q + 2r and 4096 further on; every byte is
 *                   bit-reversed (the file is LSB first).  Stereo only, as in the reference (DsdDsf.cpp:483).  The source span is
 *                   the whole pairs the chunks touch, ceil(n_chunks / 2048) * 8192 bytes.
 *   OHGPU_DSD_DFF   source bytes 4j .. 4j + 3 = L R L R, written s0 s2 | s1 s3
 *   OHGPU_DSD_RAW   source bytes 4j .. 4j + 3 = L L R R, written s0 s1 | s2 s3 (only the padding is added)
 *   OHGPU_DSD_PASS  the (4 + P) source bytes at src_offset + j * (4 + P), as they are: a playable of audio already in the format
 * With OHGPU_DSD_FLAG_SILENCE (any kind) the source is not read (src_offset is not looked at) and every output byte is 0x69.  RAW, PASS and SILENCE take whole
 * blocks only, as the reference does (Msg.cpp:2922; DsdFiller completes a Raw stream's last input block on the host, so its pad
 * positions stay 00): n_chunks not a multiple of the chunks per block is OHGPU_ERR_INVALID.
 *
 * One deliberate difference: when a DSF or DFF stream ends on a chunk count that is not a whole number of blocks, the reference
 * converts only the whole blocks (numBlocks = remainingChunks / numChunks) yet counts the leftover chunks' bytes, which are then
 * whatever its buffer last held.  Here the leftover chunks ARE converted and the 0x69 fill starts behind them.  Wherever the
 * reference's output is well defined the two agree. */
#define OHGPU_DSD_PASS 1
#define OHGPU_DSD_DSF  2
#define OHGPU_DSD_DFF  3
#define OHGPU_DSD_RAW  4
#define OHGPU_DSD_FLAG_SILENCE 0x01u
#define OHGPU_DSD_SILENCE_BYTE 0x69   /* MsgPlayableSilenceDsd, Msg.cpp:2916-2932 */

typedef struct ohgpu_dsd_desc {     /* 32 bytes */
    uint64_t src_offset;
    uint64_t dst_offset;
    uint32_t n_chunks;
    uint8_t  kind;                  /* OHGPU_DSD_* */
    uint8_t  flags;                 /* OHGPU_DSD_FLAG_SILENCE */
    uint8_t  sample_block_words;    /* W */
    uint8_t  pad_bytes_per_chunk;   /* P */
    uint8_t  reserved[8];           /* zero */
} ohgpu_dsd_desc;

/* Host only, no device needed: validates (kind, W, P, n_chunks) by the rules above and gives the source bytes a descriptor reads
 * from src_offset on (what OHGPU_DSD_FLAG_SILENCE makes 0) and the destination bytes it writes.  Either result may be NULL. */
int ohgpu_dsd_layout(uint32_t kind, uint32_t sample_block_words, uint32_t pad_bytes_per_chunk, uint32_t n_chunks,
                     uint64_t* src_bytes, uint64_t* dst_bytes);
/* Validated like ohgpu_fmt_batch_create (OHGPU_ERR_INVALID / _BOUNDS, nothing kept on a refusal; a descriptor of no chunks is
 * accepted wherever its offsets point); freed with ohgpu_batch_destroy; ohgpu_batch_info counts its descriptors, its chunks (as
 * frames in and out) and its bytes.  The batch holds no per-launch device state: it may be run any number of times, on any stream.
 * Under ohgpu_set_kernel_variant(1) the whole batch runs the plain per-byte kernel dsd_kernel_v1. */
int ohgpu_dsd_batch_create(ohgpu_ctx* ctx, const ohgpu_dsd_desc* descs, size_t n,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
int ohgpu_dsd_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* How the batch was planned (read-only, for tests and tools): descriptors that have a body of whole lanes on the wide path (offsets
 * 16-byte aligned; a packer's P <= 4 and n_chunks >= 8; PASS and silence from 16 bytes on), descriptors with chunks that are left
 * to the byte path altogether, and launches per run (1, or 0 for a batch without chunks).  The wide path also needs both arena
 * pointers 16-byte aligned at the run (ohgpu_malloc's are).  ohgpu_batch_paths_info answers OHGPU_ERR_INVALID for a DSD batch. */
int ohgpu_dsd_batch_paths(const ohgpu_batch* batch, uint32_t* wide_descs, uint32_t* generic_descs, uint32_t* launches);
/* Host-buffer convenience, as ohgpu_pcm_process_host: the context's arenas, nothing allocated in a steady state, dst_host bytes
 * that no descriptor covers preserved, counted in ohgpu_host_transfer_stats. */
int ohgpu_dsd_process_host(ohgpu_ctx* ctx, const ohgpu_dsd_desc* descs, size_t n,
                           const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes);

/* ---- DSD -> PCM: a decimating FIR over the one-bit stream (own specification) ----
 * Input: the pipeline's DSD format above, stereo; chunk j holds bits 16j .. 16j + 15 of each channel, the most significant bit of
 * the first byte first.  Bit n < 0 (before the stream start) is [0,1,1,0,1,0,0,1][n mod 8] with a non-negative modulo: the silence
 * byte 0x69 repeating, aligned at n = 0.  Samples s = 2 * bit - 1.
 * Filter: decimation D in {8, 16, 32, 64}, T taps per output (a multiple of 8 in 8 .. 64), N = D * T coefficients coef[k], int32,
 * Q28, with sum|coef| < 2^30 (every sum then fits 32 bits with the rounding added).
 * Output frame m >= 0, channel c:   acc = sum_{k < N} coef[k] * s_c[(m + 1) * D - 1 - k]
 *                                   y   = clamp(-2^23, 2^23 - 1, (acc + 16) >> 5)            (arithmetic shift)
 * -- unity DC gain is sum(coef) = 2^28 -- written S24 packed, interleaved L R, big-endian unless dst_endian says little; with
 * OHGPU_FLAG_RAMP ramped as RampApplicator's 24-bit case over the message's n_frames, like a resampled message. */
typedef struct ohgpu_dsd_pcm ohgpu_dsd_pcm;   /* a decimating filter on the device */

/* One OUTPUT message.  64 bytes.  The buffer holds chunks [src_chunk0, src_chunk0 + src_chunks) of the stream from src_offset on,
 * (4 + P) bytes each.  Every chunk of index >= 0 that ohgpu_dsd_pcm_window names for the message must be among them
 * (OHGPU_ERR_INVALID otherwise); bits of negative index are the idle pattern and are never read. */
typedef struct ohgpu_dsd_pcm_msg_desc {
    uint64_t src_offset;            /* bytes from src_base to chunk src_chunk0                                    */
    uint64_t src_chunk0;            /* absolute index of the first chunk held                                      */
    uint64_t src_chunks;            /* chunks held                                                                 */
    uint64_t out_frame0;            /* absolute index of the message's first output frame                          */
    uint64_t dst_offset;            /* bytes from dst_base                                                         */
    uint32_t n_frames;              /* output frames (at most 131071 when ramped)                                  */
    uint16_t ramp_start;
    uint16_t ramp_end;
    uint8_t  sample_block_words;    /* W  } validated as for ohgpu_dsd_desc; only P affects addressing             */
    uint8_t  pad_bytes_per_chunk;   /* P  }                                                                        */
    uint8_t  dst_endian;            /* OHGPU_ENDIAN_*                                                              */
    uint8_t  flags;                 /* OHGPU_FLAG_RAMP                                                             */
    uint8_t  reserved[12];          /* zero */
} ohgpu_dsd_pcm_msg_desc;

/* Host only.  Kaiser-windowed sinc by the rule of ohgpu_src_design's integer decimator, over all N = D * T taps: D = dsd_rate /
 * pcm_rate, stop edge pcm_rate - f_pass_hz, cutoff midway, scaled so that sum(coef) ~ gain * 2^28, Q28 rounding half up.
 * OHGPU_ERR_INVALID when dsd_rate / pcm_rate is not exactly 8, 16, 32 or 64, T is not a multiple of 8 in 8 .. 64, the capacity is
 * below N, or sum|coef| >= 2^30.  Pass coef_q28 = NULL to query D only. */
int ohgpu_dsd_pcm_design(uint32_t dsd_rate, uint32_t pcm_rate, uint32_t taps_per_output, double beta, double f_pass_hz, double gain,
                         int32_t* coef_q28, size_t coef_capacity, uint32_t* decimation);
/* The caller's coefficients go to the device (and, for N <= 1024, the byte tables of the fast route made from them).
 * OHGPU_ERR_INVALID for a (D, T) outside the specification or sum|coef| >= 2^30. */
int ohgpu_dsd_pcm_create(ohgpu_ctx* ctx, uint32_t decimation, uint32_t taps_per_output, const int32_t* coef_q28, ohgpu_dsd_pcm** filter);
int ohgpu_dsd_pcm_destroy(ohgpu_ctx* ctx, ohgpu_dsd_pcm* filter);
/* Host only: the chunks [*chunk_lo, *chunk_hi) that output frames [out_frame0, out_frame0 + n_frames) read -- bits
 * (out_frame0 + 1) * D - N .. (out_frame0 + n_frames) * D - 1, those below zero left out.  OHGPU_ERR_INVALID for n_frames == 0,
 * a (D, T) outside the specification or an out_frame0 beyond 2^40. */
int ohgpu_dsd_pcm_window(uint64_t out_frame0, uint32_t n_frames, uint32_t decimation, uint32_t taps_per_output,
                         uint64_t* chunk_lo, uint64_t* chunk_hi);
/* Validated like ohgpu_src_batch_create: OHGPU_ERR_INVALID for a bad (W, P), byte order, flag, reserved byte, ramp endpoint above
 * OHGPU_RAMP_MAX, ramped message above 131071 frames or a window that does not hold every chunk the message reads;
 * OHGPU_ERR_BOUNDS for a window or an output beyond its arena; nothing is kept on a refusal.  A message of no frames is accepted
 * wherever its offsets point.  The batch keeps no per-launch state: it may run any number of times, on any stream.  The filter
 * must outlive the batch.  ohgpu_batch_info counts the messages, the chunks read (as frames in), the frames out and the bytes.
 * Routes: the fast kernel (byte-indexed partial sums in LDS; filters of N <= 1024) unless ohgpu_set_kernel_variant(ctx, 1) is in
 * force at the creation or at the run, or the filter is longer -- then the plain kernel, one thread per output value straight from
 * the specification.  No byte outside the chunks named by ohgpu_dsd_pcm_window is read. */
int ohgpu_dsd_pcm_batch_create(ohgpu_ctx* ctx, const ohgpu_dsd_pcm* filter, const ohgpu_dsd_pcm_msg_desc* descs, size_t n,
                               uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
int ohgpu_dsd_pcm_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* Host only, no device needed: the validation of ohgpu_dsd_pcm_batch_create for a filter of (D, T), with its codes. */
int ohgpu_dsd_pcm_batch_check(uint32_t decimation, uint32_t taps_per_output, const ohgpu_dsd_pcm_msg_desc* descs, size_t n,
                              uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* How the batch was planned (read-only, for tests and tools): messages with frames on the fast route, on the plain route, and
 * launches per run (1, or 0 for a batch without frames). */
int ohgpu_dsd_pcm_batch_paths(const ohgpu_batch* batch, uint32_t* fast_descs, uint32_t* plain_descs, uint32_t* launches);
/* Host-buffer convenience, as ohgpu_src_process_host: src_host need only hold each message's window of chunks. */
int ohgpu_dsd_pcm_process_host(ohgpu_ctx* ctx, const ohgpu_dsd_pcm* filter, const ohgpu_dsd_pcm_msg_desc* descs, size_t n,
                               const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes);

/* ---- FLAC: native frames decoded on the device ----
 * Stands where libFLAC stands under CodecFlac (Codec/Flac.cpp): file bytes in, and out either the planar TInt32 frames
 * CallbackWrite is handed (what OHGPU_FLAG_SRC_PLANAR32 reads) or the packed big-endian bytes that callback makes of them.
 * A descriptor is one stream's byte range; its frames are FOUND (they carry no length): every byte position whose header is legal
 * and whose CRC-8 matches is a candidate, every candidate is parsed to its end (CRC-16), and the chain takes the lowest candidate
 * that parses -- with OHGPU_FLAC_FLAG_AT_FRAME the one at src_offset -- and then, each time, the candidate that starts exactly where
 * the last frame ended, has the descriptor's channels, depth and rate, and carries the next number.  The chain stops with
 * OHGPU_FLAC_OK where the range ends or cuts a frame short (bytes_consumed = where to resume), with OHGPU_FLAC_CORRUPT at bytes that
 * are no such frame (CodecFlac::CallbackError, Flac.cpp:421-425), OHGPU_FLAC_UNSUPPORTED at a frame of 12 or 20 bits, and with
 * OHGPU_FLAC_OVERFLOW at a frame that would land outside [0, max_samples): frames in front of the stop are delivered, nothing
 * behind it is written.  A frame's place is its own first sample number (frame number x blocksize under fixed blocking) minus
 * first_sample.  Bit depths 8, 16, 24; 1..8 channels; every subframe type, both Rice codings, escapes, wasted bits. */
#define OHGPU_FLAC_OK          0u
#define OHGPU_FLAC_CORRUPT     1u
#define OHGPU_FLAC_UNSUPPORTED 2u
#define OHGPU_FLAC_OVERFLOW    3u
#define OHGPU_FLAC_FLAG_AT_FRAME  0x01u  /* the first frame starts at src_offset (a caller resuming at bytes_consumed) */
#define OHGPU_FLAC_OUT_PACKED_BE  0x02u  /* interleaved big-endian at bits / 8 bytes at dst_offset, instead of the planes */

typedef struct ohgpu_flac_streaminfo_t {    /* 48 bytes: the STREAMINFO block */
    uint32_t min_blocksize, max_blocksize;
    uint32_t sample_rate;
    uint8_t  channels, bits, reserved[2];
    uint64_t total_samples;
    uint8_t  md5[16];
    uint32_t min_framesize, max_framesize;
} ohgpu_flac_streaminfo_t;

typedef struct ohgpu_flac_stream_desc {     /* 64 bytes */
    uint64_t src_offset;            /* the stream's bytes: [src_offset, src_offset + src_bytes) of the source arena, any alignment */
    uint64_t src_bytes;             /* < 2^31 */
    uint64_t dst_offset;            /* multiple of 4 */
    uint64_t dst_plane_stride;      /* planes: bytes between the channels' planes, multiple of 4, >= max_samples * 4; packed: 0 */
    uint64_t first_sample;          /* the stream's sample that goes to index 0 of the output */
    uint32_t max_samples;           /* the output holds samples [first_sample, first_sample + max_samples) */
    uint32_t sample_rate;           /* STREAMINFO's */
    uint32_t blocksize;             /* fixed blocking: the stream's block size; 0 = the chain's first frame's */
    uint32_t max_blocksize;         /* STREAMINFO's, 16..65535: a larger frame is no frame */
    uint8_t  channels;              /* 1..8 */
    uint8_t  bits;                  /* 8, 16, 24 */
    uint8_t  flags;                 /* OHGPU_FLAC_FLAG_AT_FRAME | OHGPU_FLAC_OUT_PACKED_BE */
    uint8_t  reserved[5];           /* zero */
} ohgpu_flac_stream_desc;

typedef struct ohgpu_flac_stream_result {   /* 48 bytes */
    uint32_t status;                /* OHGPU_FLAC_* */
    uint32_t frames;                /* frames delivered */
    uint64_t samples;               /* ... and their samples (per channel) */
    uint64_t first_sample_decoded;  /* the first delivered frame's first sample number */
    uint64_t bytes_consumed;        /* from src_offset: what lies behind is for the next call */
    uint32_t candidates;            /* headers with a matching CRC-8 in the range */
    uint32_t candidates_rejected;   /* ... that did not become frames */
    uint64_t reserved;
} ohgpu_flac_stream_result;

typedef struct ohgpu_flac_frame {           /* 24 bytes: one delivered frame */
    uint32_t stream;                /* index of its descriptor */
    uint32_t blocksize;
    uint64_t first_sample;          /* its first sample number in the stream */
    uint32_t src_pos, src_end;      /* its bytes, from the descriptor's src_offset */
} ohgpu_flac_frame;

/* Host only, no device needed: "fLaC", the metadata blocks, STREAMINFO; *audio_offset = where the first frame starts.
 * OHGPU_ERR_INVALID: bad magic, no STREAMINFO in front, or the n bytes end inside the metadata. */
int ohgpu_flac_streaminfo(const void* bytes, size_t n, ohgpu_flac_streaminfo_t* info, uint64_t* audio_offset);
/* Host only, no device needed: the validation ohgpu_flac_batch_create makes, with its codes and ohgpu_last_error() texts. */
int ohgpu_flac_batch_check(const ohgpu_flac_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* Validated on the host (ranges against the arenas: OHGPU_ERR_BOUNDS; alignment, channels, overlapping planes: OHGPU_ERR_INVALID;
 * a depth other than 8/16/24: OHGPU_ERR_UNSUPPORTED); freed with ohgpu_batch_destroy.  The batch owns its results and, from its
 * first run on, its scratch: it runs on one stream at a time. */
int ohgpu_flac_batch_create(ohgpu_ctx* ctx, const ohgpu_flac_stream_desc* descs, size_t n,
                            uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* Scan, probe, chain, restore.  The number of candidates is only known after the scan, so this call SYNCHRONISES with the host
 * between its phases (once, after the scan; the rest is queued on the stream).  Scratch -- the candidates' residuals, bounded by
 * max_blocksize x channels each -- is kept by the batch and its small arrays come from the context's block cache: a second run of
 * the same shape allocates nothing (ohgpu_device_allocations).  Under ohgpu_set_kernel_variant(1) the restore is the plain route:
 * one thread per accepted frame, everything straight from the bytes. */
int ohgpu_flac_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's per-stream results (waits for that run); n = the batch's descriptor count. */
int ohgpu_flac_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_flac_stream_result* results, size_t n);
/* The last run's delivered frames, by stream and then in stream order (waits for that run): up to `capacity` of them are written,
 * *n_frames is how many there are. */
int ohgpu_flac_batch_frames(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_flac_frame* frames, size_t capacity, size_t* n_frames);
/* The last run's phases in milliseconds from device events: scan, probe, chain, restore (waits for that run). */
int ohgpu_flac_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4]);
/* Host-buffer convenience, as ohgpu_dsd_process_host: one upload, one run.  Of dst_host only the samples that were decoded are
 * written.  results (n of them) and frames (as ohgpu_flac_batch_frames) may be NULL. */
int ohgpu_flac_process_host(ohgpu_ctx* ctx, const ohgpu_flac_stream_desc* descs, size_t n,
                            const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                            ohgpu_flac_stream_result* results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames);

/* ---- Apple Lossless packets (the format text is csrc/alac_packet_core.h) ----
 * CodecAlacApple (Codec/AlacApple.cpp, AlacAppleBase.cpp) hands the container's packets to thirdparty/apple_alac one at a time; here a
 * batch of streams, each a run of packets of a packet table, is decoded in one run of three phases -- entropy (a lane per packet),
 * predictor (a lane per channel row), matrix and store (a lane per sample) -- with no host synchronisation inside it.  Packets are
 * independent: packet p of a stream lands at sample p * frame_length of the stream's destination.  Output is host-endian TInt32
 * planes (channel c at dst_offset + c * dst_plane_stride; what OHGPU_FLAG_SRC_PLANAR32 consumes), or the reference decoder's own
 * buffer byte for byte (OHGPU_ALAC_OUT_PACKED_LE: bit_depth / 8 bytes a sample, interleaved, little-endian), or what row a1 makes of
 * that (OHGPU_ALAC_OUT_PACKED_BE).  The product links no Apple code.
 * Where this decoder is stricter than the reference's (tests/alac_textbook.py carries the same list):
 *   - the reference reads up to four bytes past a packet (AlacAppleBase.cpp:29-33); here bits past the packet's end read as zero and
 *     an element that needed one is CORRUPT;
 *   - a compressed element's sample width (bit_depth - 8 * bytes shifted, plus one for a pair) outside 1..32 is CORRUPT;
 *   - a sample count above the stream's frame_length, or audio elements of one packet that disagree about it, is CORRUPT (the
 *     reference overruns its buffers or leaves stale samples);
 *   - bit_depth 20 is UNSUPPORTED (AlacAppleBase.cpp:90 counts two bytes a sample for the decoder's three), so is a kb outside 1..31;
 *   - a rounding shift of zero rounds with nothing and a matrix shift above 31 shifts by 31 (the reference's shifts are undefined
 *     there); an escaped element carries bit_depth bits a sample whatever its shift field says;
 *   - a failed packet writes nothing to the destination.
 * Limits: 1..8 channels, frame_length 1..16384, a packet of at most frame_length * channels * 5 + 64 bytes. */
#define OHGPU_ALAC_OK          0u
#define OHGPU_ALAC_CORRUPT     1u
#define OHGPU_ALAC_UNSUPPORTED 2u
#define OHGPU_ALAC_OUT_PACKED_LE  0x01u
#define OHGPU_ALAC_OUT_PACKED_BE  0x02u
#define OHGPU_ALAC_MAX_FRAME_LENGTH 16384u

typedef struct ohgpu_alac_config {          /* 24 bytes: ALACSpecificConfig, host-endian */
    uint32_t frame_length;
    uint8_t  compatible_version;    /* 0 */
    uint8_t  bit_depth;             /* 16, 24, 32 (20: every packet UNSUPPORTED) */
    uint8_t  pb, mb, kb;
    uint8_t  channels;
    uint16_t max_run;
    uint32_t max_frame_bytes, avg_bit_rate, sample_rate;
} ohgpu_alac_config;

typedef struct ohgpu_alac_packet {          /* 16 bytes: one row of the packet table */
    uint64_t src_offset;            /* the packet's bytes: [src_offset, src_offset + bytes) of the source arena, any alignment */
    uint32_t bytes;
    uint32_t reserved;              /* zero */
} ohgpu_alac_packet;

typedef struct ohgpu_alac_stream_desc {     /* 64 bytes */
    ohgpu_alac_config config;
    uint32_t first_packet, n_packets;  /* its packets: [first_packet, first_packet + n_packets) of the table; the streams' ranges
                                          follow each other in the table without gaps, the first at 0 */
    uint64_t dst_offset;            /* multiple of 4 */
    uint64_t dst_plane_stride;      /* planes: bytes between the channels' planes, multiple of 4, >= n_packets * frame_length * 4; packed: 0 */
    uint32_t flags;                 /* 0, OHGPU_ALAC_OUT_PACKED_LE or OHGPU_ALAC_OUT_PACKED_BE */
    uint32_t reserved[3];           /* zero */
} ohgpu_alac_stream_desc;

typedef struct ohgpu_alac_packet_result { uint32_t status, samples; } ohgpu_alac_packet_result;      /* OHGPU_ALAC_*; samples per channel (0 unless OK) */
typedef struct ohgpu_alac_stream_result {   /* 16 bytes */
    uint32_t packets_ok;            /* the leading packets that decoded */
    uint32_t first_bad_status;      /* the status of the packet behind them (0 when every packet decoded) */
    uint64_t samples;               /* the samples (per channel) of the leading packets */
} ohgpu_alac_stream_result;

/* Host only, no device needed: the 24 big-endian bytes of the configuration, behind an optional 12-byte 'frma' atom and / or 12-byte
 * 'alac' atom header (ALACDecoder.cpp:96-168).  OHGPU_ERR_INVALID: fewer bytes than that, or a compatible version other than 0. */
int ohgpu_alac_config_parse(const void* bytes, size_t n, ohgpu_alac_config* config);
/* Host only, no device needed: the validation ohgpu_alac_batch_create makes, with its codes and ohgpu_last_error() texts. */
int ohgpu_alac_batch_check(const ohgpu_alac_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* Validated on the host (ranges against the arenas: OHGPU_ERR_BOUNDS; the limits above, alignment, overlapping planes, packet ranges:
 * OHGPU_ERR_INVALID; a depth other than 16/20/24/32: OHGPU_ERR_UNSUPPORTED); freed with ohgpu_batch_destroy.  The batch owns its
 * results and its scratch: it runs on one stream at a time.  Created under ohgpu_set_kernel_variant(1) the batch takes the plain
 * route -- one thread per packet does everything, over row-major scratch --, otherwise the three fused phases over the transposed
 * scratch (ohgpu_batch_paths_info: alac_route). */
int ohgpu_alac_batch_create(ohgpu_ctx* ctx, const ohgpu_alac_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                            uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* Entropy, predictor, matrix and store, queued on the stream; nothing waits for the host.  Scratch is kept by the batch and its
 * small arrays come from the context's block cache: a second run, and a second batch of the same shape, allocate nothing
 * (ohgpu_device_allocations). */
int ohgpu_alac_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's results (waits for that run): per stream (n = the batch's descriptor count) and / or per packet (n_packets = the
 * table's length); either pointer may be NULL with its count 0. */
int ohgpu_alac_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_stream_result* streams, size_t n,
                             ohgpu_alac_packet_result* packets, size_t n_packets);
/* The last run's phases in milliseconds from device events: entropy, predictor, matrix and store (waits for that run).  The plain
 * route is one phase: the other two read as 0. */
int ohgpu_alac_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[3]);
/* Host-buffer convenience, as ohgpu_flac_process_host: one upload, one run.  Of dst_host only the samples of packets that decoded
 * are written.  Either result pointer may be NULL. */
int ohgpu_alac_process_host(ohgpu_ctx* ctx, const ohgpu_alac_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                            const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                            ohgpu_alac_stream_result* stream_results, ohgpu_alac_packet_result* packet_results);

/* ---- RAOP (AirPlay) audio: AES-128-CBC decryption in front of the Apple Lossless decoder (the cipher's text is
 * csrc/raop_aes_core.h, written from FIPS-197) ----
 * ProtocolRaop::OutputAudio (Av/Raop/ProtocolRaop.cpp:705-743) passes every audio packet through RaopAudioDecryptor::Decrypt
 * (:1477-1502) before CodecRaopApple sees it: AES-128-CBC under the session key, the IV starting again with EVERY packet, the
 * bytes % 16 tail left as sent; a packet shorter than 16 bytes is all tail and a packet of 0 bytes is nothing.  Here that is one more
 * phase in front of ohgpu_alac_*'s three, a lane per 16-byte block (CBC decryption has no chain), into a plaintext scratch the batch
 * owns; the host never touches a payload byte.  The packet table is ohgpu_alac_packet: src_offset and bytes name the ENCRYPTED
 * PAYLOAD, what follows the 12 header bytes of the datagram (RtpPacketRaop: 4, RaopPacketAudio: 8).
 * Alignment: every packet's src_offset is a multiple of 4 (OHGPU_ERR_INVALID otherwise) -- with the 12-byte header in front of a
 * payload that costs a caller who places datagrams at multiples of 4 nothing.  All other limits are ohgpu_alac_*'s.
 * A stream whose alac.flags is 0, OHGPU_ALAC_OUT_PACKED_LE or _BE is decoded: results, statuses and the meaning of a failed packet
 * are exactly ohgpu_alac_*'s (a wrong key yields bytes that the decoder judges like any others).
 * A stream whose alac.flags is OHGPU_RAOP_OUT_PLAINTEXT is decrypted only (the decryptor alone, for a caller with its own decoder):
 * the plaintext of packet p lands at dst_offset + (src_offset of p - src_offset of the stream's first packet) -- the source layout
 * moved, so the alignment carries over --; bytes between packets are not written; its packets must ascend without overlap
 * (OHGPU_ERR_INVALID), dst_offset is a multiple of 4, dst_plane_stride is 0, alac.config is not read and no packet-size limit
 * applies; every packet's result is OHGPU_ALAC_OK with samples 0.  A batch may mix both kinds.
 * Datagrams arrive lost, doubled and out of order: ohgpu_raop_rx_* (ohgpu_raop_rx.h) is the receiver in front of this
 * family -- the control port's sync and resend packets, repair, the flush window and the latency -- and hands over this packet table.
 * The RSA unwrap of the session key, RTSP / SDP and the timing port stay the caller's. */
#define OHGPU_RAOP_OUT_PLAINTEXT 0x04u   /* in alac.flags: no decode */

typedef struct ohgpu_raop_stream_desc {  /* 96 bytes */
    ohgpu_alac_stream_desc alac;         /* config, packet range, destination, output form: as for ohgpu_alac_* */
    uint8_t aes_key[16];                 /* the session key as sent (after the RSA unwrap, which is the caller's) */
    uint8_t aes_iv[16];
} ohgpu_raop_stream_desc;

/* Host only, no device needed: the SDP fmtp string as CodecRaopApple::ParseFmtp reads it (CodecRaopApple.cpp:173-214): twelve decimal
 * fields separated by blanks -- field 0 is ignored, fields 1..11 are frame_length, compatible_version, bit_depth, pb, mb, kb,
 * channels, max_run, max_frame_bytes, avg_bit_rate, sample_rate ("96 352 0 16 40 10 14 2 255 0 0 44100").  Fields behind the
 * twelfth are ignored, as there.  OHGPU_ERR_INVALID: fewer fields, a field that is no decimal number, a compatible version other
 * than 0, or a value that does not fit its field -- THE ONE DEVIATION: the reference truncates such a value through WriteUint8 /
 * WriteUint16Be and goes on with the wrong configuration. */
int ohgpu_raop_fmtp_parse(const char* fmtp, size_t n, ohgpu_alac_config* config);
/* Host only, no device needed: the validation ohgpu_raop_batch_create makes, with its codes and ohgpu_last_error() texts. */
int ohgpu_raop_batch_check(const ohgpu_raop_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* As ohgpu_alac_batch_create (its codes, its two routes for the Apple Lossless part: ohgpu_batch_paths_info answers alac_route as
 * for an Apple Lossless batch; the decrypt kernel is the same on both).  The key schedules (176 bytes a stream) are made here, on
 * the host, and live in one device array of the batch; ohgpu_batch_destroy clears that array and its host copy before the block
 * goes back to the context's cache.  The work table -- a record per piece of up to 64 blocks of one packet -- is made here from the
 * validated packet table: nothing the device later reads or writes lies outside what this call checked. */
int ohgpu_raop_batch_create(ohgpu_ctx* ctx, const ohgpu_raop_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                            uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* src_base AND dst_base MUST BE 4-BYTE ALIGNED (the kernel loads and stores dwords): OHGPU_ERR_INVALID otherwise, before anything is
 * queued.  Decrypt (into the batch's scratch, each packet at a 16-byte boundary; plaintext streams straight into the destination),
 * then entropy, predictor, matrix and store over that scratch: one stream, nothing waits for the host.  A second run, and a second
 * batch of the same shape, allocate nothing (ohgpu_device_allocations). */
int ohgpu_raop_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* As ohgpu_alac_batch_results, over the caller's packet table. */
int ohgpu_raop_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_stream_result* streams, size_t n,
                             ohgpu_alac_packet_result* packets, size_t n_packets);
/* The last run's phases in milliseconds from device events: decrypt, entropy, predictor, matrix and store (waits for that run).  On
 * the plain route the three Apple Lossless phases are one: the other two read as 0. */
int ohgpu_raop_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4]);
/* Host-buffer convenience, as ohgpu_alac_process_host: one upload, one run.  Of dst_host only the samples of packets that decoded,
 * and the plaintext streams' packets, are written.  src_host is copied to a device arena, so its own alignment is free. */
int ohgpu_raop_process_host(ohgpu_ctx* ctx, const ohgpu_raop_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                            const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                            ohgpu_alac_stream_result* stream_results, ohgpu_alac_packet_result* packet_results);

/* ---- FlywheelRamper ----
 * Replaces FlywheelRamperManager::Ramp (OpenHome/Media/FlywheelRamper.cpp:44-66; per channel FlywheelRamper::Initialise
 * :176-226 = decimate, Burg's method :246-314, coefficient correction :333-372, and FeedbackModel::NextSample :449-487;
 * rendering with sample hold :83-131) for a batch of starving streams: one descriptor = one stream's ramp request.
 * Training audio is what FlywheelInput prepares (StarvationRamper.cpp:90-111, 159-186 = OHGPU_FMT_UNPACK_PLANAR):
 * planar big-endian 32-bit, channel c at src_offset + c * channel_bytes; of each plane the LAST in_samples * 4 bytes
 * are used (Initialise skips older audio, :189-194).  Output: interleaved big-endian 32-bit, what RenderChannels hands
 * to IPcmProcessor::ProcessFragment(buf, channels, 4) in blocks of block_frames. */
typedef struct ohgpu_flywheel_desc {     /* 48 bytes */
    uint64_t src_offset;
    uint64_t channel_bytes;         /* bytes per channel plane, >= in_samples * 4 */
    uint64_t dst_offset;            /* out_frames * channels * 4 bytes are written here */
    uint32_t in_samples;            /* Jiffies::ToSamples(training jiffies, rate); in_samples / decimation >= 4 */
    uint32_t out_frames;            /* Jiffies::ToSamples(ramp jiffies, rate) */
    uint32_t block_frames;          /* Jiffies::ToSamples(kMaxOutputJiffiesBlockSize = 1 ms, rate): the hold counter restarts per block */
    uint32_t sample_rate;           /* decides the decimation factor (FlywheelRamper.cpp:316-331); <= 384000 */
    uint32_t channels;              /* 1..10 (kMaxChannelCount) */
    uint32_t reserved;
} ohgpu_flywheel_desc;

int ohgpu_flywheel_batch_create(ohgpu_ctx* ctx, const ohgpu_flywheel_desc* descs, size_t n,
                                uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
int ohgpu_flywheel_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* Host-buffer convenience: H2D, run, D2H, sync (dst_host bytes that no request covers are preserved). */
int ohgpu_flywheel_process_host(ohgpu_ctx* ctx, const ohgpu_flywheel_desc* descs, size_t n,
                                const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes);

/* ---- Songcast sender frames ----
 * Replaces, for a batch of 5 ms packets of many streams, what Sender::SendPendingAudio (Av/Songcast/Sender.cpp:307-321)
 * and OhmSenderDriver::SendAudio (Av/Songcast/OhmSender.cpp:418-480) do per packet on the pipeline thread:
 *   MsgPlayable::Read of every pending message (attenuation, ramp; Msg.cpp:2646-2653)      the fragment's ramp fields
 *   Sender::DoProcessFragment (Sender.cpp:351-377): first two channels, <= 3 bytes each      fused into the same pass
 *   OhmMsgAudio::ReinitialiseFields + Serialise (OhmMsg.cpp:203-223, 363-413),
 *   OhmHeader::Externalise (Ohm.cpp:44-52), OhmMsgAudio::GetStreamHeader (OhmMsg.cpp:225-241)  the frame header kernel
 * Each frame is written to dst_base + dst_offset as the datagram OhmMsgAudio::SendableBuffer hands to the socket:
 *   "Ohm " 01 03 <total:2> | 32 <flags> <samples:2> <frame:4> <network ts:4> <media latency:4> <media ts:4> <sample start:8>
 *   | <samples total:8> <sample rate:4> <bit rate:4> <volume offset:2> <bit depth> <channels> 00 <codec len> <codec> | audio
 * (big endian).  Sending it, resend history and timestamping stay with the host. */
#define OHGPU_OHM_FLAG_HALT        0x01u   /* OhmMsgAudio::kFlagHalt .. kFlagResent, OhmMsg.h:67-70 */
#define OHGPU_OHM_FLAG_LOSSLESS    0x02u
#define OHGPU_OHM_FLAG_TIMESTAMPED 0x04u   /* the frame also gets kFlagTimestamped2 (OhmMsg.cpp:211) */
#define OHGPU_OHM_FLAG_RESENT      0x08u
#define OHGPU_OHM_MAX_CODEC_BYTES  29u     /* OhmMsgAudio::kMaxCodecBytes */
#define OHGPU_OHM_MAX_AUDIO_BYTES  5760u   /* OhmMsgAudio::kMaxSampleBytes */

typedef struct ohgpu_ohm_stream {   /* 64 bytes: what Sender::ProcessMsg(MsgDecodedStream*) (Sender.cpp:217-242) fixes for a stream */
    uint64_t samples_total;         /* TrackLength / Jiffies::PerSample */
    uint32_t sample_rate;
    uint32_t bit_rate;
    int16_t  volume_offset;         /* OhmSenderDriver::SetAudioFormat passes 0 */
    uint8_t  src_channels;          /* 1..10: the pipeline's channel count; the wire carries min(channels, 2), taken from
                                       channel 0, or channel 8 when there are >= 10 (Sender::FirstChannelToSend) */
    uint8_t  src_bits;              /* 8/16/24/32: the pipeline's depth; the wire carries min(bits, 24) */
    uint8_t  codec_bytes;           /* 0..29 */
    uint8_t  codec[29];
    uint8_t  src_endian;            /* 0 or OHGPU_ENDIAN_BIG: audio as DecodedAudio stores it (always big endian in the
                                       reference); OHGPU_ENDIAN_LITTLE: codec output not yet swapped (row a1 fused in) */
    uint8_t  reserved[13];
} ohgpu_ohm_stream;

typedef struct ohgpu_ohm_fragment { /* 24 bytes: one pending message's MsgPlayable read into the frame (Sender.cpp:312-316) */
    uint64_t src_offset;            /* packed big-endian interleaved audio at the stream's src_channels / src_bits */
    uint32_t n_frames;
    uint16_t ramp_start;
    uint16_t ramp_end;
    uint16_t attenuation;           /* 256 = unity; other values only on 16-bit audio */
    uint8_t  flags;                 /* OHGPU_FLAG_RAMP | OHGPU_FLAG_SILENCE */
    uint8_t  reserved[5];
} ohgpu_ohm_fragment;

typedef struct ohgpu_ohm_frame_desc {   /* 48 bytes: one OhmSenderDriver::SendAudio */
    uint64_t dst_offset;            /* the datagram starts here; ohgpu_ohm_frame_layout gives its size */
    uint64_t sample_start;          /* iSampleStart */
    uint32_t stream;                /* index into streams[] */
    uint32_t frame;                 /* iFrame */
    uint32_t network_timestamp;
    uint32_t media_latency;         /* iLatencyOhm */
    uint32_t media_timestamp;       /* 0 from this sender (OhmMsg.cpp:217) */
    uint32_t first_fragment;        /* fragments[first_fragment .. first_fragment + n_fragments) make up the audio, in order */
    uint16_t n_fragments;
    uint8_t  flags;                 /* OHGPU_OHM_FLAG_* */
    uint8_t  reserved[5];
} ohgpu_ohm_frame_desc;

/* Sizes of a frame of `samples` sample instants: the header (8 + 50 + codec_bytes) and the whole datagram. */
int ohgpu_ohm_frame_layout(const ohgpu_ohm_stream* stream, uint32_t samples, uint32_t* header_bytes, uint32_t* frame_bytes);
/* OHGPU_ERR_INVALID where the reference asserts: more audio than OhmMsgAudio::kMaxSampleBytes in a frame (Sender.cpp:364),
 * a codec name over 29 bytes; OHGPU_ERR_UNSUPPORTED for ramped/silent/attenuated fragments, and for any fragment of a
 * little-endian source, of more than 8 channels (those take the message path, which carries at most 8). */
int ohgpu_ohm_batch_create(ohgpu_ctx* ctx, const ohgpu_ohm_stream* streams, size_t n_streams,
                           const ohgpu_ohm_frame_desc* frames, size_t n_frames,
                           const ohgpu_ohm_fragment* fragments, size_t n_fragments,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
int ohgpu_ohm_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* Host-buffer convenience: H2D, run, D2H, sync (dst_host bytes that no frame covers are preserved). */
int ohgpu_ohm_process_host(ohgpu_ctx* ctx, const ohgpu_ohm_stream* streams, size_t n_streams,
                           const ohgpu_ohm_frame_desc* frames, size_t n_frames,
                           const ohgpu_ohm_fragment* fragments, size_t n_fragments,
                           const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes);

/* ---- Songcast receiver: parse, reorder and unpack OHM audio (the text is csrc/ohm_rx_core.h) ----
 * The other end of ohgpu_ohm_*: received datagrams in, big-endian interleaved PCM at the wire's depth out -- what the reference's
 * ProtocolOhm / ProtocolOhu hand to CodecPcm.  Per datagram OhmHeader::Internalise (Av/Songcast/Ohm.cpp:22-42) and
 * OhmMsgAudio::Create(IReader&, const OhmHeader&) (OhmMsg.cpp:101-175); per stream ProtocolOhBase::Process(OhmMsgAudio&), Repair,
 * RepairReset and the decisions of OutputAudio (ProtocolOhBase.cpp:254-553); then OutputData(aMsg.Audio()).  Three launches on one
 * stream -- parse (a lane per datagram), sequence (a lane per stream), gather (a wave per datagram) -- and no host synchronisation.
 * The source arena holds the datagrams as they came off the socket, each a whole OHM message at a src_offset that is a multiple of
 * 4; a stream's datagrams are listed in arrival order.  Messages of other types (track, metatext, join, listen, leave, slave,
 * resend, audio blob) may be in the table: they are reported (status, msg_type), not interpreted.  Timers, sockets, join / listen,
 * track and metatext stay the caller's; the resend request a repair timer would make at the end of the batch is in the result. */
#define OHGPU_OHM_RX_OK          0u
#define OHGPU_OHM_RX_NOT_OHM     1u   /* wrong magic or major version, or a type OhmHeader::Internalise throws OhmError for (Ohm.cpp:35) */
#define OHGPU_OHM_RX_NOT_AUDIO   2u   /* a valid header of another type: msg_type says which */
#define OHGPU_OHM_RX_TRUNCATED   3u   /* fewer than 8 bytes; the header's total is not the table's `bytes`; below 8 + 50 + codec bytes */
#define OHGPU_OHM_RX_BAD_HEADER  4u   /* audio header length != 50, reserved byte != 0, codec name over 29 bytes (the reference ASSERTs) */
#define OHGPU_OHM_RX_OVERSIZE    5u   /* more than OHGPU_OHM_MAX_AUDIO_BYTES audio bytes */
/* (the checks are made in this order -- csrc/ohm_rx_core.h -- and the first that fails names the status; every status but OK is
 * ignored by the sequencer and the stream goes on, as ProtocolOhm swallows OhmError, ProtocolOhm.cpp:209) */
#define OHGPU_OHM_RX_OUTPUT            1u   /* its audio is in the stream's run at dst_offset; `order` is its place in the output order */
#define OHGPU_OHM_RX_DUPLICATE         2u   /* a frame already waiting, or a resent frame at or behind the last one output */
#define OHGPU_OHM_RX_PENDING           3u   /* still waiting at the end of the batch: `order` is its place in the replay (below) */
#define OHGPU_OHM_RX_DROPPED_BY_RESET  4u   /* the frame that caused a RepairReset, and every frame that waited when one ran */
#define OHGPU_OHM_RX_STALE             5u   /* a frame in the past that is no resend, outside a repair: the stream stops (ReaderError) */
#define OHGPU_OHM_RX_NOT_REACHED       6u   /* behind the datagram the stream stopped at */
#define OHGPU_OHM_RX_IGNORED           7u   /* status != OK */
#define OHGPU_OHM_RX_EVENT_NEW_STREAM  1u   /* OutputAudio sends a MsgDecodedStream in front of this frame (ProtocolOhBase.cpp:464-488) */
#define OHGPU_OHM_RX_EVENT_DELAY       2u   /* ... a delay: the rate or the media latency changed (:489-493) */
#define OHGPU_OHM_RX_EVENT_HALT        4u   /* the wire's halt flag: wait and halt behind this frame, and the stream stops (:504-512) */
#define OHGPU_OHM_RX_STOP_NONE   0u
#define OHGPU_OHM_RX_STOP_STALE  1u
#define OHGPU_OHM_RX_STOP_HALT   2u
#define OHGPU_OHM_RX_MAX_RESEND  20u   /* ProtocolOhBase::kMaxRepairMissedFrames */

typedef struct ohgpu_ohm_rx_datagram {   /* 16 bytes */
    uint64_t src_offset;            /* a multiple of 4 */
    uint32_t bytes;                 /* as recvfrom returned */
    uint32_t reserved;
} ohgpu_ohm_rx_datagram;

typedef struct ohgpu_ohm_rx_state {      /* 32 bytes: what ProtocolOhBase carries from one datagram to the next */
    uint64_t last_sample_start;     /* iLastSampleStart (UINT_MAX, 0xffffffff, in a new receiver) */
    uint32_t frame;                 /* iFrame */
    uint32_t sample_rate;           /* iSampleRate */
    uint32_t latency;               /* iLatency (the wire's media latency) */
    uint8_t  running;               /* iRunning */
    uint8_t  stream_msg_due;        /* iStreamMsgDue (1 in a new receiver) */
    uint8_t  bit_depth;             /* iBitDepth */
    uint8_t  channels;              /* iNumChannels */
    uint32_t reserved[2];
} ohgpu_ohm_rx_state;

typedef struct ohgpu_ohm_rx_stream {     /* 64 bytes */
    uint32_t first_datagram;        /* the stream's datagrams are [first_datagram, + n_datagrams) of the table, in arrival order; */
    uint32_t n_datagrams;           /*   the streams' ranges tile the table in the streams' order */
    uint64_t dst_offset;            /* the output run starts here, any byte address */
    uint64_t dst_capacity;          /* >= the sum over the stream's datagrams of max(bytes - 58, 0): no parse is needed to size it */
    ohgpu_ohm_rx_state state_in;
    uint32_t reserved[2];
} ohgpu_ohm_rx_stream;

typedef struct ohgpu_ohm_rx_record {     /* 104 bytes, one per datagram */
    uint8_t  status;                /* OHGPU_OHM_RX_OK ... _OVERSIZE */
    uint8_t  disposition;           /* OHGPU_OHM_RX_OUTPUT ... _IGNORED */
    uint8_t  events;                /* OHGPU_OHM_RX_EVENT_*, of an OUTPUT record */
    uint8_t  flags;                 /* the wire's: OHGPU_OHM_FLAG_* and 0x10 (timestamped2) */
    uint8_t  msg_type;              /* OhmHeader's type, from NOT_AUDIO on (0 for NOT_OHM and a TRUNCATED header) */
    uint8_t  bit_depth, channels, codec_bytes;      /* every field from here on is 0 unless status is OK */
    uint16_t samples;
    int16_t  volume_offset;
    uint32_t frame, network_timestamp, media_latency, media_timestamp, sample_rate;
    uint64_t sample_start, samples_total;
    uint32_t bit_rate;
    uint32_t audio_offset;          /* of the payload within the datagram: 58 + codec_bytes */
    uint32_t audio_bytes;
    uint32_t order;                 /* OUTPUT: 0, 1, ... in the stream's output order; PENDING: 0, 1, ... in replay order */
    uint64_t dst_offset;            /* OUTPUT: where its audio_bytes lie in the destination arena */
    uint8_t  codec[32];
} ohgpu_ohm_rx_record;

typedef struct ohgpu_ohm_rx_stream_result {   /* 136 bytes */
    ohgpu_ohm_rx_state state_out;   /* the state to give the next batch.  After a stop it is what WaitForPipelineToEmpty's RepairReset
                                       leaves (ProtocolOhBase.cpp:157-160): not running, stream message due, frame and format kept */
    uint64_t out_bytes;             /* the run [dst_offset, + out_bytes) was written */
    uint32_t n_output;
    uint32_t n_pending;             /* PENDING records: the caller queues those datagrams, in `order`, in front of the next batch's
                                       arrivals -- that replay rebuilds the waiting set with no event */
    uint32_t stop_reason;           /* OHGPU_OHM_RX_STOP_* */
    uint32_t n_resend;              /* what TimerRepairExpired would ask for now (:407-447): the first 20 missing frames below the */
    uint32_t resend[20];            /*   highest waiting one, ascending -- with the reference's unsigned loops: a gap that spans the
                                       2^32 wrap contributes nothing */
} ohgpu_ohm_rx_stream_result;

/* Host only, no device needed: the validation ohgpu_ohm_rx_batch_create makes.  OHGPU_ERR_INVALID: a src_offset that is no multiple
 * of 4, stream ranges that overlap or leave part of the table out, non-zero reserved fields.  OHGPU_ERR_BOUNDS: a datagram outside
 * the source arena, a destination run [dst_offset, + dst_capacity) that ends outside the destination arena, or a dst_capacity below
 * the sum over the stream's datagrams of max(bytes - 58, 0) -- so the device never has to refuse for room.  Destination runs of
 * different streams must not overlap (not checked: as for every other family, overlapping outputs are the caller's mistake). */
int ohgpu_ohm_rx_batch_check(const ohgpu_ohm_rx_stream* streams, size_t n, const ohgpu_ohm_rx_datagram* datagrams, size_t n_datagrams,
                             uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* The tables go to the device; records, results and the sequencer's rings are the batch's, from the context's block cache.  An empty
 * batch (no streams, no datagrams) is legal.  Freed with ohgpu_batch_destroy. */
int ohgpu_ohm_rx_batch_create(ohgpu_ctx* ctx, const ohgpu_ohm_rx_stream* streams, size_t n, const ohgpu_ohm_rx_datagram* datagrams, size_t n_datagrams,
                              uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* src_base MUST BE 4-BYTE ALIGNED (the parse and the gather load dwords): OHGPU_ERR_INVALID otherwise, before anything is queued;
 * dst_base may be any address.  Parse, sequence, gather: queued on the stream, nothing waits for the host.  The batch owns its
 * records: it runs on one stream at a time.  A second run allocates nothing on the device (ohgpu_device_allocations).  The gathered
 * run is what ohgpu_pcm_* / ohgpu_src_* read as their source arena: the next batch may be queued on the same stream at once. */
int ohgpu_ohm_rx_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's results (waits for that run): per stream (n = the batch's stream count) and / or per datagram (n_datagrams = the
 * table's length); either pointer may be NULL with its count 0. */
int ohgpu_ohm_rx_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ohm_rx_stream_result* streams, size_t n,
                               ohgpu_ohm_rx_record* records, size_t n_datagrams);
/* The last run's phases in milliseconds from device events: parse, sequence, gather (waits for that run). */
int ohgpu_ohm_rx_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[3]);
/* Host-buffer convenience: one upload, one run, and of dst_host the bytes [dst_offset, + out_bytes) of every stream.  Either result
 * pointer may be NULL. */
int ohgpu_ohm_rx_process_host(ohgpu_ctx* ctx, const ohgpu_ohm_rx_stream* streams, size_t n, const ohgpu_ohm_rx_datagram* datagrams, size_t n_datagrams,
                              const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                              ohgpu_ohm_rx_stream_result* stream_results, ohgpu_ohm_rx_record* records);

/* ---- Ogg pages: find, checksum, join into packets, gather (the text is csrc/ogg_page_core.h) ----
 * What libogg's page reader and libFLAC's Ogg aspect do in front of the FLAC frame decoder (RFC 3533): the bytes of an Ogg stream
 * in, the bytes of its completed packets out, concatenated from dst_offset on at any byte alignment -- for an Ogg FLAC stream the
 * run ohgpu_flac_* reads -- with a record per packet and a result per stream.  Four launches on one stream: find (a lane per byte
 * position), verify (a wave per page: its CRC-32 in 64 slices, joined with the x^(8 len) multiplication), chain (a lane per stream:
 * the walk below), gather (a wave per piece of page body).  No host synchronisation.
 * The walk, from src_offset, at position p:
 *   1. fewer than 27 bytes, than the header (27 + segments) or than the whole page are left: the range ends here, status OK.
 *   2. 27 bytes or more without "OggS" at p, or a whole page whose CRC does not match: LOST_SYNC, stop.  Nothing is skipped.
 *   3. a whole page with a good CRC whose serial is not the stream's or whose version is not 0 is counted (pages_ignored) and passed
 *      over.  With OHGPU_OGG_ANY_SERIAL the stream's serial is that of the first whole page.
 *   4. an accepted page's number must be expect_seq, then one more each page (mod 2^32): HOLE otherwise, stop in front of that
 *      page.  With OHGPU_OGG_ANY_SEQ the first accepted page may carry any number.
 *   5. a packet is a run of lacing values 255 closed by one below 255, over any number of pages.  The "continued" flag matters in
 *      one place: on a page that sets it while no packet is open, the leading segments up to and including the first below 255 are
 *      dropped with their bytes (all of them, when all are 255).  On the first accepted page first_page_segment = r > 0 skips
 *      segments [0, r) and their bytes instead, and the packet at r is a fresh one; r above that page's segment count is BAD_RESUME.
 *   6. only completed packets are delivered.  With OHGPU_OGG_FLAC_MAPPING a completed packet whose first byte is 0x7f is the
 *      mapping's first header: shorter than 9 bytes or without "FLAC" at 1 is NOT_FLAC, a major version (byte 5) other than 1 is
 *      UNSUPPORTED_MAPPING, both stop; otherwise its first 9 bytes are not delivered.  Every packet is tested.
 *   7. a packet still open where the range ends is not delivered: bytes_consumed is then the offset of the page it began on,
 *      resume_segment its first segment there and next_seq that page's number.  With no packet open bytes_consumed is the end of the
 *      last whole page, resume_segment 0 and next_seq the last accepted number plus 1.  On a stop status bytes_consumed is the
 *      offset of the page the walk stopped at (for the mapping's two, the page the header packet ended on), and what completed
 *      before it is delivered.  A later call with (src_offset + bytes_consumed, expect_seq = next_seq, first_page_segment =
 *      resume_segment) delivers exactly what one call over the whole range would have delivered behind that point.
 * Chained streams (an Icecast mount: every track a new logical stream with its own serial, headers and granule positions).  With
 * OHGPU_OGG_FOLLOW_LINKS the descriptor's `link` holds a magic of 0 ... 8 bytes ("\x01vorbis", "\x7fFLAC"; length 0 matches any
 * body), rules 1-7 stand, and rule 3 has one exception:
 *   L1. a whole page with a good CRC and version 0 begins a link when its serial is not the followed one, it has the "first page"
 *       flag, its body begins with the magic, and the followed serial's last accepted page of this call, if there is one, did not
 *       have the "first page" flag (so the opening group of a multiplexed stream, BOS A, BOS B, ..., is no chain).  The link before
 *       it needs no "last page" flag.  A foreign first page that fails any of these is counted and passed over by rule 3.
 *   L2. at a link a packet still open is dropped, neither delivered nor counted; the followed serial becomes the page's; the page
 *       may carry any number and every later page one more (rule 4); rule 5's first_page_segment no longer applies; the first
 *       packet that begins in the new link gets OHGPU_OGG_PACKET_LINK, and OHGPU_OGG_PACKET_BOS by its own rule; with
 *       OHGPU_OGG_FLAC_MAPPING the new link's mapping header is stripped by rule 6 as any other.
 *   L3. the result's `serial` is the serial followed at the end and `links` counts the links taken, whether or not their packets
 *       were recorded.  last_granule, bos_seen and eos_seen are over every link.
 *   L4. rule 7 holds: a later call with serial = the result's serial, the flag and the same magic delivers what one call would
 *       have.  For that, a link none of whose packets has completed where the range ends (status OK) is left for the later call
 *       to take: the result is that of a range which ends in front of the link's first page (bytes_consumed that page's offset,
 *       resume_segment 0, next_seq, serial, pages, pages_ignored, bos_seen, eos_seen and links as they were there).  The known
 *       exception: a range that ends exactly between two first pages of one opening group that both match the magic -- the later
 *       call has not seen the first of them and takes the second for a link.
 *   L5. a link that reuses the serial being followed is not a link: its first page is a page of that serial and fails rule 4 with
 *       HOLE (or, with the number that happens to follow, is accepted as the stream's next page).
 * Without the flag nothing above applies and the reserved words must be zero. */
#define OHGPU_OGG_OK                   0u
#define OHGPU_OGG_LOST_SYNC            1u
#define OHGPU_OGG_HOLE                 2u
#define OHGPU_OGG_NOT_FLAC             3u
#define OHGPU_OGG_UNSUPPORTED_MAPPING  4u
#define OHGPU_OGG_BAD_RESUME           5u
#define OHGPU_OGG_ANY_SEQ        1u
#define OHGPU_OGG_FLAC_MAPPING   2u
#define OHGPU_OGG_ANY_SERIAL     4u
#define OHGPU_OGG_FOLLOW_LINKS   16u  /* rules L1-L5 (8 is not a flag) */
#define OHGPU_OGG_PACKET_BOS             1u   /* it starts with the first segment of a page that has the "first page" flag */
#define OHGPU_OGG_PACKET_EOS             2u   /* it contains the last segment of a page that has the "last page" flag */
#define OHGPU_OGG_PACKET_MAPPING_HEADER  4u   /* the mapping's first header: `bytes` is what is left of it without its first 9 */
#define OHGPU_OGG_PACKET_LINK            8u   /* the first packet that begins in a link taken by rule L1 */

typedef struct ohgpu_ogg_link_magic {   /* 12 bytes */
    uint32_t bytes;                 /* 0 ... 8; 0 matches any body */
    uint8_t  magic[8];              /* zero beyond `bytes` */
} ohgpu_ogg_link_magic;

typedef struct ohgpu_ogg_stream_desc {   /* 64 bytes */
    uint64_t src_offset;            /* the stream's bytes are [src_offset, + src_bytes) of the source arena, any address */
    uint64_t dst_offset;            /* the delivered run starts here, any address */
    uint64_t dst_capacity;          /* >= src_bytes: delivery can never run out of room */
    uint32_t src_bytes;             /* < 2^31 */
    uint32_t serial;                /* the logical stream's (ignored with OHGPU_OGG_ANY_SERIAL) */
    uint32_t expect_seq;            /* the number the first accepted page must carry (ignored with OHGPU_OGG_ANY_SEQ) */
    uint32_t packet_first;          /* the stream's records are [packet_first, + packet_capacity) of the batch's packet table; */
    uint32_t packet_capacity;       /*   packets beyond the capacity are counted, not recorded.  0: no records */
    uint32_t first_page_segment;    /* rule 5's r, <= 255 */
    uint32_t flags;                 /* OHGPU_OGG_ANY_SEQ | _FLAC_MAPPING | _ANY_SERIAL | _FOLLOW_LINKS */
    union {
        uint32_t reserved[3];       /* without OHGPU_OGG_FOLLOW_LINKS: zero */
        ohgpu_ogg_link_magic link;  /* with it: what the body of a link's first page begins with */
    };
} ohgpu_ogg_stream_desc;

typedef struct ohgpu_ogg_stream_result {   /* 64 bytes */
    uint32_t status;                /* OHGPU_OGG_OK ... _BAD_RESUME */
    uint32_t pages;                 /* accepted */
    uint32_t pages_ignored;         /* rule 3 */
    uint32_t packets;               /* completed and delivered, recorded or not */
    uint64_t bytes_delivered;       /* the run [dst_offset, + bytes_delivered) was written */
    uint64_t bytes_consumed;        /* rule 7 */
    uint32_t resume_segment;
    uint32_t next_seq;
    int64_t  last_granule;          /* the last granule position other than -1 that a delivered packet got (-1: none) */
    uint32_t serial;                /* the stream's: the descriptor's, or the first whole page's; with links, the one followed at the end */
    uint8_t  bos_seen, eos_seen;    /* an accepted page had the "first page" / "last page" flag */
    uint8_t  reserved[2];
    union {
        uint64_t reserved2;         /* the high half is zero */
        uint32_t links;             /* its low half: rule L3 (0 without OHGPU_OGG_FOLLOW_LINKS) */
    };
} ohgpu_ogg_stream_result;

typedef struct ohgpu_ogg_packet {   /* 40 bytes */
    uint64_t run_pos;               /* its delivered bytes are [dst_offset + run_pos, + bytes) */
    uint32_t bytes;
    uint32_t flags;                 /* OHGPU_OGG_PACKET_* */
    int64_t  granule;               /* the page's, for the last packet that ends on a page; -1 for the others */
    uint64_t page_offset;           /* where it began: the page (from src_offset), ... */
    uint32_t page_seq;              /* ... that page's number, ... */
    uint32_t segment;               /* ... and the segment */
} ohgpu_ogg_packet;

/* Host only, no device needed: the validation ohgpu_ogg_batch_create makes.  OHGPU_ERR_INVALID: non-zero reserved words without
 * OHGPU_OGG_FOLLOW_LINKS, with it a magic longer than 8 bytes or non-zero bytes beyond its length, unknown flags, src_bytes >= 2^31, first_page_segment > 255, packet ranges that overlap or run past the table of n_packets records.
 * OHGPU_ERR_BOUNDS: a range outside its arena, dst_capacity < src_bytes.  The empty batch is legal. */
int ohgpu_ogg_batch_check(const ohgpu_ogg_stream_desc* descs, size_t n, size_t n_packets, uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* The descriptors go to the device; lists, bitmap, plan, packet table and results are the batch's.  Freed with ohgpu_batch_destroy. */
int ohgpu_ogg_batch_create(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* descs, size_t n, size_t n_packets, uint64_t src_arena_bytes, uint64_t dst_arena_bytes,
                           ohgpu_batch** batch);
/* Find, verify, chain, gather: queued on the stream, nothing waits for the host.  Both bases may be any address.  The batch owns its
 * lists: it runs on one stream at a time.  A second run allocates nothing on the device (ohgpu_device_allocations).  The delivered
 * runs are what ohgpu_flac_* reads as its source arena: that batch may be queued on the same stream at once. */
int ohgpu_ogg_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's results, n = the batch's stream count (waits for that run). */
int ohgpu_ogg_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ogg_stream_result* results, size_t n);
/* The last run's packet table, n_packets = the table's length; of a stream's range the first min(packets, packet_capacity) records
 * are that run's (waits for that run). */
int ohgpu_ogg_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ogg_packet* packets, size_t n_packets);
/* The last run's phases in milliseconds from device events: find, verify, chain, gather (waits for that run). */
int ohgpu_ogg_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4]);
/* Host-buffer convenience: one upload, one run, and of dst_host the bytes [dst_offset, + bytes_delivered) of every stream.  Either
 * result pointer may be NULL. */
int ohgpu_ogg_process_host(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* descs, size_t n, size_t n_packets, const void* src_host, uint64_t src_bytes,
                           void* dst_host, uint64_t dst_bytes, ohgpu_ogg_stream_result* results, ohgpu_ogg_packet* packets);
/* Host only: the page checksum of any bytes (polynomial 0x04c11db7, start 0, no reflection, no final complement). */
uint32_t ohgpu_ogg_crc(const void* bytes, size_t n);
/* Host only: the head of an Ogg FLAC stream (CodecFlac::Recognise's second kind: "OggS" at 0, "fLaC" at 37).  Walks the leading
 * pages of `bytes` (any serial, any first page number, the mapping header applied), reads "fLaC" and the metadata blocks out of the
 * packets' bytes through ohgpu_flac_streaminfo, and answers where the first audio packet begins: the page's offset, the segment in
 * it, that page's number -- the (src_offset, first_page_segment, expect_seq) of the stream's first ohgpu_ogg_stream_desc.
 * OHGPU_ERR_INVALID: not Ogg FLAC, or the bytes end inside the metadata.  OHGPU_ERR_UNSUPPORTED: a metadata block that does not
 * end with its packet. */
int ohgpu_ogg_flac_head(const void* bytes, size_t n, ohgpu_flac_streaminfo_t* info, uint32_t* serial, uint64_t* audio_page_offset, uint32_t* audio_segment,
                        uint32_t* audio_seq);
/* Ogg FLAC from host buffers: one upload of the Ogg bytes, the demux into a middle arena of mid_bytes that lives on the device only,
 * one small read of the Ogg results, a FLAC batch over the delivered runs (flac_descs[i].src_offset must be ogg_descs[i].dst_offset,
 * an offset into the middle arena; its src_bytes is replaced by the stream's bytes_delivered), and of dst_host the samples that
 * were decoded.  The demuxed bytes never visit the host.  Any result pointer may be NULL; frames as ohgpu_flac_batch_frames. */
int ohgpu_ogg_flac_process_host(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* ogg_descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets,
                                const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                ohgpu_ogg_stream_result* ogg_results, ohgpu_ogg_packet* packets,
                                ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames);

/* ---- MPEG-4 container: boxes and sample tables in front of the Apple Lossless decoder (the text is csrc/mp4_box_core.h) ----
 * What Codec/Mpeg4.cpp does in front of CodecAlacApple: the bytes of an .m4a file (ISO/IEC 14496-12), or of a prefix of one, in; one
 * ohgpu_alac_packet row and one ohgpu_mp4_sample row per sample of the first Apple Lossless track out, with a result per stream.  The
 * packets are decoded where they lie in `mdat`: the rows point into the source arena, nothing is copied.
 * The walk, in file order, at most OHGPU_MP4_MAX_BOXES box headers a stream (one more: INVALID).  The first thing wrong gives the
 * status, error_offset is the box that gave it, and every other field of a refused stream reads 0 (first_bad_sample 0xffffffff):
 *   - a box is u32 size, fourcc; size 1: a u64 size follows; size 0: to the end of the stream, at top level only.  A size below its own
 *     header, or a child that ends behind its parent, is INVALID.  Fewer than 8 bytes left in a parent end it.
 *   - bytes 4..8 must be "ftyp" (Mpeg4.cpp:4692): NOT_MP4.  A stream of fewer than 8 bytes is TRUNCATED.
 *   - top level: `moof` is UNSUPPORTED; the first `mdat` is recorded; the first `moov` is entered, before or behind `mdat`, and one
 *     that reaches past src_bytes is TRUNCATED; any other box is skipped by its size, and one that reaches past src_bytes ends the
 *     walk.  No `moov` by then: TRUNCATED (error_offset: where the walk stood).
 *   - moov > trak > mdia > { mdhd, minf > stbl > { stsd, stts, stsc, stsz, stco | co64 } }.  The first box of each kind counts.
 *     `mvex` in moov and `stz2` in stbl are UNSUPPORTED.  Everything else -- free, udta, meta, uuid, at every level -- is skipped.
 *   - mdhd: version 0 or 1 (32- or 64-bit duration, Mpeg4.cpp:1705-1784); another version, a box too short, timescale 0: INVALID.
 *   - the five tables are version 0 and their entry count fits the box, else INVALID.  stsz: a non-zero sample_size means N samples of
 *     that size and no array (Mpeg4.cpp:1235-1247); N > OHGPU_MP4_MAX_SAMPLES is UNSUPPORTED.
 *   - stsd: the first sample entry only.  Its fourcc is the trak's codec; `enca` is UNSUPPORTED.  In an `alac` entry (shorter than
 *     28 bytes: INVALID): skip 16, channels u16, bit depth u16, skip 4, the rate's upper 16 bits (Mpeg4.cpp:2066-2105), then child
 *     boxes; the inner `alac` box is 4 bytes of version and flags, the 24-byte configuration, perhaps more (AlacApple.cpp:101-128).
 *     No such box, fewer than 28 bytes, a compatible version other than 0, or a configuration ohgpu_alac_batch_check refuses
 *     (channels 1..8, frame length 1..16384, depth 16/20/24/32): UNSUPPORTED.  The configuration rules; the entry's own channels,
 *     depth and rate are reported beside it (AlacApple.cpp:160-175).
 *   - a trak is entered until one has been taken, and is taken at its end when its codec is `alac`.  Then: any of mdhd and the five
 *     tables missing: INVALID (error_offset: the trak).  stsc entries (fc_k, spc_k, .), k < E: fc_0 == 1, fc strictly ascending and
 *     <= C (the chunk count), spc_k >= 1; with run_k = (fc_{k+1}, or C + 1 for the last) - fc_k and S_k = sum_{j<k} run_j spc_j,
 *     S_E >= N; else INVALID (the stsc).  stts entries (count_m, delta_m): the leading entries that cover N samples have count >= 1
 *     and there are enough of them, else INVALID (the stts).  The end of moov with no trak taken: NOT_ALAC, `codec` the first
 *     trak's entry fourcc (0: none), so that a caller can route mp4a, fLaC or Opus elsewhere.
 * The expansion, all sums in 64 bits.  For sample s (from 0): k = the last entry with S_k <= s, r = s - S_k, chunk c = fc_k - 1 +
 * r / spc_k, place in the chunk j = r mod spc_k, file offset = co[c] + sum_{i = s-j}^{s-1} size_i; first_frame and frames come from the
 * stts runs in the same way.  A sample whose bytes leave [0, src_bytes), or whose size is above the Apple Lossless packet limit
 * (frame_length x channels x 5 + 64), is refused: its packet row is {the stream's src_offset, 0 bytes}, which the Apple Lossless phases
 * judge CORRUPT and ohgpu_alac_batch_check accepts; its sample row is written as any other.  Rows [0, min(N, packet_capacity)) of the
 * stream's range are written, and samples_refused, first_bad_sample and samples_available speak of those rows.
 * Where this differs from the reference (tests/mp4_textbook.py carries the same list):
 *   - the reference streams, and fetches a `moov` behind `mdat` out of band; here the bytes are there, and the walk goes on past mdat;
 *   - the reference refuses a file at its second stsz (Mpeg4.cpp:1222-1231); here the first `alac` trak is taken and the rest skipped;
 *   - the reference's box header has no 64-bit size; here it has;
 *   - the reference wants chunk offsets that do not go backwards (Mpeg4.cpp:3540) because it streams; rows are independent here;
 *   - every sum is 64-bit, where the reference's are 32-bit with wrap checks (Mpeg4.cpp:3558);
 *   - a seek lands on the packet that holds the frame.  The reference lands on that packet's chunk (Mpeg4.cpp:3879, its own FIXME),
 *     compares an audio-sample count against a codec-sample total (:3991) and returns an offset within one stts entry as if it were
 *     the track's (:4136-4138); none of the three is reproduced;
 *   - an stts run of no samples among those that cover the track is INVALID (the reference passes over it). */
#define OHGPU_MP4_OK           0u
#define OHGPU_MP4_NOT_MP4      1u
#define OHGPU_MP4_TRUNCATED    2u
#define OHGPU_MP4_INVALID      3u
#define OHGPU_MP4_NOT_ALAC     4u
#define OHGPU_MP4_UNSUPPORTED  5u
#define OHGPU_MP4_MAX_SAMPLES  (1u << 24)
#define OHGPU_MP4_MAX_BOXES    4096u
#define OHGPU_MP4_NO_SAMPLE    0xffffffffu

typedef struct ohgpu_mp4_stream_desc {   /* 32 bytes */
    uint64_t src_offset;            /* the file's bytes are [src_offset, + src_bytes) of the source arena, any address */
    uint32_t src_bytes;             /* < 2^31: the whole file or a prefix of it */
    uint32_t flags;                 /* zero */
    uint32_t packet_first;          /* the stream's rows are [packet_first, + packet_capacity) of both tables; samples beyond the */
    uint32_t packet_capacity;       /*   capacity are counted (`samples`), not expanded.  0: no rows */
    uint32_t reserved[2];           /* zero */
} ohgpu_mp4_stream_desc;

typedef struct ohgpu_mp4_stream_result {   /* 112 bytes */
    uint32_t status;                /* OHGPU_MP4_OK ... _UNSUPPORTED */
    uint32_t codec;                 /* the taken trak's entry fourcc, first character in the top byte ('alac'); NOT_ALAC: the first trak's */
    ohgpu_alac_config config;       /* the inner `alac` box's: what the stream's ohgpu_alac_stream_desc takes */
    uint32_t timescale;             /* mdhd */
    uint32_t entry_rate;            /* the sample entry's: the upper 16 bits of its 16.16 rate */
    uint64_t duration;              /* mdhd, in timescale units */
    uint64_t frames;                /* the sum of stts over the N samples */
    uint32_t samples;               /* N (stsz) */
    uint32_t chunks;                /* C (stco / co64) */
    uint32_t samples_available;     /* the leading rows that were not refused: what a prefix of a file can play */
    uint32_t samples_refused;       /* rows refused */
    uint32_t first_bad_sample;      /* the lowest of them; OHGPU_MP4_NO_SAMPLE: none */
    uint16_t entry_channels, entry_bits;   /* the sample entry's */
    uint64_t moov_offset;           /* from src_offset */
    uint64_t mdat_offset;           /* the first mdat box (its header), and ... */
    uint64_t mdat_bytes;            /* ... its payload as its header states it; both 0 when the walk met none */
    uint64_t error_offset;          /* the box that gave a status other than OK */
} ohgpu_mp4_stream_result;

typedef struct ohgpu_mp4_sample {   /* 16 bytes: one row per sample, beside its ohgpu_alac_packet row */
    uint64_t first_frame;           /* the audio frames in front of it */
    uint32_t frames;                /* its own (its stts run's delta) */
    uint32_t chunk;                 /* from 0 */
} ohgpu_mp4_sample;

/* Host only, no device needed: the validation ohgpu_mp4_batch_create makes.  OHGPU_ERR_INVALID: non-zero reserved words or flags,
 * src_bytes >= 2^31, row ranges that overlap or run past the tables of n_packets rows.  OHGPU_ERR_BOUNDS: a range outside the source
 * arena.  The empty batch is legal. */
int ohgpu_mp4_batch_check(const ohgpu_mp4_stream_desc* descs, size_t n, size_t n_packets, uint64_t src_arena_bytes);
/* The descriptors go to the device; tiles, carries, both tables (every byte 0xa5 until a run writes it) and the results are the
 * batch's.  Created under ohgpu_set_kernel_variant(1) the batch takes the plain route: one launch, a lane per stream runs the walk
 * and the serial expansion (ohgpu_batch_paths_info: mp4_route).  Both routes write the same bytes.  Freed with ohgpu_batch_destroy. */
int ohgpu_mp4_batch_create(ohgpu_ctx* ctx, const ohgpu_mp4_stream_desc* descs, size_t n, size_t n_packets, uint64_t src_arena_bytes, ohgpu_batch** batch);
/* Walk, tile sums, carries, expand: queued on the stream, nothing waits for the host.  The device reads a stream as the aligned 4-byte
 * words that hold its bytes (no load is misaligned): up to 3 bytes in front of src_offset and behind src_offset + src_bytes are loaded
 * and never used, so src_base must be a multiple of 4 and the arena's allocation must end on a multiple of 4 (any hipMalloc block does).  The batch owns its tables: it runs on one
 * stream at a time.  A second run, and a second batch of the same shape, allocate nothing on the device (ohgpu_device_allocations). */
int ohgpu_mp4_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* stream);
/* The last run's results, n = the batch's stream count (waits for that run). */
int ohgpu_mp4_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_stream_result* results, size_t n);
/* The last run's tables, n_packets = their length; of a stream's range the first min(samples, packet_capacity) rows are that run's
 * (waits for that run).  A packet row's src_offset is absolute in the source arena: the rows are what ohgpu_alac_batch_create takes. */
int ohgpu_mp4_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets);
int ohgpu_mp4_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets);
/* The last run's phases in milliseconds from device events: walk, tile sums, carries, expand (waits for that run).  The plain route
 * is one phase: the other three read as 0. */
int ohgpu_mp4_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4]);
/* Host-buffer convenience: one upload, one run, the results and both tables home.  Any of the three pointers may be NULL. */
int ohgpu_mp4_process_host(ohgpu_ctx* ctx, const ohgpu_mp4_stream_desc* descs, size_t n, size_t n_packets, const void* src_host, uint64_t src_bytes,
                           ohgpu_mp4_stream_result* results, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples);
/* Host only: the row of a downloaded sample table that holds audio frame `frame` (a binary search), and that row's first frame.
 * OHGPU_ERR_BOUNDS: the frame lies behind the table's last row. */
int ohgpu_mp4_seek(const ohgpu_mp4_sample* samples, size_t n, uint64_t frame, uint64_t* index, uint64_t* first_frame);
/* .m4a files from host buffers to PCM: one upload of the files' bytes, the MPEG-4 batch, one small read of its results and packet
 * table (16 bytes a packet), an Apple Lossless batch over the same device source arena -- stream i's config from its result, its rows
 * [0, min(samples, packet_capacity)) as its packets, output form (flags), dst_offset and dst_plane_stride from alac_descs[i], whose
 * other fields are ignored -- and of dst_host the samples that decoded.  A stream whose status is not OK contributes no packets; the
 * others are served.  packet_results is indexed as the MPEG-4 tables are (rows that were not decoded read {0, 0}).  Any result
 * pointer may be NULL. */
int ohgpu_mp4_alac_process_host(ohgpu_ctx* ctx, const ohgpu_mp4_stream_desc* mp4_descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets,
                                const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                                ohgpu_mp4_stream_result* mp4_results, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results);

/* ---- Fragmented MPEG-4: movie fragments in front of the FLAC and Apple Lossless decoders (the text is csrc/mp4_frag_core.h) ----
 * What Codec/Mpeg4.cpp's moof switcher does in front of CodecFlac and CodecAlacApple: the bytes of an initialisation segment and its
 * media segments (ISO/IEC 14496-12 movie fragments, as DASH and CMAF deliver them), or of a prefix of them, in; a row a `trun`, an
 * ohgpu_alac_packet row and an ohgpu_mp4_sample row a sample of the taken track, and -- with OHGPU_MP4F_GATHER -- the samples' bytes as
 * one contiguous run out, with a result per stream.  ohgpu_mp4_* keeps answering such a file UNSUPPORTED; this family answers a plain
 * .m4a NOT_FRAGMENTED.  Boxes are read as in the MPEG-4 section above.
 * The walk, in file order, at most OHGPU_MP4F_MAX_BOXES box headers a stream (one more: INVALID; the boxes inside a sample description
 * are counted apart, against OHGPU_MP4_MAX_BOXES).  The first thing wrong gives the status, error_offset is the box that gave it, and
 * every other field of a refused stream reads 0 (first_bad_sample 0xffffffff; `codec` is kept by NOT_CODEC and NOT_FRAGMENTED):
 *   - top level: "ftyp" at bytes 4..8, else NOT_MP4 (fewer than 8 bytes: TRUNCATED).  The first `moov` is entered (it reaches past
 *     src_bytes: TRUNCATED); a `moof` in front of it is INVALID; every `moof` behind it is entered; a `moof`, or any other box, that
 *     reaches past src_bytes ends the walk -- what stood in front of it is served.  mdat, sidx, styp, free and the rest are skipped by
 *     their size.  No `moov`: TRUNCATED.
 *   - moov: a `trak` is entered until one is taken; it is taken at its end when its first sample entry is in `codecs`.  tkhd gives
 *     track_id (version 0 or 1, else INVALID), mdia/mdhd the timescale and the duration (the MPEG-4 section's rules); the first stsd
 *     gives the entry.  `enca`: UNSUPPORTED.  An `alac` entry follows exactly the MPEG-4 section's rules.  A `fLaC` entry (read only
 *     when `codecs` asks for it) shorter than 28 bytes is INVALID; behind the same 28-byte head come child boxes, of which `dfLa`
 *     (FLAC-in-ISOBMFF) holds 4 bytes of version and flags -- not 0: UNSUPPORTED -- and metadata blocks of 1 byte (last flag | type)
 *     and a 24-bit length.  Fewer than 4 bytes, no block, a block that leaves the box, a first block that is not STREAMINFO of 34
 *     bytes: INVALID.  A depth other than 8, 16 or 24: UNSUPPORTED.  The blocks behind STREAMINFO are skipped, up to the one with the
 *     last flag or the end of the box.  No dfLa: UNSUPPORTED.  A taken trak without tkhd, mdhd or a parsed entry: INVALID (the trak).
 *     The end of moov with no trak taken: NOT_CODEC, `codec` the first trak's entry fourcc.
 *   - the first `mvex` is read at moov's end, when the track is known: the first `trex` with track_id (shorter than 24 bytes: INVALID)
 *     gives default_sample_duration and default_sample_size; the first `mehd` (version 0 or 1, else INVALID) gives the duration when
 *     mdhd's is 0.
 *   - a stream with no mvex and no moof whose stsz counts samples is NOT_FRAGMENTED (error_offset: the moov): a file for ohgpu_mp4_*.
 *     Any other moov without a moof is OK with 0 samples: an initialisation segment alone.
 *   - moof: mfhd is skipped; every `traf` holds a `tfhd` (else INVALID, the traf) in front of its tfdt and trun boxes (else INVALID,
 *     that box).  tfhd flags: 0x1 base_data_offset (u64), 0x2 sample description index (skipped), 0x8 default duration, 0x10 default
 *     size, 0x20 default flags (skipped), 0x10000 (ignored), 0x20000 default-base-is-moof; a box too short for its flags: INVALID.  A
 *     traf of another track_id is skipped.  Neither 0x1 nor 0x20000 on a taken traf that is not the first traf of its moof:
 *     UNSUPPORTED (ISO then wants the end of the other track's data).  The first `tfdt` in front of the traf's first run (version 0:
 *     u32, 1: u64, else INVALID) gives that run's first frame.  Every `trun` with samples is one RUN: flags 0x1 data_offset (signed
 *     32), 0x4 first-sample flags (skipped); 0x100 duration, 0x200 size, 0x400 flags, 0x800 composition offset, each 4 bytes an entry
 *     in that order.  Entries that do not fit the box: INVALID.  A trun of 0 samples writes no row and is passed over.  A sample's
 *     size is the entry's, else tfhd's, else trex's, else INVALID (the trun); so is its duration.  More than OHGPU_MP4F_MAX_RUN_SAMPLES
 *     samples in a trun, or more than OHGPU_MP4F_MAX_SAMPLES in a stream: UNSUPPORTED (the trun).
 * Where a run's bytes lie: the base is tfhd's base_data_offset (beyond 2^62 it counts as 2^62) or else the moof's first byte; the run
 * starts at base + data_offset if the trun has one, else at the base if it is the traf's first run, else where the run in front of it
 * ends.  Its samples are contiguous.  Where its frames start: tfdt for the traf's first run, else where the run in front of it ended
 * (0 for the stream's first).  Frames are in mdhd's timescale, counted modulo 2^64.
 * The expansion, all sums in 64 bits: sample rows {first_frame, frames, chunk = the run's index} and packet rows {absolute offset in
 * the source arena, bytes}, the MPEG-4 section's types, so that ohgpu_alac_batch_create and ohgpu_mp4_seek take them unchanged.  A
 * sample whose bytes leave [0, src_bytes), or whose size is above the codec's limit (alac: frame_length x channels x 5 + 64; fLaC:
 * max_blocksize x channels x (bits / 8 + 1) + 64), is refused: its packet row is {the stream's src_offset, 0}.  Runs beyond
 * run_capacity and samples beyond packet_capacity (or in runs beyond run_capacity) are counted, not expanded.
 * The gather (OHGPU_MP4F_GATHER): the bytes of rows [gather_first_row, samples_available) go, in order and without gaps, to dst_offset
 * of the destination arena.  bytes_gathered is their sum; it is 0, and nothing is written, when that exceeds dst_capacity.  No other
 * destination byte is touched.
 * Where this differs from the reference (tests/mp4f_textbook.py carries the same list):
 *   - the reference plays a fragment only when its data begins right behind its moof (the three conditions at Mpeg4.cpp:4563-4568);
 *     here a run lies wherever its offsets say;
 *   - the reference ignores trex, tfdt and the entries' durations (Mpeg4BoxTrun::Process, Mpeg4.cpp:1499-1662, keeps sizes
 *     alone; no box of its table is tfdt or trex); here they
 *     give every sample its frames;
 *   - the reference refuses a trun of 0 samples (Mpeg4.cpp:1565-1567); here it is passed over;
 *   - the reference does not seek in a fragmented FLAC stream (the comment at Mpeg4.cpp:4778-4794); here the sample rows serve
 *     ohgpu_mp4_seek, and gather_first_row starts the run at the sample found;
 *   - the reference takes `sidx` for its seek table (Mpeg4BoxSidx::Process, Mpeg4.cpp:558-690); here sidx is skipped. */
#define OHGPU_MP4F_OK              0u
#define OHGPU_MP4F_NOT_MP4         1u
#define OHGPU_MP4F_TRUNCATED       2u
#define OHGPU_MP4F_INVALID         3u
#define OHGPU_MP4F_NOT_CODEC       4u
#define OHGPU_MP4F_UNSUPPORTED     5u
#define OHGPU_MP4F_NOT_FRAGMENTED  6u
#define OHGPU_MP4F_CODEC_ALAC      1u
#define OHGPU_MP4F_CODEC_FLAC      2u
#define OHGPU_MP4F_GATHER          1u
#define OHGPU_MP4F_MAX_BOXES       65536u
#define OHGPU_MP4F_MAX_SAMPLES     (1u << 24)
#define OHGPU_MP4F_MAX_RUN_SAMPLES (1u << 16)   /* 100 minutes of 4096-sample frames in one trun */
#define OHGPU_MP4F_ROUTE_PHASES    1u
#define OHGPU_MP4F_ROUTE_PLAIN     2u

typedef struct ohgpu_mp4f_stream_desc {   /* 64 bytes */
    uint64_t src_offset;            /* the stream's bytes are [src_offset, + src_bytes) of the source arena, any address */
    uint32_t src_bytes;             /* < 2^31: the initialisation segment and the media segments so far */
    uint32_t codecs;                /* OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC: the sample entries a trak is taken for */
    uint32_t flags;                 /* OHGPU_MP4F_GATHER */
    uint32_t packet_first;          /* the stream's rows are [packet_first, + packet_capacity) of both sample tables */
    uint32_t packet_capacity;
    uint32_t run_first;             /* ... and [run_first, + run_capacity) of the run table */
    uint32_t run_capacity;
    uint32_t gather_first_row;      /* GATHER: the first row whose bytes are gathered (a seek's row; 0: from the start) */
    uint64_t dst_offset;            /* GATHER: where the run goes in the destination arena, any address */
    uint64_t dst_capacity;          /* GATHER: the room there */
    uint32_t reserved[2];           /* zero */
} ohgpu_mp4f_stream_desc;

typedef struct ohgpu_mp4f_run {   /* 32 bytes: one row per trun that has samples */
    uint64_t data_offset;           /* its first byte, absolute in the source arena (src_offset + its place, modulo 2^64: a place may be negative) */
    uint64_t first_frame;
    uint32_t first_sample;          /* the stream's samples in front of it: its first row */
    uint32_t samples;
    uint64_t bytes;                 /* the sum of its samples' sizes */
} ohgpu_mp4f_run;

typedef struct ohgpu_mp4f_stream_result {   /* 168 bytes */
    uint32_t status;                /* OHGPU_MP4F_OK ... _NOT_FRAGMENTED */
    uint32_t codec;                 /* the taken trak's entry fourcc ('alac', 'fLaC'); NOT_CODEC: the first trak's */
    uint32_t track_id;              /* tkhd */
    uint32_t timescale;             /* mdhd */
    ohgpu_alac_config config;       /* 'alac': the inner box's; else 0 */
    ohgpu_flac_streaminfo_t flac;   /* 'fLaC': dfLa's STREAMINFO; else 0 */
    uint64_t duration;              /* mdhd's, or mehd's when that is 0; in timescale units */
    uint64_t frames;                /* the sum of every sample's duration */
    uint64_t samples;               /* of every run */
    uint32_t runs;                  /* truns with samples */
    uint32_t samples_available;     /* the leading rows that were not refused: what a prefix of a stream can play */
    uint32_t samples_refused;       /* rows refused */
    uint32_t first_bad_sample;      /* the lowest of them; OHGPU_MP4_NO_SAMPLE: none */
    uint32_t entry_rate;            /* the sample entry's: the upper 16 bits of its 16.16 rate */
    uint16_t entry_channels, entry_bits;
    uint64_t bytes_gathered;
    uint64_t moov_offset;           /* from src_offset */
    uint64_t first_moof_offset;     /* 0: none */
    uint64_t error_offset;          /* the box that gave a status other than OK */
} ohgpu_mp4f_stream_result;

/* Host only, no device needed: the validation ohgpu_mp4f_batch_create makes.  OHGPU_ERR_INVALID: non-zero reserved words, unknown
 * flags, a codecs mask of 0 or with unknown bits, src_bytes >= 2^31, row, run or gather ranges that overlap or (rows, runs) run past
 * their tables.  OHGPU_ERR_BOUNDS: a range outside its arena.  The empty batch is legal. */
int ohgpu_mp4f_batch_check(const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* The descriptors go to the device; the tiles, the records, the three tables (every byte 0xa5 that the LAST run did not write: a run
 * begins by filling them, so no row of an earlier run shows) and the results are the batch's.  Created under ohgpu_set_kernel_variant(1) the batch takes the plain route: one launch, a lane per stream does
 * everything serially, the gather included (ohgpu_mp4f_batch_paths).  Both routes write the same bytes.  Freed with ohgpu_batch_destroy. */
int ohgpu_mp4f_batch_create(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* Walk, run sums, carries, expand, finish, gather: queued on the stream, nothing waits for the host.  The source arena's rule is
 * ohgpu_mp4_batch_run's (src_base a multiple of 4, the allocation ends on one); dst_base may be NULL when no stream gathers.  The
 * batch owns its tables: it runs on one stream at a time.  A second run, and a second batch of the same shape, allocate nothing on
 * the device (ohgpu_device_allocations). */
int ohgpu_mp4f_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's results and tables (each waits for that run): n = the batch's stream count, n_runs / n_packets = the tables' length.
 * Of a stream's ranges the first min(runs, run_capacity) run rows and the first min(samples of those runs, packet_capacity) sample
 * and packet rows are that run's. */
int ohgpu_mp4f_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_stream_result* results, size_t n);
int ohgpu_mp4f_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs);
int ohgpu_mp4f_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets);
int ohgpu_mp4f_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets);
/* The last run's phases in milliseconds from device events: walk, run sums, carries, expand, finish, gather (waits for that run).
 * The plain route is one phase: the other five read as 0. */
int ohgpu_mp4f_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6]);
/* The route a batch was created onto (OHGPU_MP4F_ROUTE_*), the expansion's tiles and the workgroups of the two persistent launches
 * (0 on the plain route); the last two may be NULL. */
int ohgpu_mp4f_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks);
/* Host only, no device needed: the walk up to the end of `moov`, as if the stream ended there, with both codecs asked for -- what a
 * caller needs to route a stream and to fill its decoder's descriptor.  The result's status tells; the call itself fails only on a
 * null argument or n >= 2^31. */
int ohgpu_mp4f_head(const void* bytes, size_t n, ohgpu_mp4f_stream_result* result);
/* Host-buffer convenience: one upload, one run, the results and the tables home, and of dst_host the bytes that were gathered.  Any
 * of the four result pointers may be NULL; dst_host may be NULL when dst_bytes is 0. */
int ohgpu_mp4f_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, const void* src_host, uint64_t src_bytes,
                            void* dst_host, uint64_t dst_bytes, ohgpu_mp4f_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples);
/* Fragmented fLaC from host buffers to PCM: one upload, the demultiplexer gathering into a middle arena of mid_bytes that lives on the
 * device only, one small read of its results, a FLAC batch over the gathered runs (flac_descs[i].src_offset must be
 * mp4f_descs[i].dst_offset, an offset into the middle arena; its src_bytes is replaced by the stream's bytes_gathered -- 0 for a stream
 * that is not fLaC; OHGPU_FLAC_FLAG_AT_FRAME is the caller's to set), and of dst_host the samples that were decoded.  Any result
 * pointer may be NULL; frames as ohgpu_flac_batch_frames. */
int ohgpu_mp4f_flac_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* mp4f_descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_mp4f_stream_result* mp4f_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames);
/* Fragmented alac from host buffers to PCM, as ohgpu_mp4_alac_process_host: the packets are decoded where they lie (no stream may
 * gather); stream i's packets are its rows [0, samples_available), none for a stream that is not OK or not alac. */
int ohgpu_mp4f_alac_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* mp4f_descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_mp4f_stream_result* mp4f_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results);

/* ---- PCM files: WAV, AIFF and AIFC chunks walked and the audio made big-endian (the text is csrc/iff_chunk_core.h) ----
 * What CodecWav, CodecAiff and CodecAifc do: the bytes of a file, or of a prefix of one, in; the audio as the pipeline's big-endian
 * PCM out, with a result per stream.  Two launches, nothing waits for the host between them.
 * The first 12 bytes decide the kind: "RIFF" .... "WAVE", "FORM" .... "AIFF", "FORM" .... "AIFC"; anything else (fewer than 12 bytes
 * too) is NOT_IFF.  Chunks follow from byte 12: a four-character id, a 32-bit size (little-endian in RIFF, big-endian in FORM), the
 * payload, and one pad byte behind an odd size.  The walk takes the first `fmt ` and the first `data`, or the first `COMM` and the
 * first `SSND`, in either order, and stops when it has both; every other chunk, and a second one of those, is skipped by its size.
 * More than OHGPU_IFF_MAX_CHUNKS headers: INVALID.  The first thing wrong gives the status, error_offset is the chunk that gave it
 * (0 for NOT_IFF), and every other field of a refused stream reads 0.  The checks of a chunk are made in the order written here:
 *   - a chunk header (8 bytes) that the walk needs and that does not lie inside src_bytes: TRUNCATED, error_offset where it would lie.
 *   - `fmt `: size 16, 18 or 40, else INVALID; the payload not inside src_bytes: TRUNCATED.  Format tag 1 or 0xfffe, else UNSUPPORTED;
 *     a 0xfffe chunk of 40 bytes whose sub-format does not begin with the 16-bit word 1: UNSUPPORTED.  Channels 0: INVALID; above
 *     OHGPU_IFF_MAX_CHANNELS: UNSUPPORTED.  Rate 0 or byte rate 0: INVALID.  Depth 0 or no multiple of 8: INVALID; above 32:
 *     UNSUPPORTED.  A frame is channels x depth / 8 bytes (the block-align field is not read); bit_rate = byte rate x 8 (mod 2^32).
 *   - `data`: the audio is the chunk's stated size, without its pad byte.  A RIFF size field (bytes 4..8) of 0 means a continuous
 *     stream: the audio runs to the end of src_bytes, frames_total reads 0 ("unknown"), and a `data` in front of `fmt ` is INVALID
 *     (nothing can be found behind audio without an end).
 *   - `COMM`: exactly 18 bytes in AIFF, at least 22 in AIFC, else INVALID; the payload not inside src_bytes: TRUNCATED.  Channels u16
 *     (0: INVALID, above OHGPU_IFF_MAX_CHANNELS: UNSUPPORTED), sample frames u32, depth u16, the rate as an 80-bit extended number,
 *     in AIFC the compression's fourcc.  Depth 8, 16, 24 or 32 as is, 20 reported as 24, else UNSUPPORTED; a sample is ceil(depth / 8)
 *     bytes.  Rate: the sign is 0 and the exponent e lies in 0x3fff..0x401e, rate = (the mantissa's upper 32 bits) >> (0x401e - e),
 *     else INVALID; rate 0: INVALID; 22255 and 11127 (the Macintosh rates) read 22050 and 11025.  Compression "NONE" is big-endian,
 *     "sowt" and "SOWT" little-endian, anything else UNSUPPORTED.  bit_rate = rate x frame bytes x 8 (mod 2^32).
 *   - `SSND`: a payload of fewer than 8 bytes: INVALID; its 8-byte header (offset u32, block size u32) not inside src_bytes:
 *     TRUNCATED; offset > size - 8: INVALID.  The audio starts 8 + offset bytes into the payload.  When both chunks are known: sample
 *     frames x frame bytes more than the chunk holds behind that point: INVALID (error_offset: the SSND).
 *   - audio that runs past src_bytes is no error: frames_available counts the whole frames present, so a prefix of a file plays.
 * The conversion of an OK stream: frames [frame_first, frame_first + n) go to dst_offset as big-endian samples of out_bit_depth =
 * min(src_bit_depth, max_bit_depth) bits, n = min(frames_available - frame_first, dst_frame_capacity, dst_bytes_capacity / the output
 * frame's bytes), and 0 when frame_first lies behind the audio.  Each output sample is the top out_bit_depth / 8 bytes of the source
 * sample, most significant first: a 32-bit source under a limit of 24 loses its least significant byte.  8-bit WAV is copied as it
 * lies (the reference does); with OHGPU_IFF_FLAG_WAV8_UNSIGNED each byte is xor-ed with 0x80, which is what the format means.  No byte
 * of the destination outside the n frames is touched.
 * Where this differs from the reference (tests/iff_textbook.py carries the same list):
 *   - the reference streams, and wants `fmt ` before `data` and `COMM` before `SSND` (AiffBase.cpp has a FIXME of its own on it);
 *     here the bytes are there and either order is read;
 *   - CodecWav's chunk search returns the padded size, so an odd `data` size counts its pad byte as audio; here the stated size counts;
 *   - the reference does not look at an extensible format's sub-format; here one that is not PCM is UNSUPPORTED;
 *   - the reference takes a 20-bit AIFF sample for two bytes and then calls the stream 24-bit; here such a sample has three bytes;
 *   - the reference refuses 32-bit AIFF; here it is read as 32-bit WAV is;
 *   - the reference ignores SSND's offset field and holds the audio's size against the chunk's size with those 8 bytes in it; here
 *     both are honoured;
 *   - the reference's rate for exponents from 0x4013 up shifts by e - 0x4007, which is not the number the field encodes; here one
 *     formula serves every exponent;
 *   - OHGPU_IFF_FLAG_WAV8_UNSIGNED has no counterpart; without it the bytes are the reference's. */
#define OHGPU_IFF_OK           0u
#define OHGPU_IFF_NOT_IFF      1u
#define OHGPU_IFF_TRUNCATED    2u
#define OHGPU_IFF_INVALID      3u
#define OHGPU_IFF_UNSUPPORTED  4u
#define OHGPU_IFF_KIND_WAV     1u
#define OHGPU_IFF_KIND_AIFF    2u
#define OHGPU_IFF_KIND_AIFC    3u
#define OHGPU_IFF_MAX_CHUNKS   4096u
#define OHGPU_IFF_MAX_CHANNELS 10u
#define OHGPU_IFF_MAX_FRAME_BYTES 40u      /* OHGPU_IFF_MAX_CHANNELS x 4 */
#define OHGPU_IFF_FLAG_WAV8_UNSIGNED 1u    /* 8-bit WAV: xor every byte with 0x80 (unsigned to signed) */

typedef struct ohgpu_iff_stream_desc {   /* 64 bytes */
    uint64_t src_offset;            /* the file's bytes are [src_offset, + src_bytes) of the source arena, any address */
    uint32_t src_bytes;             /* < 2^31: the whole file or a prefix of it */
    uint32_t flags;                 /* OHGPU_IFF_FLAG_* */
    uint64_t dst_offset;            /* the PCM goes to [dst_offset, + n x the output frame's bytes) of the destination arena, any address */
    uint64_t dst_bytes_capacity;    /* the stream's room there, <= dst_frame_capacity x OHGPU_IFF_MAX_FRAME_BYTES: the frame's size is
                                       not known before the walk, so the caller states the room and the device keeps n inside it */
    uint64_t frame_first;           /* the first frame to convert (a seek) */
    uint32_t dst_frame_capacity;    /* frames at most */
    uint32_t max_bit_depth;         /* 24 or 32: iController->MaxBitDepth() */
    uint32_t reserved[4];           /* zero */
} ohgpu_iff_stream_desc;

typedef struct ohgpu_iff_stream_result {   /* 80 bytes */
    uint32_t status;                /* OHGPU_IFF_OK ... _UNSUPPORTED */
    uint32_t kind;                  /* OHGPU_IFF_KIND_* */
    uint32_t channels;
    uint32_t sample_rate;
    uint32_t src_bit_depth;         /* 8, 16, 24 (20 too) or 32 */
    uint32_t out_bit_depth;         /* min(src_bit_depth, max_bit_depth) */
    uint32_t src_endian;            /* OHGPU_ENDIAN_*: the file's */
    uint32_t bit_rate;
    uint64_t frames_total;          /* as the file states them; 0: a continuous stream */
    uint64_t frames_available;      /* whole frames inside src_bytes */
    uint64_t frames_written;        /* n */
    uint64_t data_offset;           /* the first audio byte, from src_offset */
    uint64_t data_bytes;            /* the audio as the file states it (a continuous stream: what there is) */
    uint64_t error_offset;          /* the chunk that gave a status other than OK, from src_offset */
} ohgpu_iff_stream_result;

/* Host only, no device needed: the validation ohgpu_iff_batch_create makes.  OHGPU_ERR_INVALID: non-zero reserved words, unknown flags,
 * max_bit_depth other than 24 or 32, src_bytes >= 2^31, dst_bytes_capacity above dst_frame_capacity x OHGPU_IFF_MAX_FRAME_BYTES,
 * destination ranges [dst_offset, + dst_bytes_capacity) that overlap.  OHGPU_ERR_BOUNDS: a range outside its arena.  The empty batch
 * is legal. */
int ohgpu_iff_batch_check(const ohgpu_iff_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* The descriptors go to the device; the list of the conversion's workgroups (from dst_bytes_capacity), the walk's records and the
 * results are the batch's.  Created under ohgpu_set_kernel_variant(1) the batch takes the plain route: one launch, a lane per stream
 * runs the walk and a byte-wise conversion (ohgpu_batch_paths_info: iff_route).  Both routes write the same bytes.  Freed with
 * ohgpu_batch_destroy. */
int ohgpu_iff_batch_create(ohgpu_ctx* ctx, const ohgpu_iff_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* Walk, convert: queued on the stream, nothing waits for the host.  The walk reads a stream as the aligned 4-byte words that hold its
 * bytes, as ohgpu_mp4_batch_run does: src_base must be a multiple of 4 and the arena's allocation must end on a multiple of 4 (any
 * hipMalloc block does).  The conversion loads only words that lie whole inside the stream and stores whole 16-byte lines of the
 * destination, with byte stores at a run's two ends.  The batch owns its records: it runs on one stream at a time.  A second run,
 * and a second batch of the same shape, allocate nothing on the device (ohgpu_device_allocations). */
int ohgpu_iff_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's results, n = the batch's stream count (waits for that run). */
int ohgpu_iff_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_iff_stream_result* results, size_t n);
/* The last run's phases in milliseconds from device events: walk, convert (waits for that run).  The plain route is one phase: the
 * second reads 0. */
int ohgpu_iff_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[2]);
/* Host-buffer convenience: one upload, one run, the results and, of dst_host, the frames_written frames of every OK stream home.
 * `results` may be NULL. */
int ohgpu_iff_process_host(ohgpu_ctx* ctx, const ohgpu_iff_stream_desc* descs, size_t n, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                           ohgpu_iff_stream_result* results);

/* ---- DSD files: DSF and DFF chunks walked and the audio packed into the pipeline's DSD format (the text is csrc/dsd_file_core.h) ----
 * What CodecDsdDsf and CodecDsdDff do in front of their packers: the bytes of a file, or of a prefix of one, in; the audio in the
 * pipeline's DSD format (the DSD section above) out, with a result per stream.  Two launches, nothing waits for the host between them.
 * The first 16 bytes decide the kind: bytes 0..4 "DSD " is DSF; bytes 0..4 "FRM8" with bytes 12..16 "DSD " is DFF; anything else, or
 * fewer than 16 bytes, is NOT_DSD.  The first thing wrong gives the status, error_offset is the chunk that gave it (0 for NOT_DSD), and
 * every other field of a refused stream reads 0.  A header the walk needs that does not lie inside src_bytes is TRUNCATED, error_offset
 * where it would lie.  The checks are made in the order written here.
 * DSF (little-endian; a chunk is an id, a u64 size that includes these 12 bytes, and its fields):
 *   - `DSD ` at 0 (28 bytes: id, size, the file's total size u64, the metadata pointer u64): its 28 bytes not inside src_bytes:
 *     TRUNCATED; size other than 28: INVALID; total file size 0: INVALID.  The metadata pointer is reported (metadata_offset) and not
 *     followed.
 *   - `fmt ` at 28, else INVALID; its size below 52 or 2^31 and above: INVALID; its 52 bytes not inside src_bytes: TRUNCATED.  The
 *     fields, all u32 but one: format version (reported), format id (0, else UNSUPPORTED), channel type (reported), channel count (2,
 *     else UNSUPPORTED), sampling rate (0: INVALID), bits per sample (1, else UNSUPPORTED: 8 means a file whose bytes are MSB first,
 *     DESIGN.md 8), sample count per channel (u64), block size per channel (4096, else UNSUPPORTED), four reserved bytes.
 *   - `data` at 28 + the `fmt ` size, else INVALID; a size below 12: INVALID.  The audio bytes are the size less 12: odd: INVALID;
 *     2 x floor(sample_count / 8) above them: INVALID.  The audio is pairs of 4096-byte planes, left then right.
 *   - chunks_total = floor(sample_count / 16) (what DsdDsf.cpp:408-414 and :203 amount to).
 * DFF (big-endian; a chunk is an id, a u64 size, the payload, and one pad byte behind an odd size):
 *   - chunks are walked from byte 16.  More than OHGPU_DSD_FILE_MAX_CHUNKS headers, the local ones of a `PROP` counted: INVALID.  A
 *     size of 2^63 or more: INVALID.  The walk takes the first `PROP` whose type is `SND ` and the first `DSD ` chunk, in either
 *     order, and stops when it has both; everything else is skipped by its size.
 *   - `FVER`, when met: size other than 4: INVALID; its payload not inside src_bytes: TRUNCATED; first byte other than 1: UNSUPPORTED;
 *     its four bytes are format_version.
 *   - `DST ` met before `DSD `: UNSUPPORTED.
 *   - `PROP`: size below 4: INVALID; its payload not inside src_bytes: TRUNCATED.  One of another type than `SND ` is skipped.  Local
 *     chunks follow its type: one that runs past the `PROP`: INVALID.  `FS  `: size 4, the rate, else INVALID; rate 0: INVALID.
 *     `CHNL`: at least 2 bytes, else INVALID; a u16 count: 2, else UNSUPPORTED.  `CMPR`: at least 4 bytes, else INVALID; the fourcc
 *     `DSD `, else UNSUPPORTED.  Others are skipped.  No `FS  ` or no `CHNL`: INVALID.  error_offset is the `PROP`.
 *   - `DSD `: the audio is its stated size, bytes L R L R; odd: INVALID.  chunks_total = floor(size / 4), sample_count = 16 x that.
 * Audio past src_bytes is no error: chunks_available counts the chunks below chunks_total whose four source bytes all lie inside
 * src_bytes -- for DSF chunk j = 2048 q + r those at data_offset + 8192 q + 2 r, the next one, and the same two 4096 further on -- so a
 * prefix of a file plays.
 * The conversion of an OK stream: chunks [chunk_first, chunk_first + n) go to dst_offset in the pipeline's format for the descriptor's
 * (W, P), the bytes exactly those an ohgpu_dsd_desc of kind OHGPU_DSD_DSF / OHGPU_DSD_DFF defines for those chunks.  With cpb = W * 4 /
 * (4 + P) and room = floor(dst_bytes_capacity / (W * 4)) * cpb, n = min(chunks_available - chunk_first, room), or 0 when chunk_first
 * lies behind the available chunks.  If the n chunks reach chunks_total, a last partial block is filled with 0x69 up to its end (the
 * DSD section's rule, and its deliberate difference from the reference: the leftover chunks are converted); if they do not, n is
 * rounded down to whole blocks.  bytes_written counts the fill.  No destination byte outside bytes_written is touched.
 * Where this differs from the reference (tests/dsd_file_textbook.py carries the same list):
 *   - the reference streams and wants DFF's chunks in its own order (FVER, PROP, DSD); here the bytes are there, `PROP` and `DSD ` are
 *     read in either order and everything else is skipped by its size;
 *   - the reference does not skip the pad byte behind an odd DFF chunk; here it is honoured;
 *   - the reference does not look at `CMPR`, plays a `DST ` file's frames it never finds, and ignores DSF's format id and bits per
 *     sample; here they are looked at and refused, instead of played as noise;
 *   - the reference refuses a DSF channel count other than 2 as corrupt and takes DFF's as it comes; here both kinds are stereo and
 *     any other count is UNSUPPORTED;
 *   - the reference does not hold DSF's sample count against the `data` chunk's size; here a count the chunk cannot hold is INVALID. */
#define OHGPU_DSD_FILE_OK           0u
#define OHGPU_DSD_FILE_NOT_DSD      1u
#define OHGPU_DSD_FILE_TRUNCATED    2u
#define OHGPU_DSD_FILE_INVALID      3u
#define OHGPU_DSD_FILE_UNSUPPORTED  4u
#define OHGPU_DSD_FILE_KIND_DSF     2u     /* = OHGPU_DSD_DSF */
#define OHGPU_DSD_FILE_KIND_DFF     3u     /* = OHGPU_DSD_DFF */
#define OHGPU_DSD_FILE_MAX_CHUNKS   4096u

typedef struct ohgpu_dsd_file_stream_desc {   /* 64 bytes */
    uint64_t src_offset;            /* the file's bytes are [src_offset, + src_bytes) of the source arena, any address */
    uint32_t src_bytes;             /* < 2^31: the whole file or a prefix of it */
    uint32_t flags;                 /* zero */
    uint64_t dst_offset;            /* a multiple of 16: the sample blocks go to [dst_offset, + bytes_written) of the destination arena */
    uint64_t dst_bytes_capacity;    /* the stream's room there */
    uint64_t chunk_first;           /* the first chunk to convert (a seek) */
    uint32_t sample_block_words;    /* W  } validated as for ohgpu_dsd_desc */
    uint32_t pad_bytes_per_chunk;   /* P  }                                 */
    uint32_t reserved[4];           /* zero */
} ohgpu_dsd_file_stream_desc;

typedef struct ohgpu_dsd_file_stream_result {   /* 96 bytes */
    uint32_t status;                /* OHGPU_DSD_FILE_OK ... _UNSUPPORTED */
    uint32_t kind;                  /* OHGPU_DSD_FILE_KIND_* */
    uint32_t channels;              /* 2 */
    uint32_t sample_rate;           /* one-bit samples a second and channel */
    uint32_t format_version;        /* DSF: the `fmt ` field; DFF: FVER's four bytes, 0 when the walk met none */
    uint32_t channel_type;          /* DSF: the `fmt ` field; DFF: 0 */
    uint64_t sample_count;          /* a channel's one-bit samples: DSF as the file states them, DFF 16 x chunks_total */
    uint64_t chunks_total;          /* chunks of sixteen samples a channel */
    uint64_t chunks_available;      /* those whose source bytes lie inside src_bytes */
    uint64_t chunks_written;        /* n */
    uint64_t bytes_written;         /* whole sample blocks, the 0x69 fill counted */
    uint64_t data_offset;           /* the first audio byte, from src_offset */
    uint64_t data_bytes;            /* the audio as the file states it */
    uint64_t metadata_offset;       /* DSF: the metadata pointer (0: none); DFF: 0 */
    uint64_t error_offset;          /* the chunk that gave a status other than OK, from src_offset */
} ohgpu_dsd_file_stream_result;

/* Host only, no device needed: the validation ohgpu_dsd_file_batch_create makes.  OHGPU_ERR_INVALID: non-zero reserved words or flags,
 * a (W, P) that ohgpu_dsd_desc refuses, src_bytes >= 2^31, a dst_offset that is no multiple of 16, destination ranges [dst_offset,
 * + dst_bytes_capacity) that overlap.  OHGPU_ERR_BOUNDS: a range outside its arena.  The empty batch is legal. */
int ohgpu_dsd_file_batch_check(const ohgpu_dsd_file_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes);
/* The descriptors go to the device; the list of the conversion's workgroups (from dst_bytes_capacity alone), the walk's records and
 * the results are the batch's.  Created under ohgpu_set_kernel_variant(1) the batch takes the plain route: one launch, a lane per
 * stream runs the walk and a byte-wise conversion (ohgpu_batch_paths_info: dsd_file_route).  Both routes write the same bytes.  Freed
 * with ohgpu_batch_destroy. */
int ohgpu_dsd_file_batch_create(ohgpu_ctx* ctx, const ohgpu_dsd_file_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes,
                                ohgpu_batch** batch);
/* Walk, convert: queued on the stream, nothing waits for the host.  The walk reads a stream as the aligned 4-byte words that hold its
 * bytes, as ohgpu_iff_batch_run does: src_base must be a multiple of 4 and the arena's allocation must end on a multiple of 4 (any
 * hipMalloc block does).  The conversion takes the audio at any address: a lane loads the aligned 16-byte lines that cover its eight
 * chunks, only lines that lie whole inside the stream, and stores whole 16-byte lines (dst_base a multiple of 16, as ohgpu_malloc's
 * are; otherwise, and for P above 4, it goes byte by byte).  The batch owns its records: it runs on one stream at a time.  A second
 * run, and a second batch of the same shape, allocate nothing on the device (ohgpu_device_allocations). */
int ohgpu_dsd_file_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The last run's results, n = the batch's stream count (waits for that run). */
int ohgpu_dsd_file_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_dsd_file_stream_result* results, size_t n);
/* The last run's phases in milliseconds from device events: walk, convert (waits for that run).  The plain route is one phase: the
 * second reads 0. */
int ohgpu_dsd_file_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[2]);
/* Host-buffer convenience: one upload, one run, the results and, of dst_host, the bytes_written bytes of every OK stream home.
 * `results` may be NULL. */
int ohgpu_dsd_file_process_host(ohgpu_ctx* ctx, const ohgpu_dsd_file_stream_desc* descs, size_t n, const void* src_host, uint64_t src_bytes,
                                void* dst_host, uint64_t dst_bytes, ohgpu_dsd_file_stream_result* results);
/* Host only, no device needed: the walk over `n` bytes of a file (or of a prefix) -- the same core, and the record the device's walk
 * gives for chunk_first 0 and unlimited room under (W, P): chunks_written = chunks_available, rounded down to whole blocks where they
 * do not reach chunks_total.  OHGPU_ERR_INVALID for a null argument, n >= 2^31 or a (W, P) that ohgpu_dsd_desc refuses. */
int ohgpu_dsd_file_head(const void* bytes, uint64_t n, uint32_t sample_block_words, uint32_t pad_bytes_per_chunk, ohgpu_dsd_file_stream_result* result);
/* Host only: where a seek to `sample` lands, by the reference's rounding -- DSF: sample & ~(32768 - 1) (DsdDsf.cpp's block pairs);
 * DFF: sample & ~(2048 - 1) --, and chunk_first = sample_rounded / 16.  OHGPU_ERR_INVALID for another kind or a null result. */
int ohgpu_dsd_file_seek(uint32_t kind, uint64_t sample, uint64_t* chunk_first, uint64_t* sample_rounded);

/* ---- sample-rate converter (own specification; DESIGN.md "Resampler") ---- */
/* Host-side filter design: Kaiser-windowed sinc, Q28 coefficients, coef_q28[p*T + k] = h[p + k*L].
 * Stop edge f_stop = rate_out - f_pass, or rate_in - f_pass from 2x upsampling on (rate_out >= 2 * rate_in: the pass band's images,
 * not the output's alias, set it -- at exactly 2x the output's rule would put the cutoff at the input rate); cutoff midway; DESIGN.md 4.
 * Pass coef_q28 = NULL to query L, M only.  Capacity must be >= L*T. */
int ohgpu_src_design(uint32_t rate_in, uint32_t rate_out, uint32_t taps_per_phase, double beta, double f_pass_hz,
                     int32_t* coef_q28, size_t coef_capacity, uint32_t* L, uint32_t* M);
int ohgpu_src_create(ohgpu_ctx* ctx, uint32_t L, uint32_t M, uint32_t taps_per_phase, const int32_t* coef_q28, ohgpu_src** src);
int ohgpu_src_destroy(ohgpu_ctx* ctx, ohgpu_src* src);
/* ceil(in_frames * L / M): output frames available once in_frames input frames have arrived */
uint64_t ohgpu_src_out_frames(uint32_t L, uint32_t M, uint64_t in_frames);
/* Host only, no device needed: the tables ohgpu_src_create makes for the matrix-pipe resampler kernel (24-bit stereo,
 * ohpipeline_amd/csrc/src_mfma_kernel.hip) -- the coefficients' balanced base-256 digits as padded rows
 * [4 digits][L][96] bytes, and one 288-byte record per 16-output step of a block row (A-row offsets, the accumulators'
 * initial values, the window's first 16-frame chunk).  *block_outputs = outputs per block; steps cover rows of up to
 * max_blocks_per_row blocks.  Query sizes with NULL buffers.  OHGPU_ERR_UNSUPPORTED when the filter does not fit the
 * tiling (taps_per_phase != 32, or a ratio whose 16-output tiles need more than 64 input frames).  Tests check the
 * tables against the integer model on the CPU; the kernel is checked on the device. */
int ohgpu_src_mfma_tables(uint32_t L, uint32_t M, uint32_t taps_per_phase, const int32_t* coef_q28, uint32_t max_blocks_per_row,
                          uint8_t* coef_digits, size_t coef_digits_capacity, void* steps, size_t steps_capacity,
                          size_t* coef_digits_bytes, size_t* steps_bytes, uint32_t* block_outputs);
/* ... and the tables it makes for the same kernel's half-band form (ohpipeline_amd/csrc/src_mfma_wg_kernel.hip, HB) when the
 * filter is a 2:1 decimator of 64 stored taps whose odd taps but the centre one (31) are zero: ONE image of the B operand's
 * coefficient digits, [4 digits][lane = 16 g + n][16 bytes] -- K groups g = 0..2 meet the even input frames 16 (s + g) .. + 15 of
 * step s (a row's image starts 64 frames before its block), group 3 the odd frames 16 (s + 1) .. + 15, output n taking sample n --
 * and the accumulators' initial value 32896 * sum(c) + 2^27.  *block_outputs = outputs per block (128).
 * OHGPU_ERR_UNSUPPORTED when the coefficients are not such a filter.  Host only. */
int ohgpu_src_mfma_halfband_tables(const int32_t* coef_q28 /* 64 */, uint8_t* image /* 4096 bytes */, int64_t* bias, uint32_t* block_outputs);
/* The messages of one batch may differ in layout (channels, depths, byte orders, packed or planar source): the batch is
 * planned per layout and runs one launch sequence per layout, messages of a stream in the order given.
 * What a batch keeps: its plan (a record per unit of 30-32 blocks, per ramped message and unit, per block-unaligned message end) on
 * the device and a copy of the ramp records on the host -- nothing per message, unless it is the generic kernel's batch (created
 * while ohgpu_set_kernel_variant(1) is in force, or of a layout no block kernel has: 56 bytes a message on the host, and on the
 * device from its first run). */
int ohgpu_src_batch_create(ohgpu_ctx* ctx, const ohgpu_src* src, const ohgpu_src_msg_desc* descs, size_t n,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
/* A batch may be run any number of times, one launch at a time (it owns device-side work counters): launches of the same
 * batch on one stream queue behind each other; a launch on ANOTHER stream while the previous one has not finished returns
 * OHGPU_ERR_INVALID (nothing is launched).  Different batches are independent.  The same holds for
 * ohgpu_flywheel_batch_run (the batch owns Burg's workspace).
 * The decoders' and demultiplexers' batches (ohgpu_flac_, _alac_, _raop_, _ohm_rx_, _ogg_, _mp4_ and _iff_batch_run) keep records of
 * their own -- counters, candidate and piece lists, tables, results, scratch -- which serve ONE RUN AT A TIME too, but these runs never
 * refuse a stream: a run on another stream than the batch's last run first WAITS ON THE HOST for that run, then proceeds.  It waits on
 * what the batch itself recorded at that run's end, never on the earlier stream, which may have been synchronised and destroyed by
 * then.  Runs on one stream queue behind each other without a wait; the results and tables are those of the last run. */
int ohgpu_src_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* The same with two events of the caller's (ohgpu_event_create) that bracket the batch's device work on `stream`: a batch that is one
 * launch of the workgroup matrix kernel carries them ON ITS DISPATCH (hipExtLaunchKernelGGL: the dispatch's own start and end
 * timestamps, no packet more in the queue -- two ohgpu_event_record calls around every launch cost a benchmark's back-to-back launches
 * 5 us each, 1.7 % of the headline's); any other batch gets them recorded in front of its first launch and behind its last.
 * ohgpu_event_elapsed_ms(start, stop) is the batch's device time either way.  A measurement's tool (bench.py's roofline): the audio
 * is ohgpu_src_batch_run's. */
int ohgpu_src_batch_run_timed(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream,
                              void* start_event, void* stop_event);

/* ---- the same batch, the next period ----
 * A caller that brings new audio every period in the same shape -- the same streams, the same tiling into messages, a whole number
 * of blocks further on in every stream -- need not plan again:
 *   - other arena positions: pass other base pointers to ohgpu_src_batch_run (the source's 16-byte aligned);
 *   - further on in the streams: ohgpu_src_batch_advance.  Every message's out_frame0 grows by blocks * block_outputs and its
 *     src_frame0 by blocks * block_inputs (ohgpu_src_batch_block), offsets and windows as they were: the plan names no absolute
 *     position (a unit is where its rows lie in the arenas, a ramp job where its frames lie in its message), and a whole number of
 *     blocks later every message has the phase it had -- so the call checks that this is such a batch and changes nothing.
 *     OHGPU_ERR_INVALID for a batch that holds a stream's first message (its window is zeros where the next period's is history),
 *     OHGPU_ERR_UNSUPPORTED for one without a block-kernel plan;
 *   - other ramp endpoints (the flags stay: which messages are ramped is the plan's shape): ohgpu_src_batch_set_ramps, one pair per
 *     message in the batch's order (those of unramped messages are not looked at).  Every ramped message's pair is checked first:
 *     OHGPU_ERR_INVALID for an endpoint beyond OHGPU_RAMP_MAX, and a refused call changes nothing.  Then, after the batch's last
 *     launch, it rewrites wherever the plan keeps the endpoints -- the ramp jobs (and refills the multiplier planes), the
 *     generic-kernel pieces, round 1's per-message records (src_block_kernel), the generic kernel's per-message descriptors (a batch
 *     created under kernel variant 1 or without a block-kernel plan).  Not for a batch of several layouts (OHGPU_ERR_UNSUPPORTED).
 * Anything else -- another tiling, other flags, other streams -- is another batch.  tests/test_plan_threads.py holds the plan of a
 * shifted period to the digest of the period it was made for; tests/test_gpu_parity.py runs both calls against the oracle,
 * tests/test_gpu_src_textbook.py on every plan kind against the textbook model. */
int ohgpu_src_batch_block(const ohgpu_batch* batch, uint32_t* block_outputs, uint32_t* block_inputs);
int ohgpu_src_batch_advance(ohgpu_ctx* ctx, ohgpu_batch* batch, uint64_t blocks);
int ohgpu_src_batch_set_ramps(ohgpu_ctx* ctx, ohgpu_batch* batch, const uint16_t* ramp_start, const uint16_t* ramp_end, size_t n);

/* Host-buffer convenience (a live pipeline's 5 ms cadence): H2D, run, D2H, sync, as ohgpu_pcm_process_host.  dst_host bytes
 * that no message covers are preserved.  src_host need only hold each message's WINDOW (ohgpu_src_msg_desc: src_frame0 /
 * src_frames), not the stream's history: host/SampleRateConverter.cpp packs the windows of a period's messages back to back. */
int ohgpu_src_process_host(ohgpu_ctx* ctx, const ohgpu_src* src, const ohgpu_src_msg_desc* descs, size_t n,
                           const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes);

/* ---- pulled resampler (own specification; DESIGN.md 4b "Pulled resampling") ----
 * The stand-in for IPullableClock::PullClock (ClockPuller.h:17-34) when one device serves many streams against one output clock:
 * instead of pulling a DAC, each stream's resampling ratio follows its own clock controller, message by message.  One prototype
 * (Kaiser-windowed sinc, P = 2^phases_log2 phases per input frame, T taps per phase) serves every ratio near rate_in -> rate_out;
 * a message carries its own position and step:
 *   output j of a message:  u = pos_frac + j * step (64 bits),  n = pos_frame + (u >> 32),  f = u & 0xffffffff,
 *                           p = f >> (32 - s),  w = (f >> (16 - s)) & 0xffff,
 *                           c_k = C[p][k] + (((C[p+1][k] - C[p][k]) * w) >> 16),
 *                           y = clamp_s24((sum_k c_k * x[n - k] + 2^27) >> 28)   (x: S24, frames before the stream start are 0)
 * then RampApplicator's 24-bit case and the pack, as for ohgpu_src_msg_desc.  Splitting a message after k outputs gives a
 * message at pos + k * step (the carry goes into pos_frame) whose bytes equal the tail of the unsplit one's. */
#define OHGPU_SRC_PULL_NOMINAL     (1u << 31)            /* IPullableClock::kNominalFreq: multiplier 1.0 in fix 1.31 */
#define OHGPU_SRC_PULL_MAX_STEP    (16ull << 32)         /* at most 16 input frames per output frame (Q32.32) */

/* One OUTPUT message of a pulled stream.  80 bytes.  The fields of ohgpu_src_msg_desc, with out_frame0 replaced by the
 * message's position (pos_frame + pos_frac / 2^32 input frames) and its step (Q32.32 input frames per output frame).  The input
 * buffer rules are ohgpu_src_msg_desc's: ohgpu_src_pull_window gives the frames a message reads. */
typedef struct ohgpu_src_pull_msg_desc {
    uint64_t src_offset;    /* bytes from src_base to input frame src_frame0                        */
    uint64_t src_frame0;    /* absolute index of the first input frame held in the buffer           */
    uint64_t src_frames;    /* number of input frames held                                          */
    uint64_t pos_frame;     /* integer part of output 0's input position                            */
    uint64_t step;          /* Q32.32 input frames per output frame, 1 .. OHGPU_SRC_PULL_MAX_STEP   */
    uint64_t dst_offset;    /* bytes from dst_base                                                  */
    uint32_t pos_frac;      /* fractional part of output 0's input position, units of 2^-32         */
    uint32_t n_frames;      /* output frames in this message                                        */
    uint16_t ramp_start;
    uint16_t ramp_end;
    uint16_t attenuation;   /* must be 256                                                          */
    uint8_t  channels;      /* 1..8                                                                 */
    uint8_t  src_bits;      /* 8, 16, 24, 32 packed                                                 */
    uint8_t  src_endian;
    uint8_t  dst_bits;      /* 16, 24, 32                                                           */
    uint8_t  dst_endian;
    uint8_t  flags;         /* OHGPU_FLAG_RAMP | OHGPU_FLAG_ZERO_LSB32                              */
    uint8_t  reserved[4];   /* zero                                                                 */
    uint64_t src_plane_stride; /* 0 (planar sources are not supported on the pulled path)          */
} ohgpu_src_pull_msg_desc;

/* Host only.  The Q28 table of (P + 1) rows of T, P = 2^phases_log2, from the prototype h[n], n = 0 .. T*P - 1: for p < P,
 * coef_q28[p*T + k] = round(h[p + k*P] / g_p * 2^28) with g_p = sum_k h[p + k*P] (each row scaled to DC gain 1 on its own, so it sums
 * to 2^28 within T / 2); row P is row 0 moved on one tap (coef_q28[P*T + k] = coef_q28[k + 1], the last 0: h[T*P] = 0).  The band
 * edges (f_stop = rate_out - f_pass, or rate_in - f_pass from 2x upsampling on; cutoff midway) hold for every input
 * rate in rate_in * [1 - max_pull, 1 + max_pull].  OHGPU_ERR_INVALID for phases_log2 outside 1 .. 16, taps_per_phase other than 32
 * or 64, a pass band that meets the stop band, a table beyond the exact-accumulation bound, or a capacity below (P + 1) * T. */
int ohgpu_src_pull_design(uint32_t rate_in, uint32_t rate_out, uint32_t taps_per_phase, uint32_t phases_log2, double beta,
                          double f_pass_hz, double max_pull, int32_t* coef_q28, size_t coef_capacity);
/* Host only.  step = floor(2 * rate_in * multiplier / rate_out): multiplier in fix 1.31 (OHGPU_SRC_PULL_NOMINAL = 1.0); above
 * nominal consumes input faster.  OHGPU_ERR_INVALID for a zero rate, or a step that is zero or beyond OHGPU_SRC_PULL_MAX_STEP. */
int ohgpu_src_pull_step(uint32_t rate_in, uint32_t rate_out, uint32_t multiplier, uint64_t* step);
/* Host only.  The input frames [first, first + frames) a message of n_frames outputs reads (first clamped at the stream start).
 * OHGPU_ERR_INVALID for n_frames == 0, a bad step, or n_frames * step overflowing. */
int ohgpu_src_pull_window(uint64_t pos_frame, uint32_t pos_frac, uint64_t step, uint32_t n_frames, uint32_t taps_per_phase,
                          uint64_t* first, uint64_t* frames);
/* The table on the device.  OHGPU_ERR_UNSUPPORTED for a table that does not fit the kernel's LDS (up to 2^8 phases, T = 32 or
 * 64); OHGPU_ERR_INVALID as ohgpu_src_pull_design refuses.  A pulled filter is for the calls below only:
 * ohgpu_src_batch_create refuses it, and these refuse a fixed-ratio filter (OHGPU_ERR_INVALID). */
int ohgpu_src_pull_create(ohgpu_ctx* ctx, uint32_t taps_per_phase, uint32_t phases_log2, const int32_t* coef_q28, ohgpu_src** src);
int ohgpu_src_pull_destroy(ohgpu_ctx* ctx, ohgpu_src* src);
/* Validated like ohgpu_src_batch_create (OHGPU_ERR_BOUNDS / _INVALID / _UNSUPPORTED, nothing kept on a refusal); freed with
 * ohgpu_batch_destroy; ohgpu_batch_info counts its messages.  The batch holds no per-launch device state: it may be run any
 * number of times, on any stream. */
int ohgpu_src_pull_batch_create(ohgpu_ctx* ctx, const ohgpu_src* src, const ohgpu_src_pull_msg_desc* descs, size_t n,
                                uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** batch);
int ohgpu_src_pull_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream);
/* Host-buffer convenience, as ohgpu_src_process_host (the context's arenas and staging; nothing allocated in a steady state). */
int ohgpu_src_pull_process_host(ohgpu_ctx* ctx, const ohgpu_src* src, const ohgpu_src_pull_msg_desc* descs, size_t n,
                                const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes);

/* What the *_process_host calls of this context have moved so far: their number, how many of them were ohgpu_src_process_host,
 * or ohgpu_src_pull_process_host, and the bytes copied to and from the device for audio (descriptors and plans not counted).  A driver's handle on "one call per
 * filter per period, windows only" (tests/cpp/test_host.cpp, bench.py's cadence.adapter). */
int ohgpu_host_transfer_stats(ohgpu_ctx* ctx, uint64_t* calls, uint64_t* src_calls, uint64_t* h2d_bytes, uint64_t* d2h_bytes);

/* How a resampler batch was planned: output frames handled by the block kernel, and the number of message pieces
 * (block-unaligned heads/tails, unsupported layouts) left to the generic kernel. */
int ohgpu_src_batch_plan(const ohgpu_batch* batch, uint64_t* block_kernel_out_frames, uint64_t* generic_pieces);

/* ... and how the block kernel's share was cut: its work units, and how many of them are "long" (every row several
 * consecutive blocks of its stream: the unit schedule of large batches, ohpipeline_amd/csrc/src_plan.cpp).  Both 0 when the
 * batch runs on the generic kernel alone. */
int ohgpu_src_batch_units(const ohgpu_batch* batch, uint64_t* units, uint64_t* long_units);

/* Planning is host work, done per batch: the descriptors are independent per message and per stream, so the library checks them
 * and cuts the streams into work units on several threads (up to 16, by the size of the batch).  `threads` caps that number for
 * every later ohgpu_*_batch_create of the process (1: the calling thread alone; 0: no cap, the default).  The plan does not depend
 * on it. */
int ohgpu_set_plan_threads(int threads);

/* The plan ohgpu_src_batch_create would make for these messages, as a 64-bit hash of its unit list, ramp jobs and generic-kernel
 * pieces -- computed on the host alone (no context, no device): what tests/test_plan_threads.py compares across thread counts.
 * coef_q28 (L * taps_per_phase of them) describes the filter as ohgpu_src_create would -- the half-band form, the matrix kernels'
 * tables, the gain bound -- so that the plan is the one a real batch gets; NULL stands for a polyphase filter of sane gain with
 * no special structure.  num_cus is the device's CU count (the long-unit schedule aims at one long unit per wave): 0 = 256.
 * `kernel` is set to the newest kernel the plan serves: 3 / 1 / 0 for src_mfma_wg_kernel / src_lean_kernel / round 1's fallback or
 * none; which one runs is the run-time variant's choice among those.  kernel_variant is read as ohgpu_set_kernel_variant reads it
 * (2 and 5 are 4). */
int ohgpu_src_plan_digest(uint32_t L, uint32_t M, uint32_t taps_per_phase, const ohgpu_src_msg_desc* descs, size_t n,
                          uint64_t src_arena_bytes, uint64_t dst_arena_bytes, int kernel_variant,
                          const int32_t* coef_q28, int num_cus,
                          uint64_t* digest, uint64_t* units, uint64_t* generic_pieces, int* kernel);

/* Which kernel ohgpu_src_batch_run launches for the batch's whole phase-aligned blocks under the context's current kernel
 * variant: "src_mfma_wg_kernel", "src_lean_kernel", "src_block_kernel" (round 1's: the fallback for a filter whose phase sums reach
 * 2^29, beyond the lean kernel's exact rounding -- five stereo layouts) or "src_kernel_v1" (the generic one alone); a batch of several layouts names its parts' kernels, comma separated.  A measurement's label (bench.py), nothing the
 * data path depends on.  The name is written to out[0, cap) NUL-terminated (truncated if it does not fit). */
int ohgpu_src_batch_kernel_name(ohgpu_ctx* ctx, const ohgpu_batch* batch, char* out, size_t cap);

/* How many workgroups of the batch's resampler kernel the device keeps on a CU at once (hipOccupancyMaxActiveBlocksPerMultiprocessor
 * of the instantiation the batch runs, with its LDS), how many its geometry was laid out for, and its LDS bytes per workgroup.  The
 * workgroup matrix kernel is sized to the LDS: three workgroups per CU at 50.7-52.0 KB each (csrc/src_mfma_wg_kernel.hip WgGeom);
 * one granule more and the device would keep two, a third of the throughput gone without an error anywhere -- tests/test_gpu_parity.py
 * holds every layout to its design.  OHGPU_ERR_UNSUPPORTED for a batch that runs on another kernel; nothing is launched.  (A
 * diagnostic like ohgpu_measure_shader_clock: no reference interface behind it.) */
int ohgpu_src_batch_occupancy(ohgpu_ctx* ctx, const ohgpu_batch* batch, int* workgroups_per_cu, int* designed_for, uint32_t* lds_bytes);

/* The shader clock the device holds right now, in MHz: a short kernel on every CU (about 0.2 ms of dependent vector work,
 * queued on `stream` like any launch) compares the shader cycle counter (s_memtime) with the constant 100 MHz reference counter
 * (s_memrealtime) and the call waits for it.  For a benchmark to report next to a kernel time, so that a slow box can be told
 * from a slow build; it touches no audio buffer. */
int ohgpu_measure_shader_clock(ohgpu_ctx* ctx, void* stream, double* mhz);

/* How many device allocations (hipMalloc) the context has made for batches' descriptors and plan arrays since ohgpu_init.  A
 * destroyed batch's blocks stay with the context and serve the next batch of that size, so a caller in a steady state -- the
 * StarvationRamper's rescue creates three batches per starving period (reference: StarvationRamper.cpp:560-620 does that work on
 * the CPU, inside the period) -- sees this number stop growing; a test's handle on "nothing is allocated in the period". */
int ohgpu_device_allocations(ohgpu_ctx* ctx, uint64_t* count);

/* Kernel selection for A/B measurement and tests: 0 = default/best; 1 = baseline "v1" kernels (a resampled batch must be CREATED under
 * 1 to run under it: only then does it keep the generic kernel's per-message form); 3 = the default kernels with the resampler's
 * long-row unit schedule forced onto batches of any size (a resampled batch created while 3 is set cuts every run of plain units
 * into rows of three blocks -- what only a batch of thousands of units gets otherwise -- so that tests reach that path with small
 * inputs; results are identical); 4 = round 2's fp64 "lean" block kernel where round 4's matrix-pipe kernel would run, for A/B.
 * 2 and 5 are accepted as aliases of 4 (they once selected round 1's block kernel and round 4's unit-per-wave matrix kernel, which
 * the library no longer has as selectable kernels).  (Round 1's kernel stays in the library for five stereo layouts as the fallback
 * for filters beyond the lean kernel's rounding bound, whatever the variant.)  Variants 3 and 4 shape the plan of batches created
 * while they are set; the variant in force when a batch is RUN
 * chooses among the kernels its plan serves (ohgpu_src_batch_kernel_name says which).  A batch planned for the workgroup kernel
 * alone (six and eight channels, the layouts only it has) is REFUSED under any other variant (OHGPU_ERR_UNSUPPORTED, nothing is
 * launched): create it under the variant it is to run under. */
int ohgpu_set_kernel_variant(ohgpu_ctx* ctx, int variant);

#ifdef __cplusplus
}
#endif

/* Protected fragmented MPEG-4 (ohgpu_cenc_*) has a header of its own beside this one; it comes with this one. */
#include "ohgpu_cenc.h"
#include "ohgpu_raop_rx.h"
#include "ohgpu_ts.h"
#include "ohgpu_vorbis.h"
#include "ohgpu_cbcs.h"

#endif /* OHGPU_H */
