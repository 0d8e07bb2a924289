"""ctypes binding of libohgpu.so -- exactly the entry points the headers under include/ declare.

The record dtypes and constants come first, then the signature tables (ABI_TABLES: one per header), the private marshalling helpers
(_typed, _ptr, _create, _fetch, _phase_ms, _paths, _process_host), and every family's named functions and Context methods over them.

There is no CPU fallback: if the library is missing this module raises, and if there is no GPU
ohgpu_init() returns OHGPU_ERR_NO_DEVICE which `Context` turns into an exception.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libohgpu.so")

OK = 0
ERR_INVALID, ERR_DEVICE, ERR_NO_DEVICE, ERR_NOMEM, ERR_BOUNDS, ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6
ENDIAN_LITTLE, ENDIAN_BIG = 1, 2
RAMP_MAX = 16384
UNITY_ATTENUATION = 256
FLAG_RAMP, FLAG_SILENCE, FLAG_ZERO_LSB32, FLAG_SRC_PLANAR32 = 1, 2, 4, 8

# numpy views of ohgpu_msg_desc (32 B) and ohgpu_src_msg_desc (64 B)
MSG_DESC = np.dtype([
    ("src_offset", "<u8"), ("dst_offset", "<u8"), ("n_frames", "<u4"),
    ("ramp_start", "<u2"), ("ramp_end", "<u2"), ("attenuation", "<u2"),
    ("channels", "u1"), ("src_bits", "u1"), ("src_endian", "u1"),
    ("dst_bits", "u1"), ("dst_endian", "u1"), ("flags", "u1")], align=False)
SRC_MSG_DESC = np.dtype([
    ("src_offset", "<u8"), ("src_frame0", "<u8"), ("src_frames", "<u8"), ("out_frame0", "<u8"),
    ("dst_offset", "<u8"), ("n_frames", "<u4"),
    ("ramp_start", "<u2"), ("ramp_end", "<u2"), ("attenuation", "<u2"),
    ("channels", "u1"), ("src_bits", "u1"), ("src_endian", "u1"),
    ("dst_bits", "u1"), ("dst_endian", "u1"), ("flags", "u1"), ("src_plane_stride", "<u8")], align=False)

# ohgpu_src_pull_msg_desc (80 B): the pulled resampler's message
SRC_PULL_MSG_DESC = np.dtype([
    ("src_offset", "<u8"), ("src_frame0", "<u8"), ("src_frames", "<u8"), ("pos_frame", "<u8"), ("step", "<u8"),
    ("dst_offset", "<u8"), ("pos_frac", "<u4"), ("n_frames", "<u4"),
    ("ramp_start", "<u2"), ("ramp_end", "<u2"), ("attenuation", "<u2"),
    ("channels", "u1"), ("src_bits", "u1"), ("src_endian", "u1"),
    ("dst_bits", "u1"), ("dst_endian", "u1"), ("flags", "u1"), ("reserved", "u1", (4,)), ("src_plane_stride", "<u8")], align=False)
assert SRC_PULL_MSG_DESC.itemsize == 80
SRC_PULL_NOMINAL = 1 << 31
SRC_PULL_MAX_STEP = 16 << 32

FMT_UNPACK_PLANAR, FMT_SENDER_PACK, FMT_FLAC_PACK = 1, 2, 3
FMT_DESC = np.dtype([
    ("src_offset", "<u8"), ("dst_offset", "<u8"), ("src_plane_stride", "<u8"), ("dst_plane_stride", "<u8"),
    ("n_frames", "<u4"), ("kind", "u1"), ("channels", "u1"), ("src_bits", "u1"), ("dst_bits", "u1"),
    ("reserved", "u1", (8,))], align=False)

# DSD: ohgpu_dsd_desc (32 B)
DSD_PASS, DSD_DSF, DSD_DFF, DSD_RAW = 1, 2, 3, 4
DSD_FLAG_SILENCE = 1
DSD_SILENCE_BYTE = 0x69
DSD_DESC = np.dtype([
    ("src_offset", "<u8"), ("dst_offset", "<u8"), ("n_chunks", "<u4"), ("kind", "u1"), ("flags", "u1"),
    ("sample_block_words", "u1"), ("pad_bytes_per_chunk", "u1"), ("reserved", "u1", (8,))], align=False)
assert DSD_DESC.itemsize == 32

# DSD -> PCM: ohgpu_dsd_pcm_msg_desc (64 B)
DSD_PCM_MSG_DESC = np.dtype([
    ("src_offset", "<u8"), ("src_chunk0", "<u8"), ("src_chunks", "<u8"), ("out_frame0", "<u8"), ("dst_offset", "<u8"),
    ("n_frames", "<u4"), ("ramp_start", "<u2"), ("ramp_end", "<u2"), ("sample_block_words", "u1"), ("pad_bytes_per_chunk", "u1"),
    ("dst_endian", "u1"), ("flags", "u1"), ("reserved", "u1", (12,))], align=False)
assert DSD_PCM_MSG_DESC.itemsize == 64

# FLAC frames: ohgpu_flac_stream_desc (64 B), ohgpu_flac_stream_result (48 B), ohgpu_flac_streaminfo_t (48 B)
FLAC_OK, FLAC_CORRUPT, FLAC_UNSUPPORTED, FLAC_OVERFLOW = 0, 1, 2, 3
FLAC_FLAG_AT_FRAME, FLAC_OUT_PACKED_BE = 1, 2
FLAC_STREAM_DESC = np.dtype([
    ("src_offset", "<u8"), ("src_bytes", "<u8"), ("dst_offset", "<u8"), ("dst_plane_stride", "<u8"), ("first_sample", "<u8"),
    ("max_samples", "<u4"), ("sample_rate", "<u4"), ("blocksize", "<u4"), ("max_blocksize", "<u4"),
    ("channels", "u1"), ("bits", "u1"), ("flags", "u1"), ("reserved", "u1", (5,))], align=False)
FLAC_STREAM_RESULT = np.dtype([
    ("status", "<u4"), ("frames", "<u4"), ("samples", "<u8"), ("first_sample_decoded", "<u8"), ("bytes_consumed", "<u8"),
    ("candidates", "<u4"), ("candidates_rejected", "<u4"), ("reserved", "<u8")], align=False)
FLAC_STREAMINFO = np.dtype([
    ("min_blocksize", "<u4"), ("max_blocksize", "<u4"), ("sample_rate", "<u4"), ("channels", "u1"), ("bits", "u1"),
    ("reserved", "u1", (2,)), ("total_samples", "<u8"), ("md5", "u1", (16,)), ("min_framesize", "<u4"), ("max_framesize", "<u4")], align=False)
FLAC_FRAME = np.dtype([("stream", "<u4"), ("blocksize", "<u4"), ("first_sample", "<u8"), ("src_pos", "<u4"), ("src_end", "<u4")], align=False)
assert FLAC_FRAME.itemsize == 24
assert FLAC_STREAM_DESC.itemsize == 64 and FLAC_STREAM_RESULT.itemsize == 48 and FLAC_STREAMINFO.itemsize == 48

# Apple Lossless packets: ohgpu_alac_config (24 B), ohgpu_alac_packet (16 B), ohgpu_alac_stream_desc (64 B)
ALAC_OK, ALAC_CORRUPT, ALAC_UNSUPPORTED = 0, 1, 2
ALAC_OUT_PACKED_LE, ALAC_OUT_PACKED_BE = 1, 2
ALAC_ROUTE_FUSED, ALAC_ROUTE_PLAIN = 1, 2
_ALAC_CONFIG_FIELDS = [("frame_length", "<u4"), ("compatible_version", "u1"), ("bit_depth", "u1"), ("pb", "u1"), ("mb", "u1"), ("kb", "u1"),
                       ("channels", "u1"), ("max_run", "<u2"), ("max_frame_bytes", "<u4"), ("avg_bit_rate", "<u4"), ("sample_rate", "<u4")]
ALAC_CONFIG = np.dtype(_ALAC_CONFIG_FIELDS, align=False)
ALAC_PACKET = np.dtype([("src_offset", "<u8"), ("bytes", "<u4"), ("reserved", "<u4")], align=False)
ALAC_STREAM_DESC = np.dtype(_ALAC_CONFIG_FIELDS + [("first_packet", "<u4"), ("n_packets", "<u4"), ("dst_offset", "<u8"), ("dst_plane_stride", "<u8"),
                                                   ("flags", "<u4"), ("reserved", "<u4", (3,))], align=False)
ALAC_PACKET_RESULT = np.dtype([("status", "<u4"), ("samples", "<u4")], align=False)
ALAC_STREAM_RESULT = np.dtype([("packets_ok", "<u4"), ("first_bad_status", "<u4"), ("samples", "<u8")], align=False)
assert ALAC_CONFIG.itemsize == 24 and ALAC_PACKET.itemsize == 16 and ALAC_STREAM_DESC.itemsize == 64 and ALAC_STREAM_RESULT.itemsize == 16
# RAOP audio: ohgpu_raop_stream_desc (96 B) = an ohgpu_alac_stream_desc, the session's AES key and IV; the packet
# table, the results and the routes are Apple Lossless's
RAOP_OUT_PLAINTEXT = 4
RAOP_STREAM_DESC = np.dtype(ALAC_STREAM_DESC.descr + [("aes_key", "u1", (16,)), ("aes_iv", "u1", (16,))], align=False)
assert RAOP_STREAM_DESC.itemsize == 96

BATCH_PATHS = np.dtype([(k, "<u4") for k in ("line_planned", "launches", "staged_chunks", "group_chunks", "heavy_chunks",
                                            "prefixed_chunks", "ohm_wide_fragments", "ohm_staged_fragments", "ohm_headers_fused",
                                            "ohm_headers_separate", "fmt_wide_records", "fmt_stereo_records", "fmt_stereo_kind",
                                            "fmt_stereo_bytes", "fmt_staged_chunks")] + [("reserved", "<u4", (1,))], align=False)
assert BATCH_PATHS.itemsize == 64

FLYWHEEL_DESC = np.dtype([
    ("src_offset", "<u8"), ("channel_bytes", "<u8"), ("dst_offset", "<u8"), ("in_samples", "<u4"),
    ("out_frames", "<u4"), ("block_frames", "<u4"), ("sample_rate", "<u4"), ("channels", "<u4"),
    ("reserved", "<u4")], align=False)

OHM_FLAG_HALT, OHM_FLAG_LOSSLESS, OHM_FLAG_TIMESTAMPED, OHM_FLAG_RESENT = 1, 2, 4, 8
OHM_STREAM = np.dtype([
    ("samples_total", "<u8"), ("sample_rate", "<u4"), ("bit_rate", "<u4"), ("volume_offset", "<i2"),
    ("src_channels", "u1"), ("src_bits", "u1"), ("codec_bytes", "u1"), ("codec", "u1", (29,)),
    ("src_endian", "u1"), ("reserved", "u1", (13,))], align=False)
OHM_FRAGMENT = np.dtype([
    ("src_offset", "<u8"), ("n_frames", "<u4"), ("ramp_start", "<u2"), ("ramp_end", "<u2"), ("attenuation", "<u2"),
    ("flags", "u1"), ("reserved", "u1", (5,))], align=False)
OHM_FRAME_DESC = np.dtype([
    ("dst_offset", "<u8"), ("sample_start", "<u8"), ("stream", "<u4"), ("frame", "<u4"), ("network_timestamp", "<u4"),
    ("media_latency", "<u4"), ("media_timestamp", "<u4"), ("first_fragment", "<u4"), ("n_fragments", "<u2"),
    ("flags", "u1"), ("reserved", "u1", (5,))], align=False)
assert OHM_STREAM.itemsize == 64 and OHM_FRAGMENT.itemsize == 24 and OHM_FRAME_DESC.itemsize == 48
# Songcast receiver: the datagram table, the stream table with the state carried between batches, a record per
# datagram (status, every header field, disposition) and a result per stream
OHM_RX_OK, OHM_RX_NOT_OHM, OHM_RX_NOT_AUDIO, OHM_RX_TRUNCATED, OHM_RX_BAD_HEADER, OHM_RX_OVERSIZE = range(6)
(OHM_RX_OUTPUT, OHM_RX_DUPLICATE, OHM_RX_PENDING, OHM_RX_DROPPED_BY_RESET, OHM_RX_STALE, OHM_RX_NOT_REACHED, OHM_RX_IGNORED) = range(1, 8)
OHM_RX_EVENT_NEW_STREAM, OHM_RX_EVENT_DELAY, OHM_RX_EVENT_HALT = 1, 2, 4
OHM_RX_STOP_NONE, OHM_RX_STOP_STALE, OHM_RX_STOP_HALT = 0, 1, 2
OHM_RX_DATAGRAM = np.dtype([("src_offset", "<u8"), ("bytes", "<u4"), ("reserved", "<u4")], align=False)
_OHM_RX_STATE = [("last_sample_start", "<u8"), ("frame", "<u4"), ("sample_rate", "<u4"), ("latency", "<u4"), ("running", "u1"),
                 ("stream_msg_due", "u1"), ("bit_depth", "u1"), ("channels", "u1"), ("state_reserved", "<u4", (2,))]
OHM_RX_STATE_FIELDS = tuple(name for name, *_ in _OHM_RX_STATE[:-1])
OHM_RX_STREAM = np.dtype([("first_datagram", "<u4"), ("n_datagrams", "<u4"), ("dst_offset", "<u8"), ("dst_capacity", "<u8")] + _OHM_RX_STATE +
                         [("reserved", "<u4", (2,))], align=False)
OHM_RX_RECORD = np.dtype([
    ("status", "u1"), ("disposition", "u1"), ("events", "u1"), ("flags", "u1"), ("msg_type", "u1"), ("bit_depth", "u1"), ("channels", "u1"),
    ("codec_bytes", "u1"), ("samples", "<u2"), ("volume_offset", "<i2"), ("frame", "<u4"), ("network_timestamp", "<u4"),
    ("media_latency", "<u4"), ("media_timestamp", "<u4"), ("sample_rate", "<u4"), ("sample_start", "<u8"), ("samples_total", "<u8"),
    ("bit_rate", "<u4"), ("audio_offset", "<u4"), ("audio_bytes", "<u4"), ("order", "<u4"), ("dst_offset", "<u8"), ("codec", "u1", (32,))], align=False)
OHM_RX_STREAM_RESULT = np.dtype(_OHM_RX_STATE + [("out_bytes", "<u8"), ("n_output", "<u4"), ("n_pending", "<u4"), ("stop_reason", "<u4"),
                                                 ("n_resend", "<u4"), ("resend", "<u4", (20,))], align=False)
assert OHM_RX_DATAGRAM.itemsize == 16 and OHM_RX_STREAM.itemsize == 64 and OHM_RX_RECORD.itemsize == 104 and OHM_RX_STREAM_RESULT.itemsize == 136
# Ogg pages: a descriptor and a result per stream, a record per completed packet
OGG_OK, OGG_LOST_SYNC, OGG_HOLE, OGG_NOT_FLAC, OGG_UNSUPPORTED_MAPPING, OGG_BAD_RESUME = range(6)
OGG_ANY_SEQ, OGG_FLAC_MAPPING, OGG_ANY_SERIAL, OGG_FOLLOW_LINKS = 1, 2, 4, 16
OGG_PACKET_BOS, OGG_PACKET_EOS, OGG_PACKET_MAPPING_HEADER, OGG_PACKET_LINK = 1, 2, 4, 8
OGG_STREAM_DESC = np.dtype([("src_offset", "<u8"), ("dst_offset", "<u8"), ("dst_capacity", "<u8"), ("src_bytes", "<u4"), ("serial", "<u4"),
                            ("expect_seq", "<u4"), ("packet_first", "<u4"), ("packet_capacity", "<u4"), ("first_page_segment", "<u4"),
                            ("flags", "<u4"), ("reserved", "<u4", (3,))], align=False)
OGG_STREAM_RESULT = np.dtype([("status", "<u4"), ("pages", "<u4"), ("pages_ignored", "<u4"), ("packets", "<u4"), ("bytes_delivered", "<u8"),
                              ("bytes_consumed", "<u8"), ("resume_segment", "<u4"), ("next_seq", "<u4"), ("last_granule", "<i8"),
                              ("serial", "<u4"), ("bos_seen", "u1"), ("eos_seen", "u1"), ("reserved", "u1", (2,)), ("reserved2", "<u8")], align=False)
# The other members of the two structs' unions, for .view(): the link magic where `reserved` is, `links` in the low half of `reserved2`
OGG_STREAM_DESC_LINKS = np.dtype(OGG_STREAM_DESC.descr[:-1] + [("link_magic_bytes", "<u4"), ("link_magic", "u1", (8,))], align=False)
OGG_STREAM_RESULT_LINKS = np.dtype(OGG_STREAM_RESULT.descr[:-1] + [("links", "<u4"), ("reserved2_high", "<u4")], align=False)
assert OGG_STREAM_DESC_LINKS.itemsize == 64 and OGG_STREAM_RESULT_LINKS.itemsize == 64
OGG_PACKET = np.dtype([("run_pos", "<u8"), ("bytes", "<u4"), ("flags", "<u4"), ("granule", "<i8"), ("page_offset", "<u8"),
                       ("page_seq", "<u4"), ("segment", "<u4")], align=False)
assert OGG_STREAM_DESC.itemsize == 64 and OGG_STREAM_RESULT.itemsize == 64 and OGG_PACKET.itemsize == 40
# MPEG-4 container: ohgpu_mp4_stream_desc (32 B), ohgpu_mp4_stream_result (112 B), ohgpu_mp4_sample (16 B); the packet
# table's rows are ALAC_PACKET
MP4_OK, MP4_NOT_MP4, MP4_TRUNCATED, MP4_INVALID, MP4_NOT_ALAC, MP4_UNSUPPORTED = range(6)
MP4_MAX_SAMPLES, MP4_MAX_BOXES, MP4_NO_SAMPLE = 1 << 24, 4096, 0xffffffff
MP4_ROUTE_FUSED, MP4_ROUTE_PLAIN = 1, 2
MP4_STREAM_DESC = np.dtype([("src_offset", "<u8"), ("src_bytes", "<u4"), ("flags", "<u4"), ("packet_first", "<u4"), ("packet_capacity", "<u4"),
                            ("reserved", "<u4", (2,))], align=False)
MP4_STREAM_RESULT = np.dtype([("status", "<u4"), ("codec", "<u4"), ("config", ALAC_CONFIG), ("timescale", "<u4"), ("entry_rate", "<u4"), ("duration", "<u8"),
                              ("frames", "<u8"), ("samples", "<u4"), ("chunks", "<u4"), ("samples_available", "<u4"), ("samples_refused", "<u4"),
                              ("first_bad_sample", "<u4"), ("entry_channels", "<u2"), ("entry_bits", "<u2"), ("moov_offset", "<u8"), ("mdat_offset", "<u8"),
                              ("mdat_bytes", "<u8"), ("error_offset", "<u8")], align=False)
MP4_SAMPLE = np.dtype([("first_frame", "<u8"), ("frames", "<u4"), ("chunk", "<u4")], align=False)
assert MP4_STREAM_DESC.itemsize == 32 and MP4_STREAM_RESULT.itemsize == 112 and MP4_SAMPLE.itemsize == 16
# fragmented MPEG-4: ohgpu_mp4f_stream_desc (64 B), ohgpu_mp4f_run (32 B), ohgpu_mp4f_stream_result (168 B); the sample and
# packet rows are MP4_SAMPLE and ALAC_PACKET
MP4F_OK, MP4F_NOT_MP4, MP4F_TRUNCATED, MP4F_INVALID, MP4F_NOT_CODEC, MP4F_UNSUPPORTED, MP4F_NOT_FRAGMENTED = range(7)
MP4F_CODEC_ALAC, MP4F_CODEC_FLAC, MP4F_GATHER = 1, 2, 1
MP4F_MAX_BOXES, MP4F_MAX_SAMPLES, MP4F_MAX_RUN_SAMPLES = 65536, 1 << 24, 1 << 16
MP4F_ROUTE_PHASES, MP4F_ROUTE_PLAIN = 1, 2
MP4F_STREAM_DESC = np.dtype([("src_offset", "<u8"), ("src_bytes", "<u4"), ("codecs", "<u4"), ("flags", "<u4"), ("packet_first", "<u4"), ("packet_capacity", "<u4"),
                             ("run_first", "<u4"), ("run_capacity", "<u4"), ("gather_first_row", "<u4"), ("dst_offset", "<u8"), ("dst_capacity", "<u8"),
                             ("reserved", "<u4", (2,))], align=False)
MP4F_RUN = np.dtype([("data_offset", "<u8"), ("first_frame", "<u8"), ("first_sample", "<u4"), ("samples", "<u4"), ("bytes", "<u8")], align=False)
MP4F_STREAM_RESULT = np.dtype([("status", "<u4"), ("codec", "<u4"), ("track_id", "<u4"), ("timescale", "<u4"), ("config", ALAC_CONFIG), ("flac", FLAC_STREAMINFO),
                               ("duration", "<u8"), ("frames", "<u8"), ("samples", "<u8"), ("runs", "<u4"), ("samples_available", "<u4"), ("samples_refused", "<u4"),
                               ("first_bad_sample", "<u4"), ("entry_rate", "<u4"), ("entry_channels", "<u2"), ("entry_bits", "<u2"), ("bytes_gathered", "<u8"),
                               ("moov_offset", "<u8"), ("first_moof_offset", "<u8"), ("error_offset", "<u8")], align=False)
assert MP4F_STREAM_DESC.itemsize == 64 and MP4F_RUN.itemsize == 32 and MP4F_STREAM_RESULT.itemsize == 168
# protected fragmented MPEG-4: ohgpu_cenc_stream_desc (112 B), ohgpu_cenc_stream_result (208 B); statuses 0..6 are MP4F_*
CENC_NO_KEY, CENC_HAVE_KEY, CENC_SCHEME = 7, 1, 0x63656e63
CENC_STREAM_DESC = np.dtype(MP4F_STREAM_DESC.descr + [("key_flags", "<u4"), ("reserved2", "<u4", (3,)), ("kid", "u1", (16,)), ("key", "u1", (16,))], align=False)
CENC_STREAM_RESULT = np.dtype([("mp4f", MP4F_STREAM_RESULT), ("entry", "<u4"), ("scheme", "<u4"), ("is_protected", "u1"), ("iv_size", "u1"), ("pad", "u1", (2,)),
                               ("reserved", "<u4"), ("kid", "u1", (16,)), ("blocks", "<u8")], align=False)
assert CENC_STREAM_DESC.itemsize == 112 and CENC_STREAM_RESULT.itemsize == 208
# protected fragmented MPEG-4, the second family: ohgpu_cbcs_stream_desc (120 B), ohgpu_cbcs_stream_result (232 B); the statuses are CENC's
CBCS_SCHEME_CENC, CBCS_SCHEME_CBCS = 0x63656e63, 0x63626373
CBCS_STREAM_DESC = np.dtype(CENC_STREAM_DESC.descr + [("subsample_first", "<u4"), ("subsample_capacity", "<u4")], align=False)
CBCS_STREAM_RESULT = np.dtype([("cenc", CENC_STREAM_RESULT), ("crypt_blocks", "u1"), ("skip_blocks", "u1"), ("constant_iv_size", "u1"), ("pad", "u1"),
                               ("subsamples", "<u4"), ("constant_iv", "u1", (16,))], align=False)
assert CBCS_STREAM_DESC.itemsize == 120 and CBCS_STREAM_RESULT.itemsize == 232
# PCM files: ohgpu_iff_stream_desc (64 B), ohgpu_iff_stream_result (80 B)
IFF_OK, IFF_NOT_IFF, IFF_TRUNCATED, IFF_INVALID, IFF_UNSUPPORTED = range(5)
IFF_KIND_WAV, IFF_KIND_AIFF, IFF_KIND_AIFC = 1, 2, 3
IFF_MAX_CHUNKS, IFF_MAX_CHANNELS, IFF_MAX_FRAME_BYTES, IFF_FLAG_WAV8_UNSIGNED = 4096, 10, 40, 1
IFF_ROUTE_FUSED, IFF_ROUTE_PLAIN = 1, 2
IFF_STREAM_DESC = np.dtype([("src_offset", "<u8"), ("src_bytes", "<u4"), ("flags", "<u4"), ("dst_offset", "<u8"), ("dst_bytes_capacity", "<u8"),
                            ("frame_first", "<u8"), ("dst_frame_capacity", "<u4"), ("max_bit_depth", "<u4"), ("reserved", "<u4", (4,))], align=False)
IFF_STREAM_RESULT = np.dtype([("status", "<u4"), ("kind", "<u4"), ("channels", "<u4"), ("sample_rate", "<u4"), ("src_bit_depth", "<u4"), ("out_bit_depth", "<u4"),
                              ("src_endian", "<u4"), ("bit_rate", "<u4"), ("frames_total", "<u8"), ("frames_available", "<u8"), ("frames_written", "<u8"),
                              ("data_offset", "<u8"), ("data_bytes", "<u8"), ("error_offset", "<u8")], align=False)
assert IFF_STREAM_DESC.itemsize == 64 and IFF_STREAM_RESULT.itemsize == 80
# DSD files: ohgpu_dsd_file_stream_desc (64 B), ohgpu_dsd_file_stream_result (96 B)
DSD_FILE_OK, DSD_FILE_NOT_DSD, DSD_FILE_TRUNCATED, DSD_FILE_INVALID, DSD_FILE_UNSUPPORTED = range(5)
DSD_FILE_KIND_DSF, DSD_FILE_KIND_DFF, DSD_FILE_MAX_CHUNKS = 2, 3, 4096
DSD_FILE_ROUTE_FUSED, DSD_FILE_ROUTE_PLAIN = 1, 2
DSD_FILE_STREAM_DESC = np.dtype([("src_offset", "<u8"), ("src_bytes", "<u4"), ("flags", "<u4"), ("dst_offset", "<u8"), ("dst_bytes_capacity", "<u8"),
                                 ("chunk_first", "<u8"), ("sample_block_words", "<u4"), ("pad_bytes_per_chunk", "<u4"), ("reserved", "<u4", (4,))], align=False)
DSD_FILE_STREAM_RESULT = np.dtype([("status", "<u4"), ("kind", "<u4"), ("channels", "<u4"), ("sample_rate", "<u4"), ("format_version", "<u4"), ("channel_type", "<u4"),
                                   ("sample_count", "<u8"), ("chunks_total", "<u8"), ("chunks_available", "<u8"), ("chunks_written", "<u8"), ("bytes_written", "<u8"),
                                   ("data_offset", "<u8"), ("data_bytes", "<u8"), ("metadata_offset", "<u8"), ("error_offset", "<u8")], align=False)
assert DSD_FILE_STREAM_DESC.itemsize == 64 and DSD_FILE_STREAM_RESULT.itemsize == 96
# the RAOP receiver (include/ohgpu_raop_rx.h): the datagram table, the stream table with the state carried between
# batches, a record per datagram, a result per stream with the resend ranges
RAOP_RX_MAX_PACKET_BYTES, RAOP_RX_MAX_FRAMES, RAOP_RX_MAX_RANGES = 1472, 63, 31
RAOP_RX_PORT_AUDIO, RAOP_RX_PORT_CONTROL = 0, 1
RAOP_RX_OK, RAOP_RX_TRUNCATED, RAOP_RX_OVERSIZE, RAOP_RX_OTHER_TYPE = range(4)
(RAOP_RX_OUTPUT, RAOP_RX_DUPLICATE, RAOP_RX_PENDING, RAOP_RX_DROPPED_BY_RESET, RAOP_RX_FLUSHED, RAOP_RX_WRONG_SESSION, RAOP_RX_SYNC, RAOP_RX_IGNORED,
 RAOP_RX_NOT_REACHED) = range(1, 10)
RAOP_RX_EVENT_NEW_STREAM, RAOP_RX_EVENT_DELAY = 1, 2
RAOP_RX_STOP_NONE, RAOP_RX_STOP_BUFFER_FULL, RAOP_RX_STOP_RESTARTED = 0, 1, 2
RAOP_RX_DATAGRAM = np.dtype([("src_offset", "<u8"), ("bytes", "<u4"), ("port", "u1"), ("reserved", "u1", (3,))], align=False)
_RAOP_RX_STATE = [("flush_seq", "<u4"), ("flush_time", "<u4"), ("session_id", "<u4"), ("latency", "<u4"), ("control_latency", "<u4"), ("frame", "<u2"),
                  ("running", "u1"), ("started", "u1"), ("resume_pending", "u1"), ("state_reserved", "u1", (7,))]
RAOP_RX_STATE_FIELDS = tuple(name for name, *_ in _RAOP_RX_STATE[:-1])
RAOP_RX_STREAM = np.dtype([("first_datagram", "<u4"), ("n_datagrams", "<u4"), ("max_frames", "<u4"), ("reserved", "<u4")] + _RAOP_RX_STATE, align=False)
RAOP_RX_RECORD = np.dtype([
    ("status", "u1"), ("disposition", "u1"), ("events", "u1"), ("resend", "u1"), ("marker", "u1"), ("extension", "u1"), ("type", "u1"), ("port", "u1"),
    ("seq", "<u2"), ("payload_offset", "<u2"), ("payload_bytes", "<u4"), ("timestamp", "<u4"), ("ssrc", "<u4"), ("sync", "<u4", (4,)), ("order", "<u4"),
    ("reserved", "<u4")], align=False)
RAOP_RX_STREAM_RESULT = np.dtype(_RAOP_RX_STATE + [("n_output", "<u4"), ("n_pending", "<u4"), ("stop_reason", "<u4"), ("n_ranges", "<u4"),
                                                  ("ranges", "<u4", (31, 2))], align=False)
assert RAOP_RX_DATAGRAM.itemsize == 16 and RAOP_RX_STREAM.itemsize == 48 and RAOP_RX_RECORD.itemsize == 48 and RAOP_RX_STREAM_RESULT.itemsize == 296
# the MPEG transport stream demultiplexer and the ADTS frame table (include/ohgpu_ts.h): a descriptor and a result per
# stream in both layers, a record per PES packet, a record per ADTS frame
TS_PACKET_BYTES, TS_NONE, TS_NO_PTS = 188, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
TS_OK, TS_NO_PAT, TS_NO_PMT, TS_NO_AUDIO, TS_CORRUPT = range(5)
TS_PES_OPEN = 1
TS_PES_CONTINUATION, TS_PES_EXCESS, TS_PES_TRUNCATED, TS_PES_CC_JUMP = 1, 2, 4, 8
ADTS_OK, ADTS_NOT_ADTS = 0, 1
ADTS_RECOGNISE, ADTS_INTERRUPTED = 1, 1
ADTS_RECOGNISE_LAST_START, ADTS_RECOGNISE_FRAMES = 1001, 5
TS_STREAM_DESC = np.dtype([("src_offset", "<u8"), ("dst_offset", "<u8"), ("dst_capacity", "<u8"), ("src_bytes", "<u4"), ("flags", "<u4"), ("pmt_pid", "<u4"),
                           ("audio_pid", "<u4"), ("pes_open_bytes", "<u4"), ("pes_first", "<u4"), ("pes_capacity", "<u4"), ("reserved", "<u4", (3,))], align=False)
TS_STREAM_RESULT = np.dtype([("status", "u1"), ("trailing_bytes", "u1"), ("reserved", "<u2"), ("pmt_pid", "<u2"), ("audio_pid", "<u2"), ("packets", "<u4"),
                             ("bad_sync", "<u4"), ("tei_packets", "<u4"), ("scrambled_packets", "<u4"), ("pat_packet", "<u4"), ("pmt_packet", "<u4"),
                             ("audio_packets", "<u4"), ("pes_packets", "<u4"), ("bad_pes_starts", "<u4"), ("bytes_delivered", "<u4"), ("dropped_bytes", "<u4"),
                             ("cc_jumps", "<u4"), ("pes_open_bytes", "<u4"), ("corrupt_packet", "<u4")], align=False)
TS_PES = np.dtype([("es_offset", "<u8"), ("pts", "<u8"), ("bytes", "<u4"), ("packet", "<u4"), ("flags", "<u4"), ("stream_id", "u1"), ("reserved", "u1", (3,))], align=False)
ADTS_STREAM_DESC = np.dtype([("src_offset", "<u8"), ("src_bytes", "<u4"), ("flags", "<u4"), ("frame_first", "<u4"), ("frame_capacity", "<u4"),
                             ("reserved", "<u4", (2,))], align=False)
ADTS_STREAM_RESULT = np.dtype([("status", "<u4"), ("frames", "<u4"), ("bytes_consumed", "<u4"), ("first_frame_offset", "<u4"), ("interruptions", "<u4"),
                               ("skipped_bytes", "<u4"), ("mean_payload_bytes", "<u4"), ("profile", "u1"), ("sf_index", "u1"), ("channel_config", "u1"),
                               ("reserved", "u1"), ("reserved2", "<u4", (8,))], align=False)
ADTS_FRAME = np.dtype([("offset", "<u8"), ("bytes", "<u4"), ("flags", "<u4"), ("header_bytes", "u1"), ("profile", "u1"), ("sf_index", "u1"), ("channel_config", "u1"),
                       ("reserved", "<u4", (3,))], align=False)
assert TS_STREAM_DESC.itemsize == 64 and TS_STREAM_RESULT.itemsize == 64 and TS_PES.itemsize == 32
assert ADTS_STREAM_DESC.itemsize == 32 and ADTS_STREAM_RESULT.itemsize == 64 and ADTS_FRAME.itemsize == 32
# the Vorbis I decoder (include/ohgpu_vorbis.h): the setup image's info, a descriptor per stream over rows of ALAC_PACKET
VORBIS_OK, VORBIS_HEADER, VORBIS_CORRUPT = 0, 1, 2
VORBIS_OUT_PLANAR32 = 1
VORBIS_INFO = np.dtype([("channels", "<u4"), ("sample_rate", "<u4"), ("blocksize_short", "<u4"), ("blocksize_long", "<u4"), ("image_bytes", "<u4"),
                        ("codebooks", "<u4"), ("modes", "<u4"), ("reserved", "<u4")], align=False)
VORBIS_STREAM_DESC = np.dtype([("image_offset", "<u8"), ("dst_offset", "<u8"), ("dst_plane_stride", "<u8"), ("max_samples", "<u8"), ("image_bytes", "<u4"),
                               ("first_packet", "<u4"), ("n_packets", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (4,))], align=False)
VORBIS_PACKET_RESULT = np.dtype([("status", "u1"), ("mode", "u1"), ("blocksize", "<u2"), ("samples", "<u4"), ("position", "<u8"), ("reserved", "<u8")], align=False)
VORBIS_STREAM_RESULT = np.dtype([("packets_ok", "<u4"), ("first_bad_status", "<u4"), ("samples", "<u8"), ("reserved", "<u8")], align=False)
assert VORBIS_INFO.itemsize == 32 and VORBIS_STREAM_DESC.itemsize == 64 and VORBIS_PACKET_RESULT.itemsize == 24 and VORBIS_STREAM_RESULT.itemsize == 24
# a link of a chained Ogg Vorbis stream (ohgpu_vorbis_link)
VORBIS_LINK_CONTINUED, VORBIS_LINK_HEAD_OPEN = 0xFFFFFFFFFFFFFFFF, 1
VORBIS_LINK = np.dtype([("stream", "<u4"), ("serial", "<u4"), ("page_offset", "<u8"), ("first_packet", "<u4"), ("n_packets", "<u4"), ("head", "<i4"),
                        ("channels", "<u4"), ("sample_rate", "<u4"), ("blocksize_short", "<u4"), ("blocksize_long", "<u4"), ("reserved", "<u4"),
                        ("dst_offset", "<u8"), ("samples", "<u8")], align=False)
assert VORBIS_LINK.itemsize == 64
MF_STEP = np.dtype([("aoff", "<u4", (16,)), ("b0", "<u4", (16,)), ("b1", "<u4", (16,)), ("b2", "<i4", (16,)), ("kc", "<u4"), ("pad", "<u4", (7,))])
assert MF_STEP.itemsize == 288

# ---- the ABI's signatures: a table per header under include/, name -> (restype, argtypes), and ABI_TABLES over the six.  lib() binds
# what ABI_TABLES lists; tests/test_capi_loads.py holds every entry to its header's prototype, argument by argument.  The shapes that
# recur have a name each.
_int, _u32, _u64, _sz, _dbl = C.c_int, C.c_uint32, C.c_uint64, C.c_size_t, C.c_double
_vp, _vpp, _str = C.c_void_p, C.POINTER(C.c_void_p), C.c_char_p
_u32p, _u64p, _szp, _intp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t), C.POINTER(C.c_int)
_HANDLE = (_int, [_vp, _vp])                                           # (ctx, handle): a destroy, a free, a wait
_CREATE = (_int, [_vp, _vp, _sz, _u64, _u64, _vpp])                    # (ctx, descs, n, src arena, dst arena, batch out)
_CREATE_FILTER = (_int, [_vp, _vp, _vp, _sz, _u64, _u64, _vpp])        # ... with a filter in front of the descriptors
_CREATE_PACKETS = (_int, [_vp, _vp, _sz, _vp, _sz, _u64, _u64, _vpp])  # ... with a second table behind them
_CHECK = (_int, [_vp, _sz, _u64, _u64])                                # _CREATE without a device
_CHECK_PACKETS = (_int, [_vp, _sz, _vp, _sz, _u64, _u64])              # _CREATE_PACKETS without a device
_RUN = (_int, [_vp, _vp, _vp, _vp, _vp])                               # (ctx, batch, src, dst, stream)
_RUN_SRC = (_int, [_vp, _vp, _vp, _vp])                                # (ctx, batch, src, stream): a batch with no destination arena
_FETCH = (_int, [_vp, _vp, _vp, _sz])                                  # (ctx, batch, out, n): a table of the last run
_FETCH_PAIR = (_int, [_vp, _vp, _vp, _sz, _vp, _sz])                   # ... two tables in one call
_PHASE_MS = (_int, [_vp, _vp, C.POINTER(C.c_float)])                   # (ctx, batch, ms[K])
_PATHS = (_int, [_vp, _u32p, _u32p, _u32p])                            # (batch, three words out)
_PATHS_PAIR = (_int, [_vp, _u32p, _u32p])                              # (batch, two words out)
_HEAD = (_int, [_vp, _sz, _vp])                                        # (bytes, n, one record out), host only
_HOST = (_int, [_vp, _vp, _sz, _vp, _u64, _vp, _u64])                  # (ctx, descs, n, src, bytes, dst, bytes)
_HOST_FILTER = (_int, [_vp, _vp, _vp, _sz, _vp, _u64, _vp, _u64])      # ... with a filter
_HOST_RESULTS = (_int, [_vp, _vp, _sz, _vp, _u64, _vp, _u64, _vp])     # ... with the stream results out
_HOST_PACKETS = (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u64, _vp, _u64, _vp, _vp])   # two tables in, two out
_FRAG_CHECK = (_int, [_vp, _sz, _sz, _sz, _u64, _u64])                 # the fragmented MPEG-4 families: descs, n, n_packets, n_runs
_FRAG_CREATE = (_int, [_vp, _vp, _sz, _sz, _sz, _u64, _u64, _vpp])
_FRAG_HOST = (_int, [_vp, _vp, _sz, _sz, _sz, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp])
_FRAG_FLAC_HOST = (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _szp])
# include/ohgpu.h
SYMBOLS = {
    "ohgpu_abi_version": (_int, []),
    "ohgpu_last_error": (_str, []),
    "ohgpu_device_count": (_int, []),
    "ohgpu_init": (_int, [_int, _vpp]),
    "ohgpu_shutdown": (_int, [_vp]),
    "ohgpu_device_name": (_int, [_vp, _str, _sz]),
    "ohgpu_device_pci_bus_id": (_int, [_vp, _str, _sz]),
    "ohgpu_malloc": (_int, [_vp, _sz, _vpp]),
    "ohgpu_free": _HANDLE,
    "ohgpu_malloc_host": (_int, [_vp, _sz, _vpp]),
    "ohgpu_free_host": _HANDLE,
    "ohgpu_memcpy_h2d": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "ohgpu_memcpy_d2h": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "ohgpu_memset": (_int, [_vp, _vp, _int, _sz, _vp]),
    "ohgpu_stream_create": (_int, [_vp, _vpp]),
    "ohgpu_stream_destroy": _HANDLE,
    "ohgpu_stream_sync": _HANDLE,
    "ohgpu_event_create": (_int, [_vp, _vpp]),
    "ohgpu_event_destroy": _HANDLE,
    "ohgpu_event_record": (_int, [_vp, _vp, _vp]),
    "ohgpu_stream_wait_event": (_int, [_vp, _vp, _vp]),
    "ohgpu_event_elapsed_ms": (_int, [_vp, _vp, _vp, C.POINTER(C.c_float)]),
    "ohgpu_ramp_table": (_int, [C.POINTER(C.c_uint16)]),
    "ohgpu_pcm_batch_create": _CREATE,
    "ohgpu_pcm_batch_run": _RUN,
    "ohgpu_batch_destroy": _HANDLE,
    "ohgpu_batch_info": (_int, [_vp, _u64p, _u64p, _u64p, _u64p, _u64p]),
    "ohgpu_batch_paths_info": (_int, [_vp, _vp]),
    "ohgpu_pcm_process_host": _HOST,
    "ohgpu_fmt_batch_create": _CREATE,
    "ohgpu_fmt_batch_run": _RUN,
    "ohgpu_dsd_layout": (_int, [_u32, _u32, _u32, _u32, _u64p, _u64p]),
    "ohgpu_dsd_batch_create": _CREATE,
    "ohgpu_dsd_batch_run": _RUN,
    "ohgpu_dsd_batch_paths": _PATHS,
    "ohgpu_dsd_process_host": _HOST,
    "ohgpu_dsd_pcm_design": (_int, [_u32, _u32, _u32, _dbl, _dbl, _dbl, _vp, _sz, _u32p]),
    "ohgpu_dsd_pcm_create": (_int, [_vp, _u32, _u32, _vp, _vpp]),
    "ohgpu_dsd_pcm_destroy": _HANDLE,
    "ohgpu_dsd_pcm_window": (_int, [_u64, _u32, _u32, _u32, _u64p, _u64p]),
    "ohgpu_dsd_pcm_batch_create": _CREATE_FILTER,
    "ohgpu_dsd_pcm_batch_check": (_int, [_u32, _u32, _vp, _sz, _u64, _u64]),
    "ohgpu_dsd_pcm_batch_run": _RUN,
    "ohgpu_dsd_pcm_batch_paths": _PATHS,
    "ohgpu_dsd_pcm_process_host": _HOST_FILTER,
    "ohgpu_flac_streaminfo": (_int, [_vp, _sz, _vp, _u64p]),
    "ohgpu_flac_batch_check": _CHECK,
    "ohgpu_flac_batch_create": _CREATE,
    "ohgpu_flac_batch_run": _RUN,
    "ohgpu_flac_batch_results": _FETCH,
    "ohgpu_flac_batch_frames": (_int, [_vp, _vp, _vp, _sz, _szp]),
    "ohgpu_flac_batch_phase_ms": _PHASE_MS,
    "ohgpu_flac_process_host": (_int, [_vp, _vp, _sz, _vp, _u64, _vp, _u64, _vp, _vp, _sz, _szp]),
    "ohgpu_alac_config_parse": _HEAD,
    "ohgpu_alac_batch_check": _CHECK_PACKETS,
    "ohgpu_alac_batch_create": _CREATE_PACKETS,
    "ohgpu_alac_batch_run": _RUN,
    "ohgpu_alac_batch_results": _FETCH_PAIR,
    "ohgpu_alac_batch_phase_ms": _PHASE_MS,
    "ohgpu_alac_process_host": _HOST_PACKETS,
    "ohgpu_raop_fmtp_parse": (_int, [_str, _sz, _vp]),
    "ohgpu_raop_batch_check": _CHECK_PACKETS,
    "ohgpu_raop_batch_create": _CREATE_PACKETS,
    "ohgpu_raop_batch_run": _RUN,
    "ohgpu_raop_batch_results": _FETCH_PAIR,
    "ohgpu_raop_batch_phase_ms": _PHASE_MS,
    "ohgpu_raop_process_host": _HOST_PACKETS,
    "ohgpu_ohm_rx_batch_check": _CHECK_PACKETS,
    "ohgpu_ohm_rx_batch_create": _CREATE_PACKETS,
    "ohgpu_ohm_rx_batch_run": _RUN,
    "ohgpu_ohm_rx_batch_results": _FETCH_PAIR,
    "ohgpu_ohm_rx_batch_phase_ms": _PHASE_MS,
    "ohgpu_ohm_rx_process_host": _HOST_PACKETS,
    "ohgpu_ogg_batch_check": (_int, [_vp, _sz, _sz, _u64, _u64]),
    "ohgpu_ogg_batch_create": (_int, [_vp, _vp, _sz, _sz, _u64, _u64, _vpp]),
    "ohgpu_ogg_batch_run": _RUN,
    "ohgpu_ogg_batch_results": _FETCH,
    "ohgpu_ogg_batch_packets": _FETCH,
    "ohgpu_ogg_batch_phase_ms": _PHASE_MS,
    "ohgpu_ogg_process_host": (_int, [_vp, _vp, _sz, _sz, _vp, _u64, _vp, _u64, _vp, _vp]),
    "ohgpu_mp4_batch_check": (_int, [_vp, _sz, _sz, _u64]),
    "ohgpu_mp4_batch_create": (_int, [_vp, _vp, _sz, _sz, _u64, _vpp]),
    "ohgpu_mp4_batch_run": _RUN_SRC,
    "ohgpu_mp4_batch_results": _FETCH,
    "ohgpu_mp4_batch_packets": _FETCH,
    "ohgpu_mp4_batch_samples": _FETCH,
    "ohgpu_mp4_batch_phase_ms": _PHASE_MS,
    "ohgpu_mp4_process_host": (_int, [_vp, _vp, _sz, _sz, _vp, _u64, _vp, _vp, _vp]),
    "ohgpu_mp4_seek": (_int, [_vp, _sz, _u64, _u64p, _u64p]),
    "ohgpu_mp4_alac_process_host": (_int, [_vp, _vp, _vp, _sz, _sz, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "ohgpu_mp4f_batch_check": _FRAG_CHECK,
    "ohgpu_mp4f_batch_create": _FRAG_CREATE,
    "ohgpu_mp4f_batch_run": _RUN,
    "ohgpu_mp4f_batch_results": _FETCH,
    "ohgpu_mp4f_batch_runs": _FETCH,
    "ohgpu_mp4f_batch_packets": _FETCH,
    "ohgpu_mp4f_batch_samples": _FETCH,
    "ohgpu_mp4f_batch_phase_ms": _PHASE_MS,
    "ohgpu_mp4f_batch_paths": _PATHS,
    "ohgpu_mp4f_head": _HEAD,
    "ohgpu_mp4f_process_host": _FRAG_HOST,
    "ohgpu_mp4f_flac_process_host": _FRAG_FLAC_HOST,
    "ohgpu_mp4f_alac_process_host": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ohgpu_iff_batch_check": _CHECK,
    "ohgpu_iff_batch_create": _CREATE,
    "ohgpu_iff_batch_run": _RUN,
    "ohgpu_iff_batch_results": _FETCH,
    "ohgpu_iff_batch_phase_ms": _PHASE_MS,
    "ohgpu_iff_process_host": _HOST_RESULTS,
    "ohgpu_dsd_file_batch_check": _CHECK,
    "ohgpu_dsd_file_batch_create": _CREATE,
    "ohgpu_dsd_file_batch_run": _RUN,
    "ohgpu_dsd_file_batch_results": _FETCH,
    "ohgpu_dsd_file_batch_phase_ms": _PHASE_MS,
    "ohgpu_dsd_file_process_host": _HOST_RESULTS,
    "ohgpu_dsd_file_head": (_int, [_vp, _u64, _u32, _u32, _vp]),
    "ohgpu_dsd_file_seek": (_int, [_u32, _u64, _u64p, _u64p]),
    "ohgpu_ogg_crc": (_u32, [_vp, _sz]),
    "ohgpu_ogg_flac_head": (_int, [_vp, _sz, _vp, _u32p, _u64p, _u32p, _u32p]),
    "ohgpu_ogg_flac_process_host": (_int, [_vp, _vp, _vp, _sz, _sz, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _sz, _szp]),
    "ohgpu_flywheel_batch_create": _CREATE,
    "ohgpu_flywheel_batch_run": _RUN,
    "ohgpu_flywheel_process_host": _HOST,
    "ohgpu_ohm_frame_layout": (_int, [_vp, _u32, _u32p, _u32p]),
    "ohgpu_ohm_batch_create": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _u64, _u64, _vpp]),
    "ohgpu_ohm_batch_run": _RUN,
    "ohgpu_ohm_process_host": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _u64, _vp, _u64]),
    "ohgpu_src_design": (_int, [_u32, _u32, _u32, _dbl, _dbl, _vp, _sz, _u32p, _u32p]),
    "ohgpu_src_create": (_int, [_vp, _u32, _u32, _u32, _vp, _vpp]),
    "ohgpu_src_destroy": _HANDLE,
    "ohgpu_src_out_frames": (_u64, [_u32, _u32, _u64]),
    "ohgpu_src_mfma_tables": (_int, [_u32, _u32, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _szp, _szp, _u32p]),
    "ohgpu_src_mfma_halfband_tables": (_int, [_vp, _vp, C.POINTER(C.c_int64), _u32p]),
    "ohgpu_src_batch_create": _CREATE_FILTER,
    "ohgpu_src_batch_run": _RUN,
    "ohgpu_src_batch_run_timed": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ohgpu_src_batch_plan": (_int, [_vp, _u64p, _u64p]),
    "ohgpu_src_batch_units": (_int, [_vp, _u64p, _u64p]),
    "ohgpu_set_plan_threads": (_int, [_int]),
    "ohgpu_src_batch_block": _PATHS_PAIR,
    "ohgpu_src_batch_advance": (_int, [_vp, _vp, _u64]),
    "ohgpu_src_batch_set_ramps": (_int, [_vp, _vp, _vp, _vp, _sz]),
    "ohgpu_src_plan_digest": (_int, [_u32, _u32, _u32, _vp, _sz, _u64, _u64, _int, _vp, _int, _u64p, _u64p, _u64p, _intp]),
    "ohgpu_src_batch_kernel_name": (_int, [_vp, _vp, _str, _sz]),
    "ohgpu_src_batch_occupancy": (_int, [_vp, _vp, _intp, _intp, _u32p]),
    "ohgpu_measure_shader_clock": (_int, [_vp, _vp, C.POINTER(C.c_double)]),
    "ohgpu_device_allocations": (_int, [_vp, _u64p]),
    "ohgpu_src_process_host": _HOST_FILTER,
    "ohgpu_host_transfer_stats": (_int, [_vp, _u64p, _u64p, _u64p, _u64p]),
    "ohgpu_set_kernel_variant": (_int, [_vp, _int]),
    "ohgpu_src_pull_design": (_int, [_u32, _u32, _u32, _u32, _dbl, _dbl, _dbl, _vp, _sz]),
    "ohgpu_src_pull_step": (_int, [_u32, _u32, _u32, _u64p]),
    "ohgpu_src_pull_window": (_int, [_u64, _u32, _u64, _u32, _u32, _u64p, _u64p]),
    "ohgpu_src_pull_create": (_int, [_vp, _u32, _u32, _vp, _vpp]),
    "ohgpu_src_pull_destroy": _HANDLE,
    "ohgpu_src_pull_batch_create": _CREATE_FILTER,
    "ohgpu_src_pull_batch_run": _RUN,
    "ohgpu_src_pull_process_host": _HOST_FILTER,
}
# include/ohgpu_cenc.h: protected fragmented MPEG-4, ohgpu_mp4f_*'s calls with a key in the descriptor
CENC_SYMBOLS = {
    "ohgpu_cenc_batch_check": _FRAG_CHECK,
    "ohgpu_cenc_batch_create": _FRAG_CREATE,
    "ohgpu_cenc_batch_run": _RUN,
    "ohgpu_cenc_batch_results": _FETCH,
    "ohgpu_cenc_batch_runs": _FETCH,
    "ohgpu_cenc_batch_packets": _FETCH,
    "ohgpu_cenc_batch_samples": _FETCH,
    "ohgpu_cenc_batch_phase_ms": _PHASE_MS,
    "ohgpu_cenc_batch_paths": _PATHS,
    "ohgpu_cenc_head": _HEAD,
    "ohgpu_cenc_process_host": _FRAG_HOST,
    "ohgpu_cenc_flac_process_host": _FRAG_FLAC_HOST,
    "ohgpu_cenc_alac_process_host": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# include/ohgpu_cbcs.h: ohgpu_cenc_*'s calls with a batch-wide n_subsamples behind n_runs
CBCS_SYMBOLS = {
    "ohgpu_cbcs_batch_check": (_int, [_vp, _sz, _sz, _sz, _sz, _u64, _u64]),
    "ohgpu_cbcs_batch_create": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _u64, _u64, _vpp]),
    "ohgpu_cbcs_batch_run": _RUN,
    "ohgpu_cbcs_batch_results": _FETCH,
    "ohgpu_cbcs_batch_runs": _FETCH,
    "ohgpu_cbcs_batch_packets": _FETCH,
    "ohgpu_cbcs_batch_samples": _FETCH,
    "ohgpu_cbcs_batch_phase_ms": _PHASE_MS,
    "ohgpu_cbcs_batch_paths": _PATHS,
    "ohgpu_cbcs_head": _HEAD,
    "ohgpu_cbcs_process_host": (_int, [_vp, _vp, _sz, _sz, _sz, _sz, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "ohgpu_cbcs_flac_process_host": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _szp]),
    "ohgpu_cbcs_alac_process_host": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# include/ohgpu_raop_rx.h
RAOP_RX_SYMBOLS = {
    "ohgpu_raop_rx_batch_check": (_int, [_vp, _sz, _vp, _sz, _u64]),
    "ohgpu_raop_rx_batch_create": (_int, [_vp, _vp, _sz, _vp, _sz, _u64, _vpp]),
    "ohgpu_raop_rx_batch_run": _RUN_SRC,
    "ohgpu_raop_rx_batch_results": _FETCH_PAIR,
    "ohgpu_raop_rx_batch_packets": _FETCH,
    "ohgpu_raop_rx_batch_phase_ms": _PHASE_MS,
    "ohgpu_raop_rx_process_host": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u64, _vp, _vp, _vp]),
    "ohgpu_raop_rx_alac_process_host": (_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
}
# include/ohgpu_ts.h
TS_SYMBOLS = {
    "ohgpu_ts_batch_check": (_int, [_vp, _sz, _sz, _u64, _u64]),
    "ohgpu_ts_batch_create": (_int, [_vp, _vp, _sz, _sz, _u64, _u64, _vpp]),
    "ohgpu_ts_batch_run": _RUN,
    "ohgpu_ts_batch_results": _FETCH,
    "ohgpu_ts_batch_pes": _FETCH,
    "ohgpu_ts_batch_phase_ms": _PHASE_MS,
    "ohgpu_ts_batch_paths": _PATHS,
    "ohgpu_ts_process_host": (_int, [_vp, _vp, _sz, _sz, _vp, _u64, _vp, _u64, _vp, _vp]),
    "ohgpu_ts_crc": (_u32, [_vp, _sz]),
    "ohgpu_adts_batch_check": (_int, [_vp, _sz, _sz, _u64]),
    "ohgpu_adts_batch_create": (_int, [_vp, _vp, _sz, _sz, _u64, _vpp]),
    "ohgpu_adts_batch_run": _RUN_SRC,
    "ohgpu_adts_batch_results": _FETCH,
    "ohgpu_adts_batch_frames": _FETCH,
    "ohgpu_adts_batch_phase_ms": _PHASE_MS,
    "ohgpu_adts_batch_paths": _PATHS_PAIR,
    "ohgpu_adts_process_host": (_int, [_vp, _vp, _sz, _sz, _vp, _u64, _vp, _vp]),
    "ohgpu_adts_header": _HEAD,
    "ohgpu_id3v2_skip": (_u64, [_vp, _sz]),
    "ohgpu_ts_adts_process_host": (_int, [_vp, _vp, _vp, _sz, _sz, _sz, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
}
# include/ohgpu_vorbis.h
VORBIS_SYMBOLS = {
    "ohgpu_vorbis_setup_parse": (_int, [_vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "ohgpu_vorbis_codewords": _HEAD,
    "ohgpu_vorbis_batch_check": (_int, [_vp, _sz, _vp, _sz, _vp, _u64, _u64, _u64]),
    "ohgpu_vorbis_batch_create": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u64, _u64, _u64, _vpp]),
    "ohgpu_vorbis_batch_run": _RUN,
    "ohgpu_vorbis_batch_results": _FETCH_PAIR,
    "ohgpu_vorbis_batch_phase_ms": _PHASE_MS,
    "ohgpu_vorbis_batch_paths": _PATHS_PAIR,
    "ohgpu_vorbis_batch_spectrum": (_int, [_vp, _vp, _sz, _u32, _vp, _sz]),
    "ohgpu_vorbis_head": (_int, [_vp, _sz, _vp, _sz, _vp, _u32p, _u64p, _u32p, _u32p]),
    "ohgpu_ogg_vorbis_process_host": (_int, [_vp, _vp, _vp, _sz, _sz, _vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "ohgpu_vorbis_process_host": (_int, [_vp, _vp, _sz, _vp, _sz, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    "ohgpu_ogg_vorbis_links_process_host": (_int, [_vp, _vp, _vp, _vp, _sz, _sz, _vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _sz, _szp, _vp]),
}
# the registry: header file name -> its table.  A header that is not entered here fails tests/test_capi_loads.py.
ABI_TABLES = {"ohgpu.h": SYMBOLS, "ohgpu_cenc.h": CENC_SYMBOLS, "ohgpu_cbcs.h": CBCS_SYMBOLS, "ohgpu_raop_rx.h": RAOP_RX_SYMBOLS,
              "ohgpu_ts.h": TS_SYMBOLS, "ohgpu_vorbis.h": VORBIS_SYMBOLS}


class OhGpuError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"ohgpu error {code}: {message}")
        self.code = code


_lib = None


def lib():
    """Loads libohgpu.so (build it first with `python -m ohpipeline_amd.build` or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build the HIP extension first (python ohpipeline_amd/build.py); "
                          "there is no CPU fallback for the product path")
    L = C.CDLL(LIB_PATH)
    for table in ABI_TABLES.values():
        for name, (res, args) in table.items():
            fn = getattr(L, name)          # AttributeError here = the library does not export what its header declares
            fn.restype = res
            fn.argtypes = args
    _lib = L
    return L


def last_error():
    return lib().ohgpu_last_error().decode("utf-8", "replace")


def check(code):
    if code != OK:
        raise OhGpuError(code, last_error())
    return code


# ---- the marshalling layer: what every family's calls below are made of.  The *_run methods do not go through it: they are one direct
# call each, because they sit inside timed loops.
def _typed(a, dtype):
    """A table as the library reads it: contiguous, and of the records the entry expects."""
    a = np.ascontiguousarray(a)
    assert a.dtype == dtype
    return a


def _ptr(a, keep=False):
    """The address of a table or host buffer.  An empty one goes as a null pointer, which every entry takes with a zero count, except
    the few that refuse a null whatever the count (a filter's coefficients, the ramps, ohgpu_flac_streaminfo's bytes): those `keep`
    the array's own address."""
    return a.ctypes.data_as(C.c_void_p) if keep or a.size else None


def _create(fn, *args):
    """An entry whose last parameter is the handle it makes (a batch, a filter, a stream, an event, memory): the handle."""
    h = C.c_void_p()
    check(fn(*args, C.byref(h)))
    return h


def _fetch(fn, ctx, batch, dtype, n):
    """A table of a batch's last run (ctx, batch, out, n): n records of dtype."""
    out = np.zeros(n, dtype=dtype)
    check(fn(ctx, batch, _ptr(out), n))
    return out


def _fetch_pair(fn, ctx, batch, dtype, n, dtype2, n2):
    """... of the entries that answer two tables in one call (ctx, batch, out, n, out2, n2)."""
    out, out2 = np.zeros(n, dtype=dtype), np.zeros(n2, dtype=dtype2)
    check(fn(ctx, batch, _ptr(out), n, _ptr(out2), n2))
    return out, out2


def _phase_ms(fn, ctx, batch, k):
    """The k phase times of a batch's last run, in milliseconds."""
    ms = (C.c_float * k)()
    check(fn(ctx, batch, ms))
    return tuple(float(v) for v in ms)


def _paths(fn, batch, *keys):
    """A *_batch_paths entry: a uint32 by reference per key, as a dict."""
    v = [C.c_uint32(0) for _ in keys]
    check(fn(batch, *map(C.byref, v)))
    return {k: int(x.value) for k, x in zip(keys, v)}


def _process_host(fn, ctx, args, src, dst, out, mid=(), tail=()):
    """An ohgpu_*_process_host: `args` (the tables' pointers and the counts, in the entry's order), the source buffer, `mid` (the size
    of a middle arena, where the entry has one), the destination buffer unless dst is None (a family that writes to no arena), the
    result tables `out`, which it returns, and whatever the entry has behind them."""
    bufs = (_ptr(src), src.nbytes, *mid) if dst is None else (_ptr(src), src.nbytes, *mid, _ptr(dst), dst.nbytes)
    check(fn(ctx, *args, *bufs, *map(_ptr, out), *tail))
    return out


def _head(fn, data, dtype):
    """A host-only parse of leading bytes into one record (bytes, n, record out)."""
    raw, out = bytes(data), np.zeros(1, dtype=dtype)
    check(fn(raw, len(raw), _ptr(out)))
    return out[0]


def ramp_table():
    out = (C.c_uint16 * 512)()
    check(lib().ohgpu_ramp_table(out))
    return np.frombuffer(out, dtype=np.uint16).copy()


def device_count():
    """GPUs visible to the process (ohgpu_device_count); 0 without one."""
    n = lib().ohgpu_device_count()
    return max(int(n), 0)


def set_plan_threads(threads):
    check(lib().ohgpu_set_plan_threads(int(threads)))


def src_plan_digest(L, M, T, descs, src_arena_bytes, dst_arena_bytes, kernel_variant=0, coef_q28=None, num_cus=0):
    """The plan ohgpu_src_batch_create would make, hashed on the host (no device): {digest, units, generic_pieces, kernel}.
    coef_q28: the filter's coefficients (the plan then is exactly a real batch's: half-band form, tables, gain); None = a plain
    polyphase filter of sane gain.  num_cus: the device's CU count (0 = 256)."""
    d = np.ascontiguousarray(descs)
    coef = None if coef_q28 is None else np.ascontiguousarray(coef_q28, dtype=np.int32)
    h, u, p, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    check(lib().ohgpu_src_plan_digest(L, M, T, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes, kernel_variant,
                                      None if coef is None else _ptr(coef, keep=True), num_cus,
                                      C.byref(h), C.byref(u), C.byref(p), C.byref(k)))
    return {"digest": int(h.value), "units": int(u.value), "generic_pieces": int(p.value), "kernel": int(k.value)}


def src_mfma_tables(L, M, T, coef_q28, max_blocks_per_row=8):
    """(digits [4][L][96] int8, steps MF_STEP[], outputs per block) -- the matrix-pipe resampler kernel's host tables (no device)."""
    coef = np.ascontiguousarray(coef_q28, dtype=np.int32)
    nb, ns, lb = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0)
    check(lib().ohgpu_src_mfma_tables(L, M, T, _ptr(coef, keep=True), max_blocks_per_row, None, 0, None, 0, C.byref(nb), C.byref(ns), C.byref(lb)))
    dig = np.zeros(nb.value, dtype=np.int8)
    steps = np.zeros(ns.value // MF_STEP.itemsize, dtype=MF_STEP)
    check(lib().ohgpu_src_mfma_tables(L, M, T, _ptr(coef, keep=True), max_blocks_per_row, _ptr(dig), dig.nbytes, _ptr(steps), steps.nbytes,
                                      C.byref(nb), C.byref(ns), C.byref(lb)))
    return dig.reshape(4, L, 96), steps, lb.value


def src_mfma_halfband_tables(coef_q28):
    """(image [4 digits][4 K groups][16 outputs][16] int8, bias, outputs per block) -- the half-band form's host tables (no device)."""
    coef = np.ascontiguousarray(coef_q28, dtype=np.int32)
    image = np.zeros(4096, dtype=np.int8)
    bias, lb = C.c_int64(0), C.c_uint32(0)
    check(lib().ohgpu_src_mfma_halfband_tables(_ptr(coef, keep=True), _ptr(image), C.byref(bias), C.byref(lb)))
    return image.reshape(4, 4, 16, 16), int(bias.value), int(lb.value)


def src_design(rate_in, rate_out, taps_per_phase=32, beta=9.0, f_pass=20000.0):
    """Returns (L, M, coef_q28[L*T]) from the library's own host-side filter design."""
    L_, M_ = C.c_uint32(0), C.c_uint32(0)
    check(lib().ohgpu_src_design(rate_in, rate_out, taps_per_phase, beta, f_pass, None, 0, C.byref(L_), C.byref(M_)))
    coef = np.zeros(L_.value * taps_per_phase, dtype=np.int32)
    check(lib().ohgpu_src_design(rate_in, rate_out, taps_per_phase, beta, f_pass, _ptr(coef), coef.size, C.byref(L_), C.byref(M_)))
    return L_.value, M_.value, coef


def src_pull_design(rate_in, rate_out, taps_per_phase=32, phases_log2=8, beta=8.0, f_pass=20000.0, max_pull=0.001):
    """The pulled resampler's Q28 table, shape (2^phases_log2 + 1, taps_per_phase) (ohgpu_src_pull_design; host only)."""
    rows = (1 << phases_log2) + 1 if 0 <= phases_log2 <= 16 else 1
    coef = np.zeros(rows * taps_per_phase, dtype=np.int32)
    check(lib().ohgpu_src_pull_design(rate_in, rate_out, taps_per_phase, phases_log2, beta, f_pass, max_pull, _ptr(coef, keep=True), coef.size))
    return coef.reshape(rows, taps_per_phase)


def src_pull_step(rate_in, rate_out, multiplier=SRC_PULL_NOMINAL):
    """floor(2 * rate_in * multiplier / rate_out): Q32.32 input frames per output frame (ohgpu_src_pull_step; host only)."""
    st = C.c_uint64(0)
    check(lib().ohgpu_src_pull_step(rate_in, rate_out, multiplier, C.byref(st)))
    return int(st.value)


def src_pull_window(pos_frame, pos_frac, step, n_frames, taps_per_phase):
    """(first, frames): the input frames a pulled message reads (ohgpu_src_pull_window; host only)."""
    first, frames = C.c_uint64(0), C.c_uint64(0)
    check(lib().ohgpu_src_pull_window(pos_frame, pos_frac, step, n_frames, taps_per_phase, C.byref(first), C.byref(frames)))
    return int(first.value), int(frames.value)


def dsd_layout(kind, sample_block_words, pad_bytes_per_chunk, n_chunks):
    """(source bytes, destination bytes) of a DSD descriptor, or OhGpuError(ERR_INVALID) (ohgpu_dsd_layout; host only)."""
    s, d = C.c_uint64(0), C.c_uint64(0)
    check(lib().ohgpu_dsd_layout(kind, sample_block_words, pad_bytes_per_chunk, n_chunks, C.byref(s), C.byref(d)))
    return int(s.value), int(d.value)


def dsd_pcm_design(dsd_rate, pcm_rate, taps_per_output=16, beta=14.0, f_pass=20000.0, gain=1.0):
    """(D, coef_q28[D * T]) from the library's own host-side decimator design (ohgpu_dsd_pcm_design; host only)."""
    D = C.c_uint32(0)
    check(lib().ohgpu_dsd_pcm_design(dsd_rate, pcm_rate, taps_per_output, beta, f_pass, gain, None, 0, C.byref(D)))
    coef = np.zeros(D.value * taps_per_output, dtype=np.int32)
    check(lib().ohgpu_dsd_pcm_design(dsd_rate, pcm_rate, taps_per_output, beta, f_pass, gain, _ptr(coef), coef.size, C.byref(D)))
    return D.value, coef


def dsd_pcm_window(out_frame0, n_frames, decimation, taps_per_output):
    """(chunk_lo, chunk_hi): the chunks a converted message reads (ohgpu_dsd_pcm_window; host only)."""
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    check(lib().ohgpu_dsd_pcm_window(out_frame0, n_frames, decimation, taps_per_output, C.byref(lo), C.byref(hi)))
    return int(lo.value), int(hi.value)


def dsd_pcm_batch_check(decimation, taps_per_output, descs, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.dsd_pcm_batch without a device (ohgpu_dsd_pcm_batch_check): OhGpuError on a bad descriptor."""
    d = _typed(descs, DSD_PCM_MSG_DESC)
    check(lib().ohgpu_dsd_pcm_batch_check(decimation, taps_per_output, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes))


def flac_streaminfo(stream):
    """(STREAMINFO as a dict, offset of the first frame) of a FLAC stream's first bytes (ohgpu_flac_streaminfo; host only)."""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    info = np.zeros(1, dtype=FLAC_STREAMINFO)
    off = C.c_uint64(0)
    check(lib().ohgpu_flac_streaminfo(_ptr(buf, keep=True), buf.size, _ptr(info), C.byref(off)))
    i = info[0]
    return ({k: int(i[k]) for k in ("min_blocksize", "max_blocksize", "sample_rate", "channels", "bits", "total_samples",
                                    "min_framesize", "max_framesize")} | {"md5": bytes(i["md5"])}, int(off.value))


def flac_batch_check(descs, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.flac_batch without a device (ohgpu_flac_batch_check): OhGpuError on a bad descriptor."""
    d = _typed(descs, FLAC_STREAM_DESC)
    check(lib().ohgpu_flac_batch_check(_ptr(d), d.size, src_arena_bytes, dst_arena_bytes))


def alac_config_parse(cookie):
    """The stream configuration (ALAC_CONFIG, one record) of a magic cookie, atom wrappers and all (ohgpu_alac_config_parse; host only)."""
    buf = np.frombuffer(bytes(cookie), dtype=np.uint8)
    cfg = np.zeros(1, dtype=ALAC_CONFIG)
    check(lib().ohgpu_alac_config_parse(_ptr(buf), buf.size, _ptr(cfg)))
    return cfg[0]


def alac_batch_check(descs, packets, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.alac_batch without a device (ohgpu_alac_batch_check): OhGpuError on a bad descriptor."""
    d, p = _typed(descs, ALAC_STREAM_DESC), _typed(packets, ALAC_PACKET)
    check(lib().ohgpu_alac_batch_check(_ptr(d), d.size, _ptr(p), p.size, src_arena_bytes, dst_arena_bytes))


def raop_fmtp_parse(fmtp):
    """The stream configuration (ALAC_CONFIG, one record) of an SDP fmtp string (ohgpu_raop_fmtp_parse; host only)."""
    return _head(lib().ohgpu_raop_fmtp_parse, fmtp.encode("ascii") if isinstance(fmtp, str) else fmtp, ALAC_CONFIG)


def raop_batch_check(descs, packets, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.raop_batch without a device (ohgpu_raop_batch_check): OhGpuError on a bad descriptor."""
    d, p = _typed(descs, RAOP_STREAM_DESC), _typed(packets, ALAC_PACKET)
    check(lib().ohgpu_raop_batch_check(_ptr(d), d.size, _ptr(p), p.size, src_arena_bytes, dst_arena_bytes))


def ohm_rx_batch_check(streams, datagrams, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.ohm_rx_batch without a device (ohgpu_ohm_rx_batch_check): OhGpuError on a bad table."""
    s, g = _typed(streams, OHM_RX_STREAM), _typed(datagrams, OHM_RX_DATAGRAM)
    check(lib().ohgpu_ohm_rx_batch_check(_ptr(s), s.size, _ptr(g), g.size, src_arena_bytes, dst_arena_bytes))


def raop_rx_batch_check(streams, datagrams, src_arena_bytes):
    """The validation of ctx.raop_rx_batch without a device (ohgpu_raop_rx_batch_check): OhGpuError on a bad table."""
    s, g = _typed(streams, RAOP_RX_STREAM), _typed(datagrams, RAOP_RX_DATAGRAM)
    check(lib().ohgpu_raop_rx_batch_check(_ptr(s), s.size, _ptr(g), g.size, src_arena_bytes))


def vorbis_setup_parse(id_packet, setup_packet):
    """The setup image of a stream's identification and setup header packets (ohgpu_vorbis_setup_parse; host only): (image as uint8, info)."""
    a, b = bytes(id_packet), bytes(setup_packet)
    info = np.zeros(1, dtype=VORBIS_INFO)
    check(lib().ohgpu_vorbis_setup_parse(a, len(a), b, len(b), None, 0, _ptr(info)))
    image = np.zeros(int(info["image_bytes"][0]), dtype=np.uint8)
    check(lib().ohgpu_vorbis_setup_parse(a, len(a), b, len(b), _ptr(image), image.size, _ptr(info)))
    return image, info[0]


def vorbis_head(data):
    """The head of an Ogg Vorbis stream (ohgpu_vorbis_head; host only): dict(image, info, serial, page_offset, segment, seq) -- where the
    first audio packet begins."""
    raw = bytes(data)
    info = np.zeros(1, dtype=VORBIS_INFO)
    serial, seg, seq, off = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    check(lib().ohgpu_vorbis_head(raw, len(raw), None, 0, _ptr(info), C.byref(serial), C.byref(off), C.byref(seg), C.byref(seq)))
    image = np.zeros(int(info["image_bytes"][0]), dtype=np.uint8)
    check(lib().ohgpu_vorbis_head(raw, len(raw), _ptr(image), image.size, _ptr(info), C.byref(serial), C.byref(off), C.byref(seg), C.byref(seq)))
    return dict(image=image, info=info[0], serial=int(serial.value), page_offset=int(off.value), segment=int(seg.value), seq=int(seq.value))


def vorbis_codewords(lengths):
    """The codewords of a list of lengths, 0 for an unused entry (ohgpu_vorbis_codewords; host only)."""
    l = np.ascontiguousarray(lengths, dtype=np.uint8)
    out = np.zeros(l.size, dtype=np.uint32)
    check(lib().ohgpu_vorbis_codewords(_ptr(l), l.size, _ptr(out)))
    return out


def vorbis_batch_check(descs, packets, images, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.vorbis_batch without a device (ohgpu_vorbis_batch_check): OhGpuError on a bad descriptor."""
    d, p, im = _typed(descs, VORBIS_STREAM_DESC), _typed(packets, ALAC_PACKET), _typed(images, np.uint8)
    check(lib().ohgpu_vorbis_batch_check(_ptr(d), d.size, _ptr(p), p.size, _ptr(im), im.size, src_arena_bytes, dst_arena_bytes))


def ts_batch_check(descs, n_pes, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.ts_batch without a device (ohgpu_ts_batch_check): OhGpuError on a bad descriptor."""
    d = _typed(descs, TS_STREAM_DESC)
    check(lib().ohgpu_ts_batch_check(_ptr(d), d.size, n_pes, src_arena_bytes, dst_arena_bytes))


def adts_batch_check(descs, n_frames, src_arena_bytes):
    """The validation of ctx.adts_batch without a device (ohgpu_adts_batch_check)."""
    d = _typed(descs, ADTS_STREAM_DESC)
    check(lib().ohgpu_adts_batch_check(_ptr(d), d.size, n_frames, src_arena_bytes))


def ts_crc(data):
    """The section CRC-32 of any bytes (ohgpu_ts_crc; host only)."""
    raw = bytes(data)
    return int(lib().ohgpu_ts_crc(raw, len(raw)))


def adts_header(data):
    """One ADTS header (ohgpu_adts_header; host only): an ADTS_FRAME record, or None where the bytes begin with no valid header."""
    raw, out = bytes(data), np.zeros(1, dtype=ADTS_FRAME)
    return out[0] if lib().ohgpu_adts_header(raw, len(raw), _ptr(out)) == OK else None


def id3v2_skip(data):
    """The bytes of the ID3v2 tags at the head of a buffer (ohgpu_id3v2_skip; host only); 0: no tag."""
    raw = bytes(data)
    return int(lib().ohgpu_id3v2_skip(raw, len(raw)))


def ogg_batch_check(descs, n_packets, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.ogg_batch without a device (ohgpu_ogg_batch_check): OhGpuError on a bad descriptor."""
    d = _typed(descs, OGG_STREAM_DESC)
    check(lib().ohgpu_ogg_batch_check(_ptr(d), d.size, n_packets, src_arena_bytes, dst_arena_bytes))


def ogg_crc(data):
    """The Ogg page checksum of any bytes (ohgpu_ogg_crc; host only)."""
    raw = bytes(data)
    return int(lib().ohgpu_ogg_crc(raw, len(raw)))


def ogg_flac_head(data):
    """The head of an Ogg FLAC stream (ohgpu_ogg_flac_head; host only): (FLAC_STREAMINFO record, serial, audio page offset, audio
    segment, audio page number)."""
    raw = bytes(data)
    info = np.zeros(1, dtype=FLAC_STREAMINFO)
    serial, seg, seq, off = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
    check(lib().ohgpu_ogg_flac_head(raw, len(raw), _ptr(info), C.byref(serial), C.byref(off), C.byref(seg), C.byref(seq)))
    return info[0], int(serial.value), int(off.value), int(seg.value), int(seq.value)


def mp4_batch_check(descs, n_packets, src_arena_bytes):
    """The validation of ctx.mp4_batch without a device (ohgpu_mp4_batch_check): OhGpuError on a bad descriptor."""
    d = _typed(descs, MP4_STREAM_DESC)
    check(lib().ohgpu_mp4_batch_check(_ptr(d), d.size, n_packets, src_arena_bytes))


def mp4_seek(samples, frame):
    """The row of a sample table (MP4_SAMPLE) that holds audio frame `frame` (ohgpu_mp4_seek; host only): (index, its first frame)."""
    t = _typed(samples, MP4_SAMPLE)
    index, first = C.c_uint64(0), C.c_uint64(0)
    check(lib().ohgpu_mp4_seek(_ptr(t), t.size, frame, C.byref(index), C.byref(first)))
    return int(index.value), int(first.value)


# The three fragmented MPEG-4 families behind one implementation (Context._frag_* has the device calls): a family's descriptor and
# result records; `counts` is (n_packets, n_runs), with n_subsamples behind them for cbcs.
_FRAG = {"mp4f": (MP4F_STREAM_DESC, MP4F_STREAM_RESULT), "cenc": (CENC_STREAM_DESC, CENC_STREAM_RESULT), "cbcs": (CBCS_STREAM_DESC, CBCS_STREAM_RESULT)}


def _frag_fn(fam, name):
    return getattr(lib(), f"ohgpu_{fam}_{name}")


def _frag_batch_check(fam, descs, counts, src_arena_bytes, dst_arena_bytes):
    d = _typed(descs, _FRAG[fam][0])
    check(_frag_fn(fam, "batch_check")(_ptr(d), d.size, *counts, src_arena_bytes, dst_arena_bytes))


def _frag_zeros(fam, n, n_packets, n_runs):
    return np.zeros(n, dtype=_FRAG[fam][1]), np.zeros(n_runs, dtype=MP4F_RUN), np.zeros(n_packets, dtype=ALAC_PACKET), np.zeros(n_packets, dtype=MP4_SAMPLE)


def mp4f_batch_check(descs, n_packets, n_runs, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.mp4f_batch without a device (ohgpu_mp4f_batch_check): OhGpuError on a bad descriptor."""
    _frag_batch_check("mp4f", descs, (n_packets, n_runs), src_arena_bytes, dst_arena_bytes)


def mp4f_head(data):
    """The walk of a fragmented stream up to the end of moov (ohgpu_mp4f_head; host only): an MP4F_STREAM_RESULT record."""
    return _head(lib().ohgpu_mp4f_head, data, MP4F_STREAM_RESULT)


def cenc_batch_check(descs, n_packets, n_runs, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.cenc_batch without a device (ohgpu_cenc_batch_check): OhGpuError on a bad descriptor."""
    _frag_batch_check("cenc", descs, (n_packets, n_runs), src_arena_bytes, dst_arena_bytes)


def cenc_head(data):
    """The walk of a protected or clear fragmented stream up to the end of moov (ohgpu_cenc_head; host only, no key): a CENC_STREAM_RESULT
    record whose is_protected and kid say which key to ask for."""
    return _head(lib().ohgpu_cenc_head, data, CENC_STREAM_RESULT)


def cbcs_batch_check(descs, n_packets, n_runs, n_subsamples, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.cbcs_batch without a device (ohgpu_cbcs_batch_check): OhGpuError on a bad descriptor."""
    _frag_batch_check("cbcs", descs, (n_packets, n_runs, n_subsamples), src_arena_bytes, dst_arena_bytes)


def cbcs_head(data):
    """The walk of a `cenc`- or `cbcs`-protected or clear fragmented stream up to the end of moov (ohgpu_cbcs_head; host only, no key): a
    CBCS_STREAM_RESULT record."""
    return _head(lib().ohgpu_cbcs_head, data, CBCS_STREAM_RESULT)


def iff_batch_check(descs, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.iff_batch without a device (ohgpu_iff_batch_check): OhGpuError on a bad descriptor."""
    d = _typed(descs, IFF_STREAM_DESC)
    check(lib().ohgpu_iff_batch_check(_ptr(d), d.size, src_arena_bytes, dst_arena_bytes))


def dsd_file_batch_check(descs, src_arena_bytes, dst_arena_bytes):
    """The validation of ctx.dsd_file_batch without a device (ohgpu_dsd_file_batch_check): OhGpuError on a bad descriptor."""
    d = _typed(descs, DSD_FILE_STREAM_DESC)
    check(lib().ohgpu_dsd_file_batch_check(_ptr(d), d.size, src_arena_bytes, dst_arena_bytes))


def dsd_file_head(data, sample_block_words, pad_bytes_per_chunk):
    """The walk over a file's bytes on the host (ohgpu_dsd_file_head): one DSD_FILE_STREAM_RESULT record."""
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    res = np.zeros(1, dtype=DSD_FILE_STREAM_RESULT)
    check(lib().ohgpu_dsd_file_head(_ptr(raw), raw.size, sample_block_words, pad_bytes_per_chunk, _ptr(res)))
    return res[0]


def dsd_file_seek(kind, sample):
    """(chunk_first, sample_rounded) of a seek to `sample` (ohgpu_dsd_file_seek)."""
    first, rounded = C.c_uint64(0), C.c_uint64(0)
    check(lib().ohgpu_dsd_file_seek(kind, sample, C.byref(first), C.byref(rounded)))
    return int(first.value), int(rounded.value)


class Context:
    """One GPU context (ohgpu_ctx).  Owns device allocations made through it."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().ohgpu_init(device, C.byref(self._h)))
        self.device = device

    @property
    def handle(self):
        return self._h

    def name(self):
        buf = C.create_string_buffer(128)
        check(lib().ohgpu_device_name(self._h, buf, 128))
        return buf.value.decode()

    def close(self):
        if self._h:
            lib().ohgpu_shutdown(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- memory
    def malloc(self, nbytes):
        return _create(lib().ohgpu_malloc, self._h, nbytes)

    def free(self, dptr):
        check(lib().ohgpu_free(self._h, dptr))

    def stream_create(self):
        return _create(lib().ohgpu_stream_create, self._h)

    def stream_destroy(self, stream):
        check(lib().ohgpu_stream_destroy(self._h, stream))

    def malloc_host(self, nbytes):
        """Pinned host memory as a uint8 array (free with free_host(array))."""
        p = _create(lib().ohgpu_malloc_host, self._h, max(nbytes, 1))
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(nbytes, 1),))[:nbytes]
        return a

    def free_host(self, array):
        check(lib().ohgpu_free_host(self._h, C.c_void_p(array.ctypes.data)))

    def copy_h2d(self, dptr, array, stream=None):
        check(lib().ohgpu_memcpy_h2d(self._h, dptr, _ptr(array), array.nbytes, stream))

    def copy_d2h(self, array, dptr, stream=None):
        check(lib().ohgpu_memcpy_d2h(self._h, _ptr(array), dptr, array.nbytes, stream))

    def upload(self, array, stream=None):
        a = np.ascontiguousarray(array)
        p = self.malloc(max(a.nbytes, 1))
        check(lib().ohgpu_memcpy_h2d(self._h, p, _ptr(a), a.nbytes, stream))
        self.sync(stream)
        return p

    def download(self, dptr, nbytes, stream=None):
        out = np.empty(nbytes, dtype=np.uint8)
        check(lib().ohgpu_memcpy_d2h(self._h, _ptr(out), dptr, nbytes, stream))
        self.sync(stream)
        return out

    def memset(self, dptr, value, nbytes, stream=None):
        check(lib().ohgpu_memset(self._h, dptr, value, nbytes, stream))

    def sync(self, stream=None):
        check(lib().ohgpu_stream_sync(self._h, stream))

    def set_kernel_variant(self, v):
        check(lib().ohgpu_set_kernel_variant(self._h, v))

    # ---- events (HIP events on the launch stream)
    def event(self):
        return _create(lib().ohgpu_event_create, self._h)

    def event_destroy(self, event):
        check(lib().ohgpu_event_destroy(self._h, event))

    def record(self, event, stream=None):
        check(lib().ohgpu_event_record(self._h, event, stream))

    def wait_event(self, stream, event):
        check(lib().ohgpu_stream_wait_event(self._h, stream, event))

    def elapsed_ms(self, start, stop):
        ms = C.c_float(0)
        check(lib().ohgpu_event_elapsed_ms(self._h, start, stop, C.byref(ms)))
        return ms.value

    # ---- batches
    def pcm_batch(self, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, MSG_DESC)
        return _create(lib().ohgpu_pcm_batch_create, self._h, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def pcm_run(self, batch, d_src, d_dst, stream=None):
        check(lib().ohgpu_pcm_batch_run(self._h, batch, d_src, d_dst, stream))

    def batch_destroy(self, batch):
        check(lib().ohgpu_batch_destroy(self._h, batch))

    def batch_info(self, batch):
        v = [C.c_uint64(0) for _ in range(5)]
        check(lib().ohgpu_batch_info(batch, *[C.byref(x) for x in v]))
        keys = ("n_msgs", "in_frames", "out_frames", "src_bytes_touched", "dst_bytes_written")
        return dict(zip(keys, (int(x.value) for x in v)))

    def batch_paths(self, batch):
        """Which kernels a pcm, Songcast frame or fmt batch was planned onto (ohgpu_batch_paths), as a dict of counts."""
        v = np.zeros(1, dtype=BATCH_PATHS)
        check(lib().ohgpu_batch_paths_info(batch, _ptr(v)))
        out = {k: int(v[k][0]) for k in BATCH_PATHS.names if k != "reserved"}
        out["alac_route"] = int(v["reserved"][0][0])        # (the header's union: the last word)
        out["mp4_route"] = out["alac_route"]                 # (the same word: a batch is of one kind)
        out["iff_route"] = out["alac_route"]
        out["dsd_file_route"] = out["alac_route"]
        out["raop_rx_route"] = out["alac_route"]
        out["vorbis_route"] = out["alac_route"]
        return out

    def pcm_process_host(self, descs, src, dst):
        d = _typed(descs, MSG_DESC)
        _process_host(lib().ohgpu_pcm_process_host, self._h, (_ptr(d), d.size), src, dst, ())
        return dst

    def fmt_batch(self, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, FMT_DESC)
        return _create(lib().ohgpu_fmt_batch_create, self._h, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def fmt_run(self, batch, d_src, d_dst, stream=None):
        check(lib().ohgpu_fmt_batch_run(self._h, batch, d_src, d_dst, stream))

    def dsd_batch(self, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, DSD_DESC)
        return _create(lib().ohgpu_dsd_batch_create, self._h, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def dsd_run(self, batch, d_src, d_dst, stream=None):
        check(lib().ohgpu_dsd_batch_run(self._h, batch, d_src, d_dst, stream))

    def dsd_batch_paths(self, batch):
        """How a DSD batch was planned (ohgpu_dsd_batch_paths): descriptors on the wide path, on the byte path, launches."""
        return _paths(lib().ohgpu_dsd_batch_paths, batch, "wide_descs", "generic_descs", "launches")

    def dsd_process_host(self, descs, src, dst):
        d = _typed(descs, DSD_DESC)
        _process_host(lib().ohgpu_dsd_process_host, self._h, (_ptr(d), d.size), src, dst, ())
        return dst

    # ---- DSD -> PCM
    def dsd_pcm_create(self, decimation, taps_per_output, coef_q28):
        c = np.ascontiguousarray(coef_q28, dtype=np.int32)
        assert c.size == decimation * taps_per_output
        return _create(lib().ohgpu_dsd_pcm_create, self._h, decimation, taps_per_output, _ptr(c, keep=True))

    def dsd_pcm_destroy(self, filt):
        check(lib().ohgpu_dsd_pcm_destroy(self._h, filt))

    def dsd_pcm_batch(self, filt, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, DSD_PCM_MSG_DESC)
        return _create(lib().ohgpu_dsd_pcm_batch_create, self._h, filt, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def dsd_pcm_run(self, batch, d_src, d_dst, stream=None):
        check(lib().ohgpu_dsd_pcm_batch_run(self._h, batch, d_src, d_dst, stream))

    def dsd_pcm_batch_paths(self, batch):
        """How a DSD -> PCM batch was planned (ohgpu_dsd_pcm_batch_paths): messages on the fast route, on the plain route, launches."""
        return _paths(lib().ohgpu_dsd_pcm_batch_paths, batch, "fast_descs", "plain_descs", "launches")

    def dsd_pcm_process_host(self, filt, descs, src, dst):
        d = _typed(descs, DSD_PCM_MSG_DESC)
        _process_host(lib().ohgpu_dsd_pcm_process_host, self._h, (filt, _ptr(d), d.size), src, dst, ())
        return dst

    def flac_batch(self, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, FLAC_STREAM_DESC)
        return _create(lib().ohgpu_flac_batch_create, self._h, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def flac_run(self, batch, d_src, d_dst, stream=None):
        """Scan, probe, chain, restore (ohgpu_flac_batch_run): synchronises with the host once, after the scan."""
        check(lib().ohgpu_flac_batch_run(self._h, batch, d_src, d_dst, stream))

    def flac_results(self, batch, n):
        """The last run's FLAC_STREAM_RESULT per stream (waits for the run)."""
        return _fetch(lib().ohgpu_flac_batch_results, self._h, batch, FLAC_STREAM_RESULT, n)

    def flac_frames(self, batch):
        """The last run's delivered frames (FLAC_FRAME), by stream and in stream order."""
        n = C.c_size_t(0)
        check(lib().ohgpu_flac_batch_frames(self._h, batch, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=FLAC_FRAME)
        check(lib().ohgpu_flac_batch_frames(self._h, batch, _ptr(out), out.size, C.byref(n)))
        return out

    def flac_phase_ms(self, batch):
        """The last run's (scan, probe, chain, restore) in milliseconds, from device events."""
        return _phase_ms(lib().ohgpu_flac_batch_phase_ms, self._h, batch, 4)

    def flac_process_host(self, descs, src, dst):
        """Host buffers in and out (ohgpu_flac_process_host); returns the results.  Only decoded samples are written to dst."""
        d = _typed(descs, FLAC_STREAM_DESC)
        res = np.zeros(d.size, dtype=FLAC_STREAM_RESULT)
        return _process_host(lib().ohgpu_flac_process_host, self._h, (_ptr(d), d.size), src, dst, (res,), tail=(None, 0, None))[0]

    def alac_batch(self, descs, packets, src_arena_bytes, dst_arena_bytes):
        d, p = _typed(descs, ALAC_STREAM_DESC), _typed(packets, ALAC_PACKET)
        return _create(lib().ohgpu_alac_batch_create, self._h, _ptr(d), d.size, _ptr(p), p.size, src_arena_bytes, dst_arena_bytes)

    def alac_run(self, batch, d_src, d_dst, stream=None):
        """Entropy, predictor, matrix and store (ohgpu_alac_batch_run): queued on the stream, nothing waits for the host."""
        check(lib().ohgpu_alac_batch_run(self._h, batch, d_src, d_dst, stream))

    def alac_results(self, batch, n, n_packets):
        """The last run's (ALAC_STREAM_RESULT per stream, ALAC_PACKET_RESULT per packet); waits for the run."""
        return _fetch_pair(lib().ohgpu_alac_batch_results, self._h, batch, ALAC_STREAM_RESULT, n, ALAC_PACKET_RESULT, n_packets)

    def alac_phase_ms(self, batch):
        """The last run's (entropy, predictor, matrix and store) in milliseconds, from device events."""
        return _phase_ms(lib().ohgpu_alac_batch_phase_ms, self._h, batch, 3)

    def alac_process_host(self, descs, packets, src, dst):
        """Host buffers in and out (ohgpu_alac_process_host); returns (stream results, packet results).  Only decoded samples are written to dst."""
        d, p = _typed(descs, ALAC_STREAM_DESC), _typed(packets, ALAC_PACKET)
        out = np.zeros(d.size, dtype=ALAC_STREAM_RESULT), np.zeros(p.size, dtype=ALAC_PACKET_RESULT)
        return _process_host(lib().ohgpu_alac_process_host, self._h, (_ptr(d), d.size, _ptr(p), p.size), src, dst, out)

    def raop_batch(self, descs, packets, src_arena_bytes, dst_arena_bytes):
        d, p = _typed(descs, RAOP_STREAM_DESC), _typed(packets, ALAC_PACKET)
        return _create(lib().ohgpu_raop_batch_create, self._h, _ptr(d), d.size, _ptr(p), p.size, src_arena_bytes, dst_arena_bytes)

    def raop_run(self, batch, d_src, d_dst, stream=None):
        """Decrypt, then entropy, predictor, matrix and store (ohgpu_raop_batch_run): queued on the stream; both bases 4-byte aligned."""
        check(lib().ohgpu_raop_batch_run(self._h, batch, d_src, d_dst, stream))

    def raop_results(self, batch, n, n_packets):
        """The last run's (ALAC_STREAM_RESULT per stream, ALAC_PACKET_RESULT per packet); waits for the run."""
        return _fetch_pair(lib().ohgpu_raop_batch_results, self._h, batch, ALAC_STREAM_RESULT, n, ALAC_PACKET_RESULT, n_packets)

    def raop_phase_ms(self, batch):
        """The last run's (decrypt, entropy, predictor, matrix and store) in milliseconds, from device events."""
        return _phase_ms(lib().ohgpu_raop_batch_phase_ms, self._h, batch, 4)

    def raop_process_host(self, descs, packets, src, dst):
        """Host buffers in and out (ohgpu_raop_process_host); returns (stream results, packet results)."""
        d, p = _typed(descs, RAOP_STREAM_DESC), _typed(packets, ALAC_PACKET)
        out = np.zeros(d.size, dtype=ALAC_STREAM_RESULT), np.zeros(p.size, dtype=ALAC_PACKET_RESULT)
        return _process_host(lib().ohgpu_raop_process_host, self._h, (_ptr(d), d.size, _ptr(p), p.size), src, dst, out)

    def flywheel_batch(self, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, FLYWHEEL_DESC)
        return _create(lib().ohgpu_flywheel_batch_create, self._h, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def flywheel_run(self, batch, d_src, d_dst, stream=None):
        check(lib().ohgpu_flywheel_batch_run(self._h, batch, d_src, d_dst, stream))

    def ohm_batch(self, streams, frames, fragments, src_arena_bytes, dst_arena_bytes):
        st, fr, fg = _typed(streams, OHM_STREAM), _typed(frames, OHM_FRAME_DESC), _typed(fragments, OHM_FRAGMENT)
        return _create(lib().ohgpu_ohm_batch_create, self._h, _ptr(st), st.size, _ptr(fr), fr.size, _ptr(fg), fg.size, src_arena_bytes, dst_arena_bytes)

    def ohm_run(self, batch, d_src, d_dst, stream=None):
        check(lib().ohgpu_ohm_batch_run(self._h, batch, d_src, d_dst, stream))

    def ohm_rx_batch(self, streams, datagrams, src_arena_bytes, dst_arena_bytes):
        s, g = _typed(streams, OHM_RX_STREAM), _typed(datagrams, OHM_RX_DATAGRAM)
        return _create(lib().ohgpu_ohm_rx_batch_create, self._h, _ptr(s), s.size, _ptr(g), g.size, src_arena_bytes, dst_arena_bytes)

    def ohm_rx_run(self, batch, d_src, d_dst, stream=None):
        """Parse, sequence, gather (ohgpu_ohm_rx_batch_run): queued on the stream; d_src 4-byte aligned."""
        check(lib().ohgpu_ohm_rx_batch_run(self._h, batch, d_src, d_dst, stream))

    def ohm_rx_results(self, batch, n, n_datagrams):
        """The last run's (OHM_RX_STREAM_RESULT per stream, OHM_RX_RECORD per datagram); waits for the run."""
        return _fetch_pair(lib().ohgpu_ohm_rx_batch_results, self._h, batch, OHM_RX_STREAM_RESULT, n, OHM_RX_RECORD, n_datagrams)

    def ohm_rx_phase_ms(self, batch):
        """The last run's (parse, sequence, gather) in milliseconds, from device events."""
        return _phase_ms(lib().ohgpu_ohm_rx_batch_phase_ms, self._h, batch, 3)

    def ohm_rx_process_host(self, streams, datagrams, src, dst):
        """Host buffers in and out (ohgpu_ohm_rx_process_host); returns (stream results, records)."""
        s, g = _typed(streams, OHM_RX_STREAM), _typed(datagrams, OHM_RX_DATAGRAM)
        out = np.zeros(s.size, dtype=OHM_RX_STREAM_RESULT), np.zeros(g.size, dtype=OHM_RX_RECORD)
        return _process_host(lib().ohgpu_ohm_rx_process_host, self._h, (_ptr(s), s.size, _ptr(g), g.size), src, dst, out)

    def raop_rx_batch(self, streams, datagrams, src_arena_bytes):
        s, g = _typed(streams, RAOP_RX_STREAM), _typed(datagrams, RAOP_RX_DATAGRAM)
        return _create(lib().ohgpu_raop_rx_batch_create, self._h, _ptr(s), s.size, _ptr(g), g.size, src_arena_bytes)

    def raop_rx_run(self, batch, d_src, stream=None):
        """Parse, sequence, table (ohgpu_raop_rx_batch_run): queued on the stream; d_src 4-byte aligned."""
        check(lib().ohgpu_raop_rx_batch_run(self._h, batch, d_src, stream))

    def raop_rx_results(self, batch, n, n_datagrams):
        """The last run's (RAOP_RX_STREAM_RESULT per stream, RAOP_RX_RECORD per datagram); waits for the run."""
        return _fetch_pair(lib().ohgpu_raop_rx_batch_results, self._h, batch, RAOP_RX_STREAM_RESULT, n, RAOP_RX_RECORD, n_datagrams)

    def raop_rx_packets(self, batch, n_datagrams):
        """The last run's packet table (ALAC_PACKET per datagram row); waits for the run."""
        return _fetch(lib().ohgpu_raop_rx_batch_packets, self._h, batch, ALAC_PACKET, n_datagrams)

    def raop_rx_phase_ms(self, batch):
        """The last run's (parse, sequence, table) in milliseconds, from device events."""
        return _phase_ms(lib().ohgpu_raop_rx_batch_phase_ms, self._h, batch, 3)

    def raop_rx_process_host(self, streams, datagrams, src):
        """Host buffer in (ohgpu_raop_rx_process_host); returns (stream results, records, packet rows)."""
        s, g = _typed(streams, RAOP_RX_STREAM), _typed(datagrams, RAOP_RX_DATAGRAM)
        out = np.zeros(s.size, dtype=RAOP_RX_STREAM_RESULT), np.zeros(g.size, dtype=RAOP_RX_RECORD), np.zeros(g.size, dtype=ALAC_PACKET)
        return _process_host(lib().ohgpu_raop_rx_process_host, self._h, (_ptr(s), s.size, _ptr(g), g.size), src, None, out)

    def raop_rx_alac_process_host(self, streams, descs, datagrams, src, dst):
        """Datagrams to PCM or plaintext (ohgpu_raop_rx_alac_process_host); returns (stream results, records, packet rows, Apple
        Lossless stream results, packet results by datagram row)."""
        s, g, d = _typed(streams, RAOP_RX_STREAM), _typed(datagrams, RAOP_RX_DATAGRAM), _typed(descs, RAOP_STREAM_DESC)
        assert d.size == s.size
        out = (np.zeros(s.size, dtype=RAOP_RX_STREAM_RESULT), np.zeros(g.size, dtype=RAOP_RX_RECORD), np.zeros(g.size, dtype=ALAC_PACKET),
               np.zeros(s.size, dtype=ALAC_STREAM_RESULT), np.zeros(g.size, dtype=ALAC_PACKET_RESULT))
        return _process_host(lib().ohgpu_raop_rx_alac_process_host, self._h, (_ptr(s), _ptr(d), s.size, _ptr(g), g.size), src, dst, out)

    def vorbis_batch(self, descs, packets, images, src_arena_bytes, dst_arena_bytes):
        d, p, im = _typed(descs, VORBIS_STREAM_DESC), _typed(packets, ALAC_PACKET), _typed(images, np.uint8)
        return _create(lib().ohgpu_vorbis_batch_create, self._h, _ptr(d), d.size, _ptr(p), p.size, _ptr(im), im.size, src_arena_bytes, dst_arena_bytes)

    def vorbis_run(self, batch, d_src, d_dst, stream=None):
        """Head, entropy, synthesis, store (ohgpu_vorbis_batch_run): queued on the stream."""
        check(lib().ohgpu_vorbis_batch_run(self._h, batch, d_src, d_dst, stream))

    def vorbis_results(self, batch, n, n_packets):
        """The last run's (VORBIS_STREAM_RESULT per stream, VORBIS_PACKET_RESULT per packet); waits for the run."""
        return _fetch_pair(lib().ohgpu_vorbis_batch_results, self._h, batch, VORBIS_STREAM_RESULT, n, VORBIS_PACKET_RESULT, n_packets)

    def vorbis_phase_ms(self, batch):
        """(head, entropy, synthesis, store) of the last run in milliseconds."""
        return _phase_ms(lib().ohgpu_vorbis_batch_phase_ms, self._h, batch, 4)

    def vorbis_paths(self, batch):
        """{route, blocks} of a Vorbis batch (ohgpu_vorbis_batch_paths)."""
        return _paths(lib().ohgpu_vorbis_batch_paths, batch, "route", "blocks")

    def vorbis_spectrum(self, batch, packet, channel, n_values):
        """The float32 spectrum the last run transformed for one packet and channel (ohgpu_vorbis_batch_spectrum)."""
        out = np.zeros(n_values, dtype=np.float32)
        check(lib().ohgpu_vorbis_batch_spectrum(self._h, batch, packet, channel, _ptr(out), n_values))
        return out

    def vorbis_process_host(self, descs, packets, images, src, dst):
        """Host buffers in and out (ohgpu_vorbis_process_host); returns (stream results, packet results)."""
        d, p, im = _typed(descs, VORBIS_STREAM_DESC), _typed(packets, ALAC_PACKET), _typed(images, np.uint8)
        out = np.zeros(d.size, dtype=VORBIS_STREAM_RESULT), np.zeros(p.size, dtype=VORBIS_PACKET_RESULT)
        return _process_host(lib().ohgpu_vorbis_process_host, self._h, (_ptr(d), d.size, _ptr(p), p.size, _ptr(im), im.size), src, dst, out)

    def ogg_vorbis_process_host(self, ogg_descs, vorbis_descs, n_packets, images, src, mid_bytes, dst):
        """Ogg bytes to PCM (ohgpu_ogg_vorbis_process_host); returns (Ogg results, Ogg packet table, Vorbis stream results, packet results
        indexed as the Ogg table)."""
        o, v, im = _typed(ogg_descs, OGG_STREAM_DESC), _typed(vorbis_descs, VORBIS_STREAM_DESC), _typed(images, np.uint8)
        assert v.size == o.size
        out = (np.zeros(o.size, dtype=OGG_STREAM_RESULT), np.zeros(n_packets, dtype=OGG_PACKET),
               np.zeros(o.size, dtype=VORBIS_STREAM_RESULT), np.zeros(n_packets, dtype=VORBIS_PACKET_RESULT))
        return _process_host(lib().ohgpu_ogg_vorbis_process_host, self._h, (_ptr(o), _ptr(v), o.size, n_packets, _ptr(im), im.size), src, dst, out,
                             mid=(mid_bytes,))

    def ogg_vorbis_links_process_host(self, ogg_descs, vorbis_descs, dst_capacity_bytes, n_packets, images, src, mid_bytes, dst, links_capacity=None):
        """Chained Ogg bytes to PCM (ohgpu_ogg_vorbis_links_process_host); returns (Ogg results, Ogg packet table, the link rows -- all of
        them unless links_capacity says how many there is room for, then (rows, true count) --, packet results indexed as the Ogg table)."""
        o, v, im = _typed(ogg_descs, OGG_STREAM_DESC), _typed(vorbis_descs, VORBIS_STREAM_DESC), _typed(images, np.uint8)
        caps = np.ascontiguousarray(dst_capacity_bytes, dtype="<u8")
        assert v.size == o.size == caps.size
        room = o.size + n_packets if links_capacity is None else links_capacity
        links, count, pres = np.zeros(room, dtype=VORBIS_LINK), C.c_size_t(0), np.zeros(n_packets, dtype=VORBIS_PACKET_RESULT)
        ores, orecs, _ = _process_host(lib().ohgpu_ogg_vorbis_links_process_host, self._h, (_ptr(o), _ptr(v), _ptr(caps), o.size, n_packets, _ptr(im), im.size),
                                       src, dst, (np.zeros(o.size, dtype=OGG_STREAM_RESULT), np.zeros(n_packets, dtype=OGG_PACKET), links), mid=(mid_bytes,),
                                       tail=(room, C.byref(count), _ptr(pres)))
        if links_capacity is None:
            return ores, orecs, links[:count.value].copy(), pres
        return ores, orecs, (links, count.value), pres

    def ts_batch(self, descs, n_pes, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, TS_STREAM_DESC)
        return _create(lib().ohgpu_ts_batch_create, self._h, _ptr(d), d.size, n_pes, src_arena_bytes, dst_arena_bytes)

    def ts_run(self, batch, d_src, d_dst, stream=None):
        """Parse, tables and sums, gather (ohgpu_ts_batch_run): queued on the stream."""
        check(lib().ohgpu_ts_batch_run(self._h, batch, d_src, d_dst, stream))

    def ts_results(self, batch, n, n_pes):
        """The last run's (TS_STREAM_RESULT per stream, the PES table as TS_PES); waits for the run."""
        return _fetch(lib().ohgpu_ts_batch_results, self._h, batch, TS_STREAM_RESULT, n), _fetch(lib().ohgpu_ts_batch_pes, self._h, batch, TS_PES, n_pes)

    def ts_phase_ms(self, batch):
        """(parse, tables and sums, gather) of the last run in milliseconds."""
        return _phase_ms(lib().ohgpu_ts_batch_phase_ms, self._h, batch, 3)

    def ts_paths(self, batch):
        """{route, tiles, wave_blocks} of a transport stream batch (ohgpu_ts_batch_paths)."""
        return _paths(lib().ohgpu_ts_batch_paths, batch, "route", "tiles", "wave_blocks")

    def ts_process_host(self, descs, n_pes, src, dst):
        """Host buffers in and out (ohgpu_ts_process_host); returns (stream results, PES table)."""
        d = _typed(descs, TS_STREAM_DESC)
        out = np.zeros(d.size, dtype=TS_STREAM_RESULT), np.zeros(n_pes, dtype=TS_PES)
        return _process_host(lib().ohgpu_ts_process_host, self._h, (_ptr(d), d.size, n_pes), src, dst, out)

    def adts_batch(self, descs, n_frames, src_arena_bytes):
        d = _typed(descs, ADTS_STREAM_DESC)
        return _create(lib().ohgpu_adts_batch_create, self._h, _ptr(d), d.size, n_frames, src_arena_bytes)

    def adts_run(self, batch, d_src, stream=None):
        """Map, chain (ohgpu_adts_batch_run): queued on the stream."""
        check(lib().ohgpu_adts_batch_run(self._h, batch, d_src, stream))

    def adts_results(self, batch, n, n_frames):
        """The last run's (ADTS_STREAM_RESULT per stream, the frame table as ADTS_FRAME); waits for the run."""
        return (_fetch(lib().ohgpu_adts_batch_results, self._h, batch, ADTS_STREAM_RESULT, n),
                _fetch(lib().ohgpu_adts_batch_frames, self._h, batch, ADTS_FRAME, n_frames))

    def adts_phase_ms(self, batch):
        """(map, chain) of the last run in milliseconds."""
        return _phase_ms(lib().ohgpu_adts_batch_phase_ms, self._h, batch, 2)

    def adts_paths(self, batch):
        """{route, tiles} of an ADTS batch (ohgpu_adts_batch_paths)."""
        return _paths(lib().ohgpu_adts_batch_paths, batch, "route", "tiles")

    def adts_process_host(self, descs, n_frames, src):
        """Host bytes in (ohgpu_adts_process_host); returns (stream results, frame table)."""
        d = _typed(descs, ADTS_STREAM_DESC)
        out = np.zeros(d.size, dtype=ADTS_STREAM_RESULT), np.zeros(n_frames, dtype=ADTS_FRAME)
        return _process_host(lib().ohgpu_adts_process_host, self._h, (_ptr(d), d.size, n_frames), src, None, out)

    def ts_adts_process_host(self, ts_descs, adts_descs, n_pes, n_frames, src, dst):
        """Transport bytes to the elementary run, the PES table and the frame table (ohgpu_ts_adts_process_host); returns (TS results, PES
        table, ADTS results, frame table)."""
        t, a = _typed(ts_descs, TS_STREAM_DESC), _typed(adts_descs, ADTS_STREAM_DESC)
        assert t.size == a.size
        out = (np.zeros(t.size, dtype=TS_STREAM_RESULT), np.zeros(n_pes, dtype=TS_PES),
               np.zeros(t.size, dtype=ADTS_STREAM_RESULT), np.zeros(n_frames, dtype=ADTS_FRAME))
        return _process_host(lib().ohgpu_ts_adts_process_host, self._h, (_ptr(t), _ptr(a), t.size, n_pes, n_frames), src, dst, out)

    def ogg_batch(self, descs, n_packets, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, OGG_STREAM_DESC)
        return _create(lib().ohgpu_ogg_batch_create, self._h, _ptr(d), d.size, n_packets, src_arena_bytes, dst_arena_bytes)

    def ogg_run(self, batch, d_src, d_dst, stream=None):
        """Find, verify, chain, gather (ohgpu_ogg_batch_run): queued on the stream."""
        check(lib().ohgpu_ogg_batch_run(self._h, batch, d_src, d_dst, stream))

    def ogg_results(self, batch, n, n_packets):
        """The last run's (OGG_STREAM_RESULT per stream, the packet table as OGG_PACKET); waits for the run."""
        return (_fetch(lib().ohgpu_ogg_batch_results, self._h, batch, OGG_STREAM_RESULT, n),
                _fetch(lib().ohgpu_ogg_batch_packets, self._h, batch, OGG_PACKET, n_packets))

    def ogg_phase_ms(self, batch):
        """The last run's (find, verify, chain, gather) in milliseconds, from device events."""
        return _phase_ms(lib().ohgpu_ogg_batch_phase_ms, self._h, batch, 4)

    def ogg_process_host(self, descs, n_packets, src, dst):
        """Host buffers in and out (ohgpu_ogg_process_host); returns (stream results, packet table)."""
        d = _typed(descs, OGG_STREAM_DESC)
        out = np.zeros(d.size, dtype=OGG_STREAM_RESULT), np.zeros(n_packets, dtype=OGG_PACKET)
        return _process_host(lib().ohgpu_ogg_process_host, self._h, (_ptr(d), d.size, n_packets), src, dst, out)

    def ogg_flac_process_host(self, ogg_descs, flac_descs, n_packets, src, mid_bytes, dst, frames_capacity=0):
        """Ogg FLAC from host buffers (ohgpu_ogg_flac_process_host); returns (Ogg results, packet table, FLAC results, frames)."""
        o, f = _typed(ogg_descs, OGG_STREAM_DESC), _typed(flac_descs, FLAC_STREAM_DESC)
        assert f.size == o.size
        out = (np.zeros(o.size, dtype=OGG_STREAM_RESULT), np.zeros(n_packets, dtype=OGG_PACKET),
               np.zeros(o.size, dtype=FLAC_STREAM_RESULT), np.zeros(frames_capacity, dtype=FLAC_FRAME))
        n_frames = C.c_size_t(0)
        _process_host(lib().ohgpu_ogg_flac_process_host, self._h, (_ptr(o), _ptr(f), o.size, n_packets), src, dst, out, mid=(mid_bytes,),
                      tail=(frames_capacity, C.byref(n_frames)))
        return (*out[:3], out[3][:min(int(n_frames.value), frames_capacity)])

    def mp4_batch(self, descs, n_packets, src_arena_bytes):
        d = _typed(descs, MP4_STREAM_DESC)
        return _create(lib().ohgpu_mp4_batch_create, self._h, _ptr(d), d.size, n_packets, src_arena_bytes)

    def mp4_run(self, batch, d_src, stream=None):
        """Walk, tile sums, carries, expand (ohgpu_mp4_batch_run): queued on the stream."""
        check(lib().ohgpu_mp4_batch_run(self._h, batch, d_src, stream))

    def mp4_results(self, batch, n, n_packets):
        """The last run's (MP4_STREAM_RESULT per stream, the packet table as ALAC_PACKET, the sample table as MP4_SAMPLE); waits for the run."""
        return (_fetch(lib().ohgpu_mp4_batch_results, self._h, batch, MP4_STREAM_RESULT, n),
                _fetch(lib().ohgpu_mp4_batch_packets, self._h, batch, ALAC_PACKET, n_packets),
                _fetch(lib().ohgpu_mp4_batch_samples, self._h, batch, MP4_SAMPLE, n_packets))

    def mp4_phase_ms(self, batch):
        """The last run's (walk, tile sums, carries, expand) in milliseconds, from device events; the plain route: (all of it, 0, 0, 0)."""
        return _phase_ms(lib().ohgpu_mp4_batch_phase_ms, self._h, batch, 4)

    def mp4_process_host(self, descs, n_packets, src):
        """Host bytes in (ohgpu_mp4_process_host); returns (stream results, packet table, sample table)."""
        d = _typed(descs, MP4_STREAM_DESC)
        out = np.zeros(d.size, dtype=MP4_STREAM_RESULT), np.zeros(n_packets, dtype=ALAC_PACKET), np.zeros(n_packets, dtype=MP4_SAMPLE)
        return _process_host(lib().ohgpu_mp4_process_host, self._h, (_ptr(d), d.size, n_packets), src, None, out)

    def mp4_alac_process_host(self, mp4_descs, alac_descs, n_packets, src, dst):
        """.m4a bytes in, PCM out (ohgpu_mp4_alac_process_host); returns (MPEG-4 results, packet table, sample table, Apple Lossless stream
        results, packet results indexed as the tables are).  Of alac_descs only flags, dst_offset and dst_plane_stride are read."""
        m, a = _typed(mp4_descs, MP4_STREAM_DESC), _typed(alac_descs, ALAC_STREAM_DESC)
        assert a.size == m.size
        out = (np.zeros(m.size, dtype=MP4_STREAM_RESULT), np.zeros(n_packets, dtype=ALAC_PACKET), np.zeros(n_packets, dtype=MP4_SAMPLE),
               np.zeros(m.size, dtype=ALAC_STREAM_RESULT), np.zeros(n_packets, dtype=ALAC_PACKET_RESULT))
        return _process_host(lib().ohgpu_mp4_alac_process_host, self._h, (_ptr(m), _ptr(a), m.size, n_packets), src, dst, out)

    # ---- the three fragmented MPEG-4 families: one implementation (counts: see _FRAG), then each family's names over it
    def _frag_batch(self, fam, descs, counts, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, _FRAG[fam][0])
        return _create(_frag_fn(fam, "batch_create"), self._h, _ptr(d), d.size, *counts, src_arena_bytes, dst_arena_bytes)

    def _frag_results(self, fam, batch, n, n_packets, n_runs):
        return (_fetch(_frag_fn(fam, "batch_results"), self._h, batch, _FRAG[fam][1], n), _fetch(_frag_fn(fam, "batch_runs"), self._h, batch, MP4F_RUN, n_runs),
                _fetch(_frag_fn(fam, "batch_packets"), self._h, batch, ALAC_PACKET, n_packets), _fetch(_frag_fn(fam, "batch_samples"), self._h, batch, MP4_SAMPLE, n_packets))

    def _frag_process_host(self, fam, descs, counts, src, dst):
        d = _typed(descs, _FRAG[fam][0])
        return _process_host(_frag_fn(fam, "process_host"), self._h, (_ptr(d), d.size, *counts), src, dst, _frag_zeros(fam, d.size, *counts[:2]))

    def _frag_flac_process_host(self, fam, descs, flac_descs, counts, src, mid_bytes, dst, frames_capacity):
        m, f = _typed(descs, _FRAG[fam][0]), _typed(flac_descs, FLAC_STREAM_DESC)
        assert f.size == m.size
        out = (*_frag_zeros(fam, m.size, *counts[:2]), np.zeros(m.size, dtype=FLAC_STREAM_RESULT), np.zeros(frames_capacity, dtype=FLAC_FRAME))
        n_frames = C.c_size_t(0)
        _process_host(_frag_fn(fam, "flac_process_host"), self._h, (_ptr(m), _ptr(f), m.size, *counts), src, dst, out, mid=(mid_bytes,),
                      tail=(frames_capacity, C.byref(n_frames)))
        return (*out[:5], out[5][:min(int(n_frames.value), frames_capacity)])

    def _frag_alac_process_host(self, fam, descs, alac_descs, counts, src, mid, dst):
        """mid: (mid_bytes,) for a protected family, () for mp4f, whose packets are decoded where they lie"""
        m, a = _typed(descs, _FRAG[fam][0]), _typed(alac_descs, ALAC_STREAM_DESC)
        assert a.size == m.size
        out = (*_frag_zeros(fam, m.size, *counts[:2]), np.zeros(m.size, dtype=ALAC_STREAM_RESULT), np.zeros(counts[0], dtype=ALAC_PACKET_RESULT))
        return _process_host(_frag_fn(fam, "alac_process_host"), self._h, (_ptr(m), _ptr(a), m.size, *counts), src, dst, out, mid=mid)

    def mp4f_batch(self, descs, n_packets, n_runs, src_arena_bytes, dst_arena_bytes):
        return self._frag_batch("mp4f", descs, (n_packets, n_runs), src_arena_bytes, dst_arena_bytes)

    def mp4f_run(self, batch, d_src, d_dst, stream=None):
        """Walk, run sums, carries, expand, finish, gather (ohgpu_mp4f_batch_run): queued on the stream."""
        check(lib().ohgpu_mp4f_batch_run(self._h, batch, d_src, d_dst, stream))

    def mp4f_results(self, batch, n, n_packets, n_runs):
        """The last run's (MP4F_STREAM_RESULT per stream, the run table, the packet table, the sample table); waits for the run."""
        return self._frag_results("mp4f", batch, n, n_packets, n_runs)

    def mp4f_phase_ms(self, batch):
        """(walk, run sums, carries, expand, finish, gather) of the last run in milliseconds."""
        return _phase_ms(lib().ohgpu_mp4f_batch_phase_ms, self._h, batch, 6)

    def mp4f_paths(self, batch):
        """{route, tiles, wave_blocks} of a fragmented MPEG-4 batch (ohgpu_mp4f_batch_paths)."""
        return _paths(lib().ohgpu_mp4f_batch_paths, batch, "route", "tiles", "wave_blocks")

    def mp4f_process_host(self, descs, n_packets, n_runs, src, dst):
        """Host bytes in (ohgpu_mp4f_process_host), the gathered runs into dst; returns (results, run table, packet table, sample table)."""
        return self._frag_process_host("mp4f", descs, (n_packets, n_runs), src, dst)

    def mp4f_flac_process_host(self, mp4f_descs, flac_descs, n_packets, n_runs, src, mid_bytes, dst, frames_capacity=0):
        """Fragmented fLaC from host buffers to PCM (ohgpu_mp4f_flac_process_host); returns (results, run table, packet table, sample table,
        FLAC results, frames)."""
        return self._frag_flac_process_host("mp4f", mp4f_descs, flac_descs, (n_packets, n_runs), src, mid_bytes, dst, frames_capacity)

    def mp4f_alac_process_host(self, mp4f_descs, alac_descs, n_packets, n_runs, src, dst):
        """Fragmented alac from host buffers to PCM (ohgpu_mp4f_alac_process_host); returns (results, run table, packet table, sample table,
        Apple Lossless stream results, packet results indexed as the tables are)."""
        return self._frag_alac_process_host("mp4f", mp4f_descs, alac_descs, (n_packets, n_runs), src, (), dst)

    def cenc_batch(self, descs, n_packets, n_runs, src_arena_bytes, dst_arena_bytes):
        return self._frag_batch("cenc", descs, (n_packets, n_runs), src_arena_bytes, dst_arena_bytes)

    def cenc_run(self, batch, d_src, d_dst, stream=None):
        """Walk, run sums, carries, expand, finish, decrypt-gather (ohgpu_cenc_batch_run): queued on the stream."""
        check(lib().ohgpu_cenc_batch_run(self._h, batch, d_src, d_dst, stream))

    def cenc_results(self, batch, n, n_packets, n_runs):
        """The last run's (CENC_STREAM_RESULT per stream, the run table, the packet table, the sample table); waits for the run."""
        return self._frag_results("cenc", batch, n, n_packets, n_runs)

    def cenc_phase_ms(self, batch):
        """(walk, run sums, carries, expand, finish, decrypt-gather) of the last run in milliseconds."""
        return _phase_ms(lib().ohgpu_cenc_batch_phase_ms, self._h, batch, 6)

    def cenc_paths(self, batch):
        """{route, tiles, wave_blocks: the persistent decrypt-gather launch's workgroups} of a protected MPEG-4 batch (ohgpu_cenc_batch_paths)."""
        return _paths(lib().ohgpu_cenc_batch_paths, batch, "route", "tiles", "wave_blocks")

    def cenc_process_host(self, descs, n_packets, n_runs, src, dst):
        """Host bytes in (ohgpu_cenc_process_host), the clear runs into dst; returns (results, run table, packet table, sample table)."""
        return self._frag_process_host("cenc", descs, (n_packets, n_runs), src, dst)

    def cenc_flac_process_host(self, cenc_descs, flac_descs, n_packets, n_runs, src, mid_bytes, dst, frames_capacity=0):
        """Protected fLaC from host buffers to PCM (ohgpu_cenc_flac_process_host); returns (results, run table, packet table, sample table,
        FLAC results, frames)."""
        return self._frag_flac_process_host("cenc", cenc_descs, flac_descs, (n_packets, n_runs), src, mid_bytes, dst, frames_capacity)

    def cenc_alac_process_host(self, cenc_descs, alac_descs, n_packets, n_runs, src, mid_bytes, dst):
        """Protected alac from host buffers to PCM (ohgpu_cenc_alac_process_host); returns (results, run table, packet table, sample table,
        Apple Lossless stream results, packet results indexed as the tables are)."""
        return self._frag_alac_process_host("cenc", cenc_descs, alac_descs, (n_packets, n_runs), src, (mid_bytes,), dst)

    def cbcs_batch(self, descs, n_packets, n_runs, n_subsamples, src_arena_bytes, dst_arena_bytes):
        return self._frag_batch("cbcs", descs, (n_packets, n_runs, n_subsamples), src_arena_bytes, dst_arena_bytes)

    def cbcs_run(self, batch, d_src, d_dst, stream=None):
        """Walk and subsample chain, run sums, carries, expand, finish, decrypt-gather (ohgpu_cbcs_batch_run): queued on the stream."""
        check(lib().ohgpu_cbcs_batch_run(self._h, batch, d_src, d_dst, stream))

    def cbcs_results(self, batch, n, n_packets, n_runs):
        """The last run's (CBCS_STREAM_RESULT per stream, the run table, the packet table, the sample table); waits for the run."""
        return self._frag_results("cbcs", batch, n, n_packets, n_runs)

    def cbcs_phase_ms(self, batch):
        """(walk, run sums, carries, expand, finish, decrypt-gather) of the last run in milliseconds."""
        return _phase_ms(lib().ohgpu_cbcs_batch_phase_ms, self._h, batch, 6)

    def cbcs_paths(self, batch):
        """{route, tiles, wave_blocks: the persistent decrypt-gather launch's workgroups} of a batch of the family (ohgpu_cbcs_batch_paths)."""
        return _paths(lib().ohgpu_cbcs_batch_paths, batch, "route", "tiles", "wave_blocks")

    def cbcs_process_host(self, descs, n_packets, n_runs, n_subsamples, src, dst):
        """Host bytes in (ohgpu_cbcs_process_host), the clear runs into dst; returns (results, run table, packet table, sample table)."""
        return self._frag_process_host("cbcs", descs, (n_packets, n_runs, n_subsamples), src, dst)

    def cbcs_flac_process_host(self, descs, flac_descs, n_packets, n_runs, n_subsamples, src, mid_bytes, dst, frames_capacity=0):
        """Protected fLaC from host buffers to PCM (ohgpu_cbcs_flac_process_host); returns (results, run table, packet table, sample table,
        FLAC results, frames)."""
        return self._frag_flac_process_host("cbcs", descs, flac_descs, (n_packets, n_runs, n_subsamples), src, mid_bytes, dst, frames_capacity)

    def cbcs_alac_process_host(self, descs, alac_descs, n_packets, n_runs, n_subsamples, src, mid_bytes, dst):
        """Protected alac from host buffers to PCM (ohgpu_cbcs_alac_process_host); returns (results, run table, packet table, sample table,
        Apple Lossless stream results, packet results indexed as the tables are)."""
        return self._frag_alac_process_host("cbcs", descs, alac_descs, (n_packets, n_runs, n_subsamples), src, (mid_bytes,), dst)

    def iff_batch(self, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, IFF_STREAM_DESC)
        return _create(lib().ohgpu_iff_batch_create, self._h, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def iff_run(self, batch, d_src, d_dst, stream=None):
        """Walk, convert (ohgpu_iff_batch_run): queued on the stream."""
        check(lib().ohgpu_iff_batch_run(self._h, batch, d_src, d_dst, stream))

    def iff_results(self, batch, n):
        """The last run's IFF_STREAM_RESULT per stream; waits for the run."""
        return _fetch(lib().ohgpu_iff_batch_results, self._h, batch, IFF_STREAM_RESULT, n)

    def iff_phase_ms(self, batch):
        """The last run's (walk, convert) in milliseconds, from device events; the plain route: (all of it, 0)."""
        return _phase_ms(lib().ohgpu_iff_batch_phase_ms, self._h, batch, 2)

    def dsd_file_batch(self, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, DSD_FILE_STREAM_DESC)
        return _create(lib().ohgpu_dsd_file_batch_create, self._h, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def dsd_file_run(self, batch, d_src, d_dst, stream=None):
        """Walk, convert (ohgpu_dsd_file_batch_run): queued on the stream."""
        check(lib().ohgpu_dsd_file_batch_run(self._h, batch, d_src, d_dst, stream))

    def dsd_file_results(self, batch, n):
        """The last run's DSD_FILE_STREAM_RESULT per stream; waits for the run."""
        return _fetch(lib().ohgpu_dsd_file_batch_results, self._h, batch, DSD_FILE_STREAM_RESULT, n)

    def dsd_file_phase_ms(self, batch):
        """(walk, convert) of the last run in milliseconds; waits for the run."""
        return list(_phase_ms(lib().ohgpu_dsd_file_batch_phase_ms, self._h, batch, 2))     # (a list where its siblings answer a tuple)

    def dsd_file_process_host(self, descs, src, dst):
        """File bytes in, sample blocks of the pipeline's DSD format into dst (ohgpu_dsd_file_process_host); returns the stream results."""
        d = _typed(descs, DSD_FILE_STREAM_DESC)
        return _process_host(lib().ohgpu_dsd_file_process_host, self._h, (_ptr(d), d.size), src, dst, (np.zeros(d.size, dtype=DSD_FILE_STREAM_RESULT),))[0]

    def iff_process_host(self, descs, src, dst):
        """File bytes in, big-endian PCM into dst (ohgpu_iff_process_host); returns the stream results."""
        d = _typed(descs, IFF_STREAM_DESC)
        return _process_host(lib().ohgpu_iff_process_host, self._h, (_ptr(d), d.size), src, dst, (np.zeros(d.size, dtype=IFF_STREAM_RESULT),))[0]

    def src_create(self, L, M, T, coef_q28):
        c = np.ascontiguousarray(coef_q28, dtype=np.int32)
        return _create(lib().ohgpu_src_create, self._h, L, M, T, _ptr(c, keep=True))

    def src_destroy(self, src):
        check(lib().ohgpu_src_destroy(self._h, src))

    def src_batch(self, src, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, SRC_MSG_DESC)
        return _create(lib().ohgpu_src_batch_create, self._h, src, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def src_batch_block(self, batch):
        lo, mi = C.c_uint32(0), C.c_uint32(0)
        check(lib().ohgpu_src_batch_block(batch, C.byref(lo), C.byref(mi)))
        return int(lo.value), int(mi.value)

    def src_batch_advance(self, batch, blocks):
        check(lib().ohgpu_src_batch_advance(self._h, batch, blocks))

    def src_batch_set_ramps(self, batch, ramp_start, ramp_end):
        a = np.ascontiguousarray(ramp_start, dtype=np.uint16)
        e = np.ascontiguousarray(ramp_end, dtype=np.uint16)
        assert a.size == e.size
        check(lib().ohgpu_src_batch_set_ramps(self._h, batch, _ptr(a, keep=True), _ptr(e, keep=True), a.size))

    def src_process_host(self, src, descs, src_bytes, dst_bytes_array):
        """ohgpu_src_process_host: host buffers in, host buffers out (validation, upload, launch, download, sync in one call)."""
        d = _typed(descs, SRC_MSG_DESC)
        _process_host(lib().ohgpu_src_process_host, self._h, (src, _ptr(d), d.size), src_bytes, dst_bytes_array, ())
        return dst_bytes_array

    def src_plan(self, batch):
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib().ohgpu_src_batch_plan(batch, C.byref(a), C.byref(b)))
        return {"block_kernel_out_frames": int(a.value), "generic_pieces": int(b.value)}

    def src_units(self, batch):
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(lib().ohgpu_src_batch_units(batch, C.byref(a), C.byref(b)))
        return {"units": int(a.value), "long_units": int(b.value)}

    def src_kernel_name(self, batch):
        buf = C.create_string_buffer(256)
        check(lib().ohgpu_src_batch_kernel_name(self._h, batch, buf, 256))
        return buf.value.decode()

    def src_occupancy(self, batch):
        g, want, lds = C.c_int(0), C.c_int(0), C.c_uint32(0)
        check(lib().ohgpu_src_batch_occupancy(self._h, batch, C.byref(g), C.byref(want), C.byref(lds)))
        return {"workgroups_per_cu": int(g.value), "designed_for": int(want.value), "lds_bytes": int(lds.value)}

    def device_allocations(self):
        n = C.c_uint64(0)
        check(lib().ohgpu_device_allocations(self._h, C.byref(n)))
        return int(n.value)

    def pci_bus_id(self):
        buf = C.create_string_buffer(64)
        check(lib().ohgpu_device_pci_bus_id(self._h, buf, 64))
        return buf.value.decode()

    def host_transfer_stats(self):
        """What the *_process_host calls of this context moved so far (ohgpu_host_transfer_stats)."""
        v = [C.c_uint64(0) for _ in range(4)]
        check(lib().ohgpu_host_transfer_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("calls", "src_calls", "h2d_bytes", "d2h_bytes"), (int(x.value) for x in v)))

    def shader_clock_mhz(self, stream=None):
        mhz = C.c_double(0)
        check(lib().ohgpu_measure_shader_clock(self._h, stream, C.byref(mhz)))
        return float(mhz.value)

    def src_run(self, batch, d_src, d_dst, stream=None, events=None):
        """`events` = (start, stop) of ctx.event(): they bracket the batch's device work (on the dispatch itself where the batch is one launch)."""
        if events is not None:
            check(lib().ohgpu_src_batch_run_timed(self._h, batch, d_src, d_dst, stream, events[0], events[1]))
        else:
            check(lib().ohgpu_src_batch_run(self._h, batch, d_src, d_dst, stream))

    # ---- the pulled resampler
    def src_pull_create(self, taps_per_phase, phases_log2, coef_q28):
        c = np.ascontiguousarray(coef_q28, dtype=np.int32)
        return _create(lib().ohgpu_src_pull_create, self._h, taps_per_phase, phases_log2, _ptr(c, keep=True))

    def src_pull_destroy(self, src):
        check(lib().ohgpu_src_pull_destroy(self._h, src))

    def src_pull_batch(self, src, descs, src_arena_bytes, dst_arena_bytes):
        d = _typed(descs, SRC_PULL_MSG_DESC)
        return _create(lib().ohgpu_src_pull_batch_create, self._h, src, _ptr(d), d.size, src_arena_bytes, dst_arena_bytes)

    def src_pull_run(self, batch, d_src, d_dst, stream=None):
        check(lib().ohgpu_src_pull_batch_run(self._h, batch, d_src, d_dst, stream))

    def src_pull_process_host(self, src, descs, src_bytes, dst_bytes_array):
        """ohgpu_src_pull_process_host: host buffers in, host buffers out."""
        d = _typed(descs, SRC_PULL_MSG_DESC)
        _process_host(lib().ohgpu_src_pull_process_host, self._h, (src, _ptr(d), d.size), src_bytes, dst_bytes_array, ())
        return dst_bytes_array

