// ohgpu_internal.h -- host-side structures behind the opaque handles of include/ohgpu.h.
#pragma once

#include <sys/mman.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ohgpu.h"
#include "alac_packet_core.h"
#include "flac_frame_core.h"
#include "ogg_page_core.h"
#include "mp4_box_core.h"
#include "mp4_frag_core.h"
#include "iff_chunk_core.h"
#include "dsd_file_core.h"
#include "ohm_rx_core.h"
#include "raop_rx_core.h"
#include "raop_aes_core.h"
#include "cenc_core.h"
#include "cbcs_core.h"
#include "ts_packet_core.h"
#include "vorbis_core.h"

namespace ohgpu {

// Device-side form of one piece of a resampled output message (56 bytes): everything 64-bit that can be
// precomputed on the host has been.  in_rel0 = n0(first output) - src_frame0 (negative only at a stream
// start, where frames with a negative absolute index read as zero); phase0 = (first output * M) % L.
// A piece is a whole message, or the part of one that the block kernel leaves to the generic kernel;
// ramp_i0 / ramp_n place it inside its message for RampApplicator's (iLoopCount, iNumSamples).
struct DevSrcDesc {
    uint64_t src_offset;
    uint64_t dst_offset;
    int64_t  in_rel0;
    uint32_t phase0;
    uint32_t n_frames;
    uint32_t ramp_i0;
    uint32_t ramp_n;
    uint16_t ramp_start;
    uint16_t ramp_end;
    uint8_t  channels;
    uint8_t  src_bits;
    uint8_t  src_endian;
    uint8_t  dst_bits;
    uint8_t  dst_endian;
    uint8_t  flags;
    uint8_t  pad[2];
    uint32_t plane_frames;    // OHGPU_FLAG_SRC_PLANAR32: frames (4-byte units) between the channels' planes
};
static_assert(sizeof(DevSrcDesc) == 56, "DevSrcDesc layout");
static_assert(sizeof(ohgpu_msg_desc) == 32, "ohgpu_msg_desc layout");
static_assert(sizeof(ohgpu_src_msg_desc) == 64, "ohgpu_src_msg_desc layout");
static_assert(sizeof(ohgpu_fmt_desc) == 48, "ohgpu_fmt_desc layout");
static_assert(sizeof(ohgpu_batch_paths) == 64, "ohgpu_batch_paths layout");
static_assert(sizeof(ohgpu_dsd_desc) == 32, "ohgpu_dsd_desc layout");
static_assert(sizeof(ohgpu_flac_stream_desc) == 64 && sizeof(ohgpu_flac_stream_result) == 48 && sizeof(ohgpu_flac_streaminfo_t) == 48 && sizeof(ohgpu_flac_frame) == 24, "FLAC layouts");
static_assert(sizeof(flaccore::Result) == sizeof(ohgpu_flac_stream_result) && sizeof(flaccore::Stream) == 64 && sizeof(flaccore::Probe) == 56 && sizeof(flaccore::Sub) == 80, "FLAC device layouts");

// ---- block ("fast") resampler plan: contiguous runs of output messages cut into phase-aligned blocks ----
struct SrcSeg {               // one contiguous run of output messages of one stream
    int64_t  src_base;        // byte offset (in the source arena) of the stream's absolute input frame 0
    int64_t  dst_base;        // byte offset (in the destination arena) of the stream's absolute output frame 0
    uint32_t msg_begin;       // [msg_begin, msg_end) in the SegMsg array, ordered by out0
    uint32_t msg_end;
};
struct SegMsg {               // ramp parameters of one output message, 24 bytes
    uint64_t out0;            // absolute index of its first output frame
    uint32_t n;               // frames
    uint16_t ramp_start;
    uint16_t ramp_end;
    uint8_t  flags;
    uint8_t  s_n1;            // x / (n - 1) == umulhi(x, m_n1) >> s_n1 for x < 2^31 (m_n1 == 0: n - 1 <= 1): the ramp's division
    uint8_t  pad[2];
    uint32_t m_n1;
};
static_assert(sizeof(SegMsg) == 24, "SegMsg");
struct SrcWork {              // one workgroup's share: up to `rows` consecutive blocks of one segment
    uint64_t first_block;     // absolute block index (block b covers outputs [b*L_blk, (b+1)*L_blk))
    uint32_t seg;
    uint32_t n_blocks;
    uint32_t msg_first;       // index (in the SegMsg array) of the message that holds the unit's first output frame
    uint32_t flags;           // kWorkRamped | kWorkChecked (src_block_common.h)
    uint32_t plane;           // a ramped unit's multiplier plane (lean kernel): its index in SrcFastPlan::d_planes
    uint32_t pad;
};
struct LeanUnit {             // the lean kernel's own view of a unit (same order as the SrcWork array): ONE 32-byte scalar load,
                              // nothing to look up behind it -- a unit's set-up used to wait for work[], then for segs[work.seg]
    int64_t  src_row0;        // source arena offset of row 0's input frame at advance -T: seg.src_base + (first_block * M_blk - T) * fb_src
    int64_t  dst_row0;        // destination arena offset of row 0's first output byte: seg.dst_base + first_block * L_blk * fb_dst
    uint32_t n_blocks;
    uint32_t flags;           // kWorkRamped | kWorkChecked | kWorkFirst; bits 8..15: blocks per ROW (a row = that many consecutive blocks)
    uint32_t plane;
    uint32_t src_plane_stride; // planar source: bytes between the channels' planes (the planner keeps such a batch off this kernel
                               // unless every plane of a unit is within 4 GiB of its first)
};
struct RampJob {              // ramp_plane_kernel: frames [i0, i0 + count) of one ramped message go to entries [plane_entry, + count) of the planes
    uint64_t plane_entry;     // index of the first uint16 entry
    uint32_t i0, count;
    uint32_t n;               // the message's frames (RampApplicator's iNumSamples)
    uint32_t m_n1;            // x / (n - 1) == umulhi(x, m_n1) >> s_n1 for x < 2^31 (m_n1 == 0: n - 1 <= 1)
    uint16_t ramp_start, ramp_end;
    uint8_t  s_n1;
    uint8_t  pad[3];
};
static_assert(sizeof(SegMsg) == 24 && sizeof(SrcWork) == 32 && sizeof(SrcSeg) == 24 && sizeof(LeanUnit) == 32 && sizeof(RampJob) == 32, "plan layouts");
struct MfStep {               // the matrix-pipe tables: one step = 16 consecutive output frames of a row (the same for every row: rows start at phase 0)
    uint32_t aoff[16];        // output m's A row: byte offset into a digit's table, phase * 96 + (31 + k0 - n0(m))
    uint32_t b0[16], b1[16], b2[16];   // its accumulators' initial values: bits 0..15 and (signed) bits 16.. of 32896 * sum(c[phase]) + 2^27 -- below 2^28, so
                              // that class 2's accumulator holds them beside its own 2^22 -- and zero (b2: a third read per tile until round 4's end)
    uint32_t kc;              // the step's window is input chunks kc .. kc + 3 (a chunk = 16 frames; frame 0 of chunk 0 = the row's frame -32)
    uint32_t pad[7];
};
static_assert(sizeof(MfStep) == 288, "MfStep");

struct SrcFastParams {        // kernel argument block
    const SrcSeg*  segs;
    const SegMsg*  msgs;
    const SrcWork* work;
    const double*  coef;      // [L][T]
    const uint16_t* ramp_table;
    const uint8_t* src;
    uint8_t*       dst;
    uint64_t src_arena_bytes;
    uint32_t L, M;
    uint32_t L_blk, M_blk;    // outputs / inputs per block
    uint32_t channels, sb, db; // the batch's layout: selects the kernel instantiation
    uint32_t src_le, dst_le;
};

struct SrcFastPlan {
    bool     enabled = false;
    uint32_t T = 0;               // taps per phase
    SrcFastParams params{};
    uint32_t n_work = 0;
    uint32_t n_long = 0;          // ... of which units whose rows are several blocks long
    uint32_t n_lean = 0;          // LeanUnit count (a lean unit may hold several blocks per row: it need not equal n_work)
    uint32_t coef_lds_bytes = 0;  // the coefficient table's share of a workgroup's LDS
    uint32_t wave_lds_bytes = 0;  // per wave: input stages, message table, output ring
    uint32_t max_waves = 0;       // waves per workgroup the LDS allows (<= 12)
    uint32_t ring_bytes = 0;      // bytes of packed output a block row's LDS ring holds
    bool     lean = false;        // the batch runs on src_lean_kernel (round 2) rather than src_block_kernel
    bool     lean_only = false;   // ... and round 1's main list has no instantiation for its layout
    bool     lean_halfband = false;   // ... in its half-band form (the filter is one AND the layout has that instantiation): LDS sizing and dispatch agree on this
    bool     wg_only = false;     // ... or no block kernel but src_mfma_wg_kernel has one: any variant that asks for another kernel gets the generic one
    uint32_t lean_coef_lds_bytes = 0, lean_wave_lds_bytes = 0, lean_max_waves = 0;
    bool     mfma_wg = false;     // ... and src_mfma_wg_kernel runs the lean kernel's units (the filter's digit tables) as it cuts them: one unit per workgroup (rows of ONE block; the units whose input image leaves the arena -- kWorkEdge, in front of the list -- run on it too, through its checked loads)
    bool     mfma_wg_halfband = false;   // ... in its half-band form (the filter's tables are build_mfma_halfband's)
    uint32_t wg_unit_rows = 0;    // ... and the rows its units were cut to (WgGeom::kUnitRows: the launch checks)
    const void* d_mf_amat = nullptr;   // (owned by the ohgpu_src)
    const void* d_mf_steps = nullptr;
    void*    d_planes = nullptr;  // uint16: RampApplicator's multiplier per output frame of every ramped unit, [blocks of the unit][L_blk]
    hipEvent_t planes_ready = nullptr;   // recorded on the context's stream behind the kernel that fills them: a run on any stream waits for it (on the device)
    uint32_t plane_stride = 0;    // the unit of SrcWork::plane / LeanUnit::plane in bytes (16: planes are as long as their units)
    void*    d_slab = nullptr;    // the one allocation the arrays below live in
    void*    d_segs = nullptr;
    void*    d_msgs = nullptr;
    void*    d_work = nullptr;
    void*    d_lean_units = nullptr;   // LeanUnit [n_work], when `lean`
    void*    d_counter = nullptr; // uint32[2]: units claimed / waves finished by the running launch; the kernel's last wave zeroes them
    void*    d_ramp_jobs = nullptr; // RampJob[]: what ramp_plane_kernel filled the planes from (kept for the batch's lifetime)
    void*    d_rem = nullptr;     // DevSrcDesc[] the generic kernel finishes (block-unaligned heads and tails)
    size_t   n_rem = 0;
    uint64_t fast_out_frames = 0;
    // host copies of what carries the messages' ramp endpoints on the device, and whose they are (the caller's message index):
    // ohgpu_src_batch_set_ramps rewrites them; `stream_start`: some message's filter window reaches in front of its stream's first
    // frame (such a batch cannot be advanced: ohgpu_src_batch_advance)
    std::vector<RampJob> host_jobs;
    std::vector<uint32_t> job_msg;
    std::vector<DevSrcDesc> host_rem;
    std::vector<uint32_t> rem_msg;
    // ... and round 1's plan (d_work, not lean), whose kernel reads the endpoints from the SegMsg array itself: that array, and for
    // each ramped message its place in it and the caller's index
    std::vector<SegMsg> host_msgs;
    std::vector<uint32_t> msgs_ramped, msgs_ramped_msg;
    size_t   plane_entries = 0;
    bool     stream_start = false;
    uint64_t advanced_blocks = 0;       // ohgpu_src_batch_advance: blocks added to every message's position since creation
};

int plan_thread_cap();     // ohgpu_set_plan_threads (0: no cap)
// How many threads a host loop over n independent items is worth (at least `per_thread` items each, at most 16 and what the host grants the process)
unsigned usable_cpus();    // csrc/ohgpu_api.hip: the affinity mask's CPUs, capped by the container's CPU quota
inline unsigned plan_threads(size_t n, size_t per_thread)
{
    const unsigned hw = usable_cpus();
    size_t t = n / (per_thread ? per_thread : 1);
    if (t < 1) t = 1;
    if (t > 16) t = 16;
    if (hw && t > hw) t = hw;
    if (ohgpu::plan_thread_cap() > 0 && t > (size_t)ohgpu::plan_thread_cap()) t = (size_t)ohgpu::plan_thread_cap();
    return (unsigned)t;
}
// f(range, lo, hi) over [0, n) cut into n_ranges contiguous ranges, run by up to `threads` threads of the library's planning pool (the
// caller's among them), each claiming the next range when it has done one.  The pool's threads are started on first use and sleep
// between jobs: starting sixteen threads per pass cost more than the passes of a half-million-message plan.
void run_on_pool(unsigned n_ranges, unsigned threads, void (*job)(void* arg, unsigned t), void* arg);     // csrc/ohgpu_api.hip
template <typename F>
inline void parallel_ranges(size_t n, unsigned n_ranges, unsigned threads, F&& f)
{
    if (n_ranges <= 1) { f(0u, (size_t)0, n); return; }
    struct Ctx { F* f; size_t n; unsigned n_ranges; } c{&f, n, n_ranges};
    run_on_pool(n_ranges, threads, [](void* a, unsigned t) {
        Ctx* c = (Ctx*)a;
        (*c->f)(t, c->n * t / c->n_ranges, c->n * (t + 1) / c->n_ranges);
    }, &c);
}
template <typename F>
inline void parallel_ranges(size_t n, unsigned n_thr, F&& f) { parallel_ranges(n, n_thr, n_thr, static_cast<F&&>(f)); }

// x / d == umulhi(x, m) >> s for every x < 2^31 (d >= 2; m == 0 stands for d == 1): with 2^(l-1) < d <= 2^l and
// m = floor(2^(31+l) / d) + 1 the error term x * (m * d - 2^(31+l)) stays below 2^(31+l).  Host side of the line kernels.
inline void magic_u31(uint32_t d, uint32_t* m, uint32_t* s)
{
    if (d <= 1) { *m = 0; *s = 0; return; }
    const uint32_t l = 32u - (uint32_t)__builtin_clz(d - 1u);          // 2^(l-1) < d <= 2^l
    *m = (uint32_t)(((1ull << (31 + l)) / d) + 1);
    *s = l - 1;
}

// ---- line kernel of the PCM message path (csrc/pcm_line_kernel.hip) ----
struct PcmChunk {             // one wave's share of a message: subsamples [q0, q0 + nq); 64 bytes = one scalar load
    // ---- the first 16 bytes are what it takes to START a chunk (issue its loads): the uniform path fetches them for the
    // next trip's chunks ahead of time and the whole record only once the audio is on its way (PcmChunkHead) ----
    uint64_t src_off;             // byte offset of the chunk's first source byte in the arena
    uint32_t nq;
    uint8_t  channels, sb, db, flags;   // bytes per subsample; kChunk* bits
    uint64_t dst_off;             // byte offset of the chunk's first destination byte
    uint32_t q0;
    uint32_t n_frames;            // of the whole message (ramp)
    uint16_t ramp_start, ramp_end;
    uint32_t attenuation;
    uint32_t m_ch, m_n1;          // x / d == umulhi(x, m) >> s for x < 2^31 (m == 0: d == 1); d = channels, n_frames - 1
    uint8_t  s_ch, s_n1;
    uint8_t  prefix_bytes;        // bytes the chunk's wave copies from the batch's prefix blob to just before dst_off (0: none) --
    uint8_t  pad8;                //   a Songcast frame's header, written with the frame's first audio (csrc/ohm_frame_kernel.hip)
    uint32_t plain_sel;           // v_perm_b32 selector of the plain path: source bytes -> destination bytes in memory order
    uint32_t prefix_off;          // of those bytes in the blob (a multiple of 4; entries are padded to whole dwords)
    uint32_t pad;
};
struct PcmChunkHead { uint64_t src_off; uint32_t nq; uint8_t channels, sb, db, flags; };
static_assert(sizeof(PcmChunkHead) == 16, "the head of a chunk record");
static_assert(sizeof(PcmChunk) == 64, "chunk record = one 64-byte scalar load");
enum { kChunkRamp = 1, kChunkSilence = 2, kChunkZeroLsb = 4, kChunkSrcLe = 8, kChunkDstLe = 16 };
constexpr uint32_t kLineLists = 10;   // chunk lists of a plan: [0] the general path, [1 + (sb - 2) * 3 + (db - 2)] the 16/24/32-bit layouts
struct PcmLinePlan {
    bool     enabled = false;
    bool     prefixed = false;    // chunks carry prefixes (d_prefix): only this kernel writes them
    uint32_t n_chunks = 0;
    uint32_t list_first[kLineLists] = {}, list_count[kLineLists] = {};   // d_chunks[list_first[k], + list_count[k]): one launch each
    uint8_t  list_heavy[kLineLists] = {};   // ... and the share of each list's subsamples, in percent, that is ramped or attenuated (the launch's occupancy)
    uint32_t n_staged = 0, n_group = 0, n_heavy = 0, n_prefixed = 0;     // chunks by path (ohgpu_batch_paths): list 0 / plain runs / ramped or attenuated messages
    void*    d_chunks = nullptr;
    void*    d_prefix = nullptr;  // the prefix blob
};
struct MsgPrefix { uint32_t off; uint32_t bytes; };   // per message: [off, off + bytes) of the blob goes right before its destination (bytes <= 255; 0: none)

// ---- line kernel of the layout-changing processors (csrc/fmt_line_kernel.hip) ----
struct FmtChunk {             // 64 bytes = one scalar load
    uint64_t src_off, dst_off;    // first source byte of run 0 / first destination byte
    uint64_t run_src_stride;      // run r starts at src_off + r * run_src_stride (a14: one run per plane)
    uint32_t nq;                  // destination subsamples
    uint32_t run_bytes;           // source bytes per run
    uint16_t n_runs;
    uint16_t run_lds_stride;      // run r is staged run_lds_stride bytes after run r - 1
    uint16_t map_a, map_b, map_c, map_d;   // source subsample of destination subsample q: (q / A) * B + C + (q % A) * D
    uint32_t m_a;                 // q / A == umulhi(q, m_a) >> s_a (m_a == 0: A == 1)
    uint32_t sel;                 // v_perm_b32 selector: source bytes -> destination bytes in memory order
    uint8_t  s_a, sb, db, pad8;
    uint32_t pad[2];
};
static_assert(sizeof(FmtChunk) == 64, "chunk record = one 64-byte scalar load");
struct FmtLinePlan {
    bool     enabled = false;
    uint8_t  group_kind = 0;      // OHGPU_FMT_UNPACK_PLANAR / _FLAC_PACK: a uniform stereo batch on the register-only kernels
    uint8_t  group_bytes = 0;     // its source (a11) / destination (a14) bytes per subsample
    uint32_t n_chunks = 0;
    void*    d_chunks = nullptr;
    uint32_t n_wide = 0;          // a batch of Sender packs that all drop channels: OhmSelRec[n_wide] for ohm_wide_kernel
    void*    d_wide = nullptr;
};

// ---- DSD (csrc/dsd_line_kernel.hip) ----
struct DsdPiece {             // 32 bytes: one wave's share of a descriptor -- chunks [j0, j0 + n), then `fill` bytes of 0x69
    uint64_t src_off, dst_off;    // the DESCRIPTOR's offsets (a DSF chunk's place in its plane pair follows from its index)
    uint32_t j0, n;
    uint32_t fill;                // bytes of 0x69 right behind chunk j0 + n - 1 (the descriptor's last piece; every piece of a silent one)
    uint8_t  kind, pad;           // OHGPU_DSD_*, padBytesPerChunk
    uint8_t  flags;               // kPieceWide: whole lanes of eight chunks go out in 16-byte stores; kPieceSilence
    uint8_t  pad8;
};
static_assert(sizeof(DsdPiece) == 32, "DsdPiece");
struct DsdPlan {
    uint32_t n_pieces = 0;
    uint32_t n_wide = 0, n_generic = 0;   // descriptors with / without a 16-byte-store body (ohgpu_dsd_batch_paths)
    void*    d_pieces = nullptr;
};

// ---- FlywheelRamper (csrc/flywheel_kernel.hip) ----
struct FlywheelLane { uint32_t req, channel; };      // one lane = one channel of one request
struct FlywheelPlan {
    uint32_t n_lanes = 0, lanes_padded = 0, max_count = 0;
    void*    d_lanes = nullptr;
    void*    d_work = nullptr;    // int16 [3][max_count][lanes_padded]: decimated input, per, pef of Burg's method
};

// ---- Songcast sender frames (csrc/ohm_frame_kernel.hip) ----
struct OhmFrameRec {              // 48 bytes: the 36 per-frame header bytes in wire order, and where they go
    uint64_t dst_off;
    uint32_t w[9];
    uint32_t stream_and_bytes;    // bits 0..23: index of the 64-byte stream record (bytes [0, n) = OhmMsgAudio::GetStreamHeader);
                                  // bits 24..31: the whole header's size, 36 + n
};
struct OhmSelRec {               // 48 bytes: one audible fragment of a stream of more than two channels (ohm_wide_kernel)
    uint64_t src_off, dst_off;
    uint32_t n_frames;
    uint32_t m_n1;                // x / (n_frames - 1) == umulhi(x, m_n1) >> s_n1 for x < 2^31 (m_n1 == 0: n_frames - 1 <= 1)
    uint16_t ramp_start, ramp_end, attenuation, pad16;      // (every field inside an aligned dword: the record is read with scalar loads)
    uint8_t  channels, sb, first_ch, flags;
    uint8_t  s_n1, little;
    uint8_t  prefix_bytes;        // the frame's header: [prefix_off, + prefix_bytes) of the batch's blob, written right before dst_off when
    uint8_t  pad8;                //   the fragment is the frame's first audio (0: it is not)
    uint32_t prefix_off;          // (a multiple of 4)
    uint32_t safe_frames;         // frames [0, safe_frames) may be read with one 8-byte load each (it stays inside the source arena)
};
static_assert(sizeof(OhmSelRec) == 48, "OhmSelRec");
struct OhmPlan {
    ohgpu_batch* direct = nullptr;         // pcm batch: fragments of mono/stereo streams, source -> frames (ramp + depth in one pass, headers as prefixes)
    ohgpu_batch* stage = nullptr;          // pcm batch: silent fragments of wider streams -> scratch
    ohgpu_batch* select_staged = nullptr;  // fmt batch: scratch -> frames
    void*    d_selr = nullptr;             // OhmSelRec[n_selr]: audible fragments of wider streams (ohm_wide_kernel: select, attenuation, ramp, header)
    uint32_t n_selr = 0;
    void*    d_wide_prefix = nullptr;      // their frames' headers
    void*    d_scratch = nullptr;
    void*    d_frames = nullptr;           // OhmFrameRec[n_frames] for ohm_header_kernel: [0, n_unfolded) the headers no audio pass writes,
    void*    d_streams = nullptr;          //   then, up to n_unfolded_generic, those `direct` writes unless the generic kernel runs it
    uint32_t n_frames = 0;
    uint32_t n_unfolded = 0, n_unfolded_generic = 0;
};

// ---- what the batch states below share (FlacState, AlacState, OhmRxState, OggState, Mp4State, Mp4fState, FileState; RaopState for its blocks and
// its one event).  The events of a run's phases: n_events are in use, the last of them is recorded at the run's end.  The tracking of
// run_begin / run_end (api_common.h).  The registry of the device blocks that die with the batch: WHERE each pointer member lives (a
// state is heap-allocated and never moves), not what it holds, so a block that a run frees and replaces (FLAC's lists and rows) needs
// nothing more.  state_events, dev_array, state_release and fetch_after_run (api_common.h) are what works on it.
struct RunState {
    static constexpr int kMaxEvents = 7;  // (the family with the most phases has six and the end of a run: fragmented MPEG-4)
    hipEvent_t ev[kMaxEvents] = {};
    int n_events = 0;
    hipStream_t last_stream = nullptr;
    bool ran = false, ended = false;      // (ended: the last run recorded its end -- run_begin, api_common.h)
    std::vector<void**> blocks;
    hipEvent_t end_event() const { return ev[n_events - 1]; }
    RunState() = default;
    RunState(const RunState&) = delete;   // (the registry points into the state)
    RunState& operator=(const RunState&) = delete;
};

// ---- FLAC frames (csrc/flac_frame_kernel.hip): what a batch keeps between runs; the batch's d_descs holds nothing ----
struct FlacScanTile { uint32_t stream, pos0; };       // one workgroup's share of the scan: positions [pos0, pos0 + 1024) of a stream
struct FlacState : RunState {
    std::vector<flaccore::Stream> streams;            // the descriptors (cand_first / cand_count are each run's)
    uint32_t n_tiles = 0, max_blocksize = 0;
    void* d_tables = nullptr;                         // flaccore::Tables
    void* d_tiles = nullptr;                          // FlacScanTile[n_tiles]
    void* d_streams = nullptr;                        // flaccore::Stream[n]
    void* d_results = nullptr;                        // flaccore::Result[n]
    void* d_counter = nullptr;                        // uint32: candidates the scan found
    // grown when a run needs more, kept otherwise
    void* d_list = nullptr;   size_t list_cap = 0;    // uint2 (stream, pos), in the scan's order
    void* d_probes = nullptr; size_t probes_cap = 0;  // flaccore::Probe, sorted
    void* d_rowcand = nullptr; void* d_subs = nullptr; size_t rows_cap = 0;   // per row (candidate, channel): its candidate; flaccore::Sub
    void* d_rows = nullptr;   size_t rows_words = 0;  // int32 [rows][max_blocksize]
    std::vector<flaccore::Probe> host_probes;
    std::vector<uint32_t> host_rowcand;
    std::vector<uint32_t> host_list;
    uint32_t n_candidates = 0;
};

// ---- Apple Lossless packets (csrc/alac_packet_kernel.hip): what a batch keeps between runs; the batch's d_descs holds nothing ----
struct AlacState : RunState {
    std::vector<alaccore::Stream> streams;            // the descriptors
    std::vector<alaccore::Packet> packets;            // the table, by stream, with each packet's rows
    uint32_t n_rows = 0, n_groups = 0, max_frame_length = 0;   // rows with the groups' padding
    bool     plain = false;                           // created under kernel variant 1
    void* d_streams = nullptr;                        // alaccore::Stream[n]
    void* d_packets = nullptr;                        // alaccore::Packet[n_packets]
    void* d_outs = nullptr;                           // alaccore::PacketOut[n_packets]
    void* d_chans = nullptr;                          // alaccore::Chan[n_rows]
    void* d_rowpacket = nullptr;                      // uint32[n_rows]: the row's packet, ~0u for padding
    void* d_groupbase = nullptr;                      // uint64[n_groups + 1]
    void* d_rows = nullptr; size_t rows_bytes = 0;    // int32, the groups one after the other
};
static_assert(sizeof(ohgpu_alac_config) == 24 && sizeof(ohgpu_alac_packet) == 16 && sizeof(ohgpu_alac_stream_desc) == 64 && sizeof(ohgpu_alac_stream_result) == 16 && sizeof(ohgpu_alac_packet_result) == 8, "Apple Lossless layouts");
static_assert(sizeof(alaccore::Stream) == 48 && sizeof(alaccore::Packet) == 32 && sizeof(alaccore::Chan) == 80 && sizeof(alaccore::PacketOut) == sizeof(ohgpu_alac_packet_result), "Apple Lossless device layouts");

// ---- RAOP audio (csrc/raop_decrypt_kernel.hip): the decrypt phase in front of an AlacState.  The batch's AlacState
// holds the DECODING streams only, their packets rewritten to where the decrypt phase leaves them in the plaintext scratch. ----
struct RaopState : RunState {
    std::vector<uint32_t> keys;                       // raopcore::kKeyWords words per stream: the schedule, the IV (cleared in raop_free)
    std::vector<int64_t>  alac_packet;                // per packet of the caller's table: its place in the AlacState's, -1 for a plaintext stream's
    std::vector<uint32_t> alac_first;                 // per stream: its first packet in the AlacState's table (decoding streams)
    std::vector<uint8_t>  plaintext;                  // per stream: OHGPU_RAOP_OUT_PLAINTEXT
    std::vector<uint32_t> first_packet, n_packets;    // per stream, in the caller's table
    uint32_t n_pieces = 0;
    void* d_pieces = nullptr;                         // raopcore::Piece[n_pieces]
    void* d_keys = nullptr; size_t keys_bytes = 0;    // uint32[n * kKeyWords]
    void* d_plain = nullptr; size_t plain_bytes = 0;  // the plaintext scratch: every decoding packet at a 16-byte boundary
    // (ev[0], its one event: before the decrypt phase -- the AlacState's ev[0] is behind it; the run tracking is the AlacState's)
};
static_assert(sizeof(ohgpu_raop_stream_desc) == 96 && sizeof(raopcore::Piece) == 32 && sizeof(raopcore::Job) == 32, "RAOP layouts");

// ---- DSD -> PCM (csrc/dsd_pcm_kernel.hip): a batch is cut on the host into tiles of up to kDsdPcmTile consecutive output frames of
// one message; both kernels loop over them.  The batch's d_descs holds the messages.
constexpr uint32_t kDsdPcmTile = 512;
constexpr uint32_t kDsdPcmTableTaps = 1024;     // the fast route's tables (N / 8 KiB) and its staging fit the LDS up to here
struct DsdPcmTile { uint32_t msg, f0, count, pad; };   // frames [f0, f0 + count) of message msg
static_assert(sizeof(DsdPcmTile) == 16, "DsdPcmTile");
struct DsdPcmPlan {
    uint32_t n_tiles = 0;
    uint32_t n_fast = 0, n_plain = 0;     // messages with frames, by route (ohgpu_dsd_pcm_batch_paths)
    bool     fast = false;                // planned onto dsd_pcm_table_kernel
    void*    d_tiles = nullptr;
};
static_assert(sizeof(ohgpu_dsd_pcm_msg_desc) == 64, "ohgpu_dsd_pcm_msg_desc layout");

// ---- Songcast receiver (csrc/ohm_rx_kernel.hip): the tables, the records and results of the last run, the
// sequencer's rings.  The batch's d_descs holds nothing.
struct OhmRxState : RunState {
    size_t n_streams = 0, n_datagrams = 0;
    void* d_streams = nullptr;                        // ohmrx::Stream[n_streams]
    void* d_datagrams = nullptr;                      // ohmrx::Datagram[n_datagrams]
    void* d_records = nullptr;                        // ohmrx::Record[n_datagrams]
    void* d_results = nullptr;                        // ohmrx::StreamResult[n_streams]
    void* d_rings = nullptr;                          // uint32[n_streams][ohmrx::kRing]
};
static_assert(sizeof(ohgpu_ohm_rx_datagram) == sizeof(ohmrx::Datagram) && sizeof(ohgpu_ohm_rx_state) == sizeof(ohmrx::State) && sizeof(ohgpu_ohm_rx_stream) == sizeof(ohmrx::Stream) &&
              sizeof(ohgpu_ohm_rx_record) == sizeof(ohmrx::Record) && sizeof(ohgpu_ohm_rx_stream_result) == sizeof(ohmrx::StreamResult), "Songcast receiver layouts");

// ---- RAOP receiver (csrc/raop_rx_kernel.hip): the tables, each datagram's stream, the records, keys, rows and results of
// the last run, and the plain route's waiting lists.  The batch's d_descs holds nothing.
struct RaopRxState : RunState {
    size_t n_streams = 0, n_datagrams = 0;
    bool   plain = false;                             // created under kernel variant 1
    void* d_streams = nullptr;                        // raoprx::Stream[n_streams]
    void* d_datagrams = nullptr;                      // raoprx::Datagram[n_datagrams]
    void* d_owner = nullptr;                          // uint32[n_datagrams]: the datagram's stream
    void* d_records = nullptr;                        // raoprx::Record[n_datagrams]
    void* d_keys = nullptr;                           // raoprx::Key[n_datagrams]
    void* d_rows = nullptr;                           // raoprx::PacketRow[n_datagrams]
    void* d_results = nullptr;                        // raoprx::StreamResult[n_streams]
    void* d_slots = nullptr;                          // uint64[n_streams][raoprx::kSlots], the plain route only
};
static_assert(sizeof(ohgpu_raop_rx_datagram) == sizeof(raoprx::Datagram) && sizeof(ohgpu_raop_rx_state) == sizeof(raoprx::State) && sizeof(ohgpu_raop_rx_stream) == sizeof(raoprx::Stream) &&
              sizeof(ohgpu_raop_rx_record) == sizeof(raoprx::Record) && sizeof(ohgpu_raop_rx_stream_result) == sizeof(raoprx::StreamResult) &&
              sizeof(ohgpu_alac_packet) == sizeof(raoprx::PacketRow) && offsetof(ohgpu_raop_rx_record, order) == offsetof(raoprx::Record, order) &&
              offsetof(ohgpu_raop_rx_state, frame) == offsetof(raoprx::State, frame), "RAOP receiver layouts");

// ---- MPEG transport stream and ADTS (csrc/ts_packet_kernel.hip): the descriptors, each stream's first row of the
// per-packet lists, the gather's tiles, the PES table and results of the last run; the map's tiles, the bitmap of valid headers, the
// frame table.  The batch's d_descs holds nothing.
struct TsTile { uint32_t stream, piece0; };           // one wave's share of the gather: destination pieces [piece0, piece0 + 64) of a stream
struct TsState : RunState {
    size_t n_streams = 0, n_pes = 0;
    bool   plain = false;                             // created under kernel variant 1
    uint64_t n_grid = 0;                              // grid packets of all streams
    uint32_t n_tiles = 0, wave_blocks = 0;
    void* d_streams = nullptr;                        // tspkt::Stream[n_streams]
    void* d_results = nullptr;                        // tspkt::Result[n_streams]
    void* d_first = nullptr;                          // uint64[n_streams + 1]: the stream's first row of the three lists below
    void* d_pkt = nullptr;                            // tspkt::Pkt[n_grid]
    void* d_run_end = nullptr;                        // uint32[n_grid]
    void* d_src_at = nullptr;                         // uint32[n_grid]
    void* d_tiles = nullptr;                          // TsTile[n_tiles]
    void* d_pes = nullptr;                            // tspkt::Pes[n_pes]
};
struct AdtsTile { uint32_t stream, pos0; };           // one workgroup's share of the map: positions [pos0, pos0 + 1024) of a stream
struct AdtsState : RunState {
    size_t n_streams = 0, n_frames = 0;
    bool   plain = false;
    uint32_t n_tiles = 0;
    size_t bits_bytes = 0;
    void* d_streams = nullptr;                        // adts::Stream[n_streams]
    void* d_results = nullptr;                        // adts::Result[n_streams]
    void* d_bit_base = nullptr;                       // uint64[n_streams]: the stream's first bit in d_bits (a multiple of 1024)
    void* d_tiles = nullptr;                          // AdtsTile[n_tiles]
    void* d_bits = nullptr;                           // a bit per source byte: a valid header starts here
    void* d_frames = nullptr;                         // adts::Frame[n_frames]
};
static_assert(sizeof(ohgpu_ts_stream_desc) == sizeof(tspkt::Stream) && sizeof(ohgpu_ts_stream_result) == sizeof(tspkt::Result) && sizeof(ohgpu_ts_pes) == sizeof(tspkt::Pes) &&
              offsetof(ohgpu_ts_stream_desc, pes_first) == offsetof(tspkt::Stream, pes_first) && offsetof(ohgpu_ts_stream_result, corrupt_packet) == offsetof(tspkt::Result, corrupt_packet) &&
              offsetof(ohgpu_ts_pes, stream_id) == offsetof(tspkt::Pes, stream_id) && sizeof(ohgpu_adts_stream_desc) == sizeof(adts::Stream) &&
              sizeof(ohgpu_adts_stream_result) == sizeof(adts::Result) && sizeof(ohgpu_adts_frame) == sizeof(adts::Frame) &&
              offsetof(ohgpu_adts_stream_result, profile) == offsetof(adts::Result, profile) && offsetof(ohgpu_adts_frame, header_bytes) == offsetof(adts::Frame, header_bytes) &&
              tspkt::kNone == OHGPU_TS_NONE && tspkt::kNoPts == OHGPU_TS_NO_PTS && tspkt::kCorrupt == OHGPU_TS_CORRUPT && tspkt::kCcJump == OHGPU_TS_PES_CC_JUMP &&
              adts::kLastStart == OHGPU_ADTS_RECOGNISE_LAST_START && adts::kRecogniseFrames == OHGPU_ADTS_RECOGNISE_FRAMES, "transport stream and ADTS layouts");

// ---- Ogg pages (csrc/ogg_page_kernel.hip): the descriptors, the find phase's tiles, the candidate list, the bitmap of
// verified page starts, the gather plan and its dense work list, the packet table and results of the last run.  The batch's d_descs
// holds nothing.
struct OggTile { uint32_t stream, pos0; };            // one workgroup's share of the find: positions [pos0, pos0 + 1024) of a stream
struct OggState : RunState {
    size_t n_streams = 0, n_packets = 0;
    uint32_t n_tiles = 0, cand_cap = 0, piece_cap = 0;
    size_t bits_bytes = 0;
    bool follow_links = false;                        // a stream has OHGPU_OGG_FOLLOW_LINKS: the chain launch is the instance that follows them
    void* d_streams = nullptr;                        // oggpage::Stream[n_streams]
    void* d_results = nullptr;                        // oggpage::Result[n_streams]
    void* d_bit_base = nullptr;                       // uint64[n_streams]: the stream's first bit in d_bits
    void* d_piece_first = nullptr;                    // uint64[n_streams]: the stream's first record in d_pieces
    void* d_tables = nullptr;                         // oggpage::Tables
    void* d_counters = nullptr;                       // uint32[2]: candidates found, pieces in the work list
    void* d_list = nullptr;                           // oggpage::Candidate[cand_cap]
    void* d_pieces = nullptr;                         // oggpage::Piece[piece_cap], a region a stream
    void* d_work = nullptr;                           // uint32[piece_cap]: the pieces to copy, dense
    void* d_tiles = nullptr;                          // OggTile[n_tiles]
    void* d_bits = nullptr;                           // a bit per source byte of every stream: a verified page starts here
    void* d_packets = nullptr;                        // oggpage::Packet[n_packets]
};
static_assert(sizeof(ohgpu_ogg_stream_desc) == sizeof(oggpage::Stream) && sizeof(ohgpu_ogg_stream_result) == sizeof(oggpage::Result) && sizeof(ohgpu_ogg_packet) == sizeof(oggpage::Packet), "Ogg layouts");

// ---- MPEG-4 sample tables (csrc/mp4_table_kernel.hip): the descriptors, the tiles of the sums and the expansion, the
// carries, the record of each stream's tables, both row tables and the results of the last run.  The batch's d_descs holds nothing.
constexpr uint32_t kMp4Tile = mp4box::kTile;          // 1024 samples: tests/test_gpu_mp4_textbook.py restates it
struct Mp4Tile { uint32_t stream, s0; };              // one workgroup's share: samples [s0, s0 + kMp4Tile) of a stream
struct Mp4Plan { uint32_t tile_first, n_tiles, stsc_first, stts_first; };   // a stream's tiles in the tile list, its carries in d_carry_*
struct Mp4State : RunState {
    size_t n_streams = 0, n_packets = 0;
    uint32_t n_tiles = 0, n_stsc = 0, n_stts = 0;
    bool plain = false;                               // created under kernel variant 1: one launch, a lane per stream
    void* d_streams = nullptr;                        // mp4box::Stream[n_streams]
    void* d_results = nullptr;                        // mp4box::Result[n_streams]
    void* d_tables = nullptr;                         // mp4box::Tables[n_streams]
    void* d_plan = nullptr;                           // Mp4Plan[n_streams]
    void* d_tiles = nullptr;                          // Mp4Tile[n_tiles]
    void* d_tile_carry = nullptr;                     // uint64[n_tiles]: the tile's sum, then the sum of the stream's tiles in front of it
    void* d_stsc_carry = nullptr;                     // uint64[n_stsc]: S_k
    void* d_stts_carry = nullptr;                     // uint64[2 * n_stts]: the samples, then the frames, in front of each stts run
    void* d_packets = nullptr;                        // mp4box::Row[n_packets]
    void* d_samples = nullptr;                        // mp4box::Sample[n_packets]
};
static_assert(sizeof(ohgpu_mp4_stream_desc) == sizeof(mp4box::Stream) && sizeof(ohgpu_mp4_stream_result) == sizeof(mp4box::Result) && sizeof(ohgpu_mp4_sample) == sizeof(mp4box::Sample) &&
              sizeof(ohgpu_alac_packet) == sizeof(mp4box::Row) && sizeof(ohgpu_alac_config) == sizeof(mp4box::Config) && offsetof(ohgpu_mp4_stream_result, error_offset) == offsetof(mp4box::Result, error_offset) &&
              offsetof(ohgpu_mp4_stream_result, first_bad_sample) == offsetof(mp4box::Result, first_bad_sample), "MPEG-4 layouts");

// ---- fragmented MPEG-4 (csrc/mp4_frag_kernel.hip): the descriptors, the map of the run slots and the tiles of the
// expansion (both made at create, from the capacities), the walk's records of streams and runs, the three tables and the results of the
// last run.  The batch's d_descs holds nothing.
struct Mp4fTile { uint32_t stream, s0; };             // one workgroup's share: samples [s0, s0 + mp4frag::kTile) of a stream
struct Mp4fState : RunState {
    size_t n_streams = 0, n_packets = 0, n_runs = 0;
    uint32_t n_tiles = 0, wave_blocks = 0;            // (wave_blocks: the size of the two persistent launches, a wave a run slot)
    bool plain = false;                               // created under kernel variant 1: one launch, a lane per stream
    bool gathers = false;                             // some stream gathers: either route needs the destination arena
    void* d_streams = nullptr;                        // mp4frag::Stream[n_streams]
    void* d_results = nullptr;                        // mp4frag::Result[n_streams]
    void* d_recs = nullptr;                           // mp4frag::Rec[n_streams]
    void* d_runrecs = nullptr;                        // mp4frag::RunRec[n_runs], indexed as the run table is
    void* d_slot_stream = nullptr;                    // uint32[n_runs]: the stream whose range the run slot lies in, kNone for a guard row
    void* d_tiles = nullptr;                          // Mp4fTile[n_tiles]
    void* d_runs = nullptr;                           // mp4frag::Run[n_runs]
    void* d_packets = nullptr;                        // mp4box::Row[n_packets]
    void* d_samples = nullptr;                        // mp4box::Sample[n_packets]
};
static_assert(sizeof(ohgpu_mp4f_stream_desc) == sizeof(mp4frag::Stream) && sizeof(ohgpu_mp4f_stream_result) == sizeof(mp4frag::Result) && sizeof(ohgpu_mp4f_run) == sizeof(mp4frag::Run) &&
              sizeof(ohgpu_flac_streaminfo_t) == sizeof(mp4frag::FlacInfo) && offsetof(ohgpu_mp4f_stream_desc, dst_offset) == offsetof(mp4frag::Stream, dst_offset) &&
              offsetof(ohgpu_mp4f_stream_result, flac) == offsetof(mp4frag::Result, flac) && offsetof(ohgpu_mp4f_stream_result, error_offset) == offsetof(mp4frag::Result, error_offset) &&
              offsetof(ohgpu_mp4f_stream_result, first_bad_sample) == offsetof(mp4frag::Result, first_bad_sample) && offsetof(ohgpu_mp4f_run, bytes) == offsetof(mp4frag::Run, bytes) &&
              offsetof(ohgpu_flac_streaminfo_t, md5) == offsetof(mp4frag::FlacInfo, md5) && mp4frag::kMaxBoxes == OHGPU_MP4F_MAX_BOXES && mp4frag::kMaxSamples == OHGPU_MP4F_MAX_SAMPLES && mp4frag::kMaxRunSamples == OHGPU_MP4F_MAX_RUN_SAMPLES &&
              mp4frag::kNotFragmented == OHGPU_MP4F_NOT_FRAGMENTED && mp4frag::kGather == OHGPU_MP4F_GATHER, "fragmented MPEG-4 layouts");

// ---- protected fragmented MPEG-4 (csrc/cenc_kernel.hip): an Mp4fState whose packet table is the expansion's own (places
// in the source arena), and what stands behind it -- the descriptors without their keys, the expanded keys, what the protection boxes gave,
// the public packet table (places in the destination arena), and the unit prefixes of the decrypt-gather (csrc/protected_shell.h: a UNIT is a keystream block, or the second family's work unit).
struct CencState : Mp4fState {
    std::vector<uint32_t> keys;                       // the family's schedule words per stream (cleared in protected_free)
    std::vector<uint32_t> tile_first;                 // per stream: its first tile; n_streams + 1 entries
    uint32_t crypt_blocks = 0;                        // the size of the persistent decrypt-gather launch
    uint64_t n_chunks = 0;                            // its slots: chunks of fragu::kLanes units, from the capacities
    void* d_cstreams = nullptr;                       // cenc::Stream[n_streams] (cbcs::Stream in the second family), the keys zero
    void* d_keys = nullptr; size_t keys_bytes = 0;    // uint32[n_streams * the family's schedule words]
    void* d_extras = nullptr;                         // cenc::Extra[n_streams]
    void* d_rows = nullptr;                           // mp4box::Row[n_packets]: the public packet table
    void* d_row_first = nullptr;                      // [n_packets]: a row's units in front of it in its tile -- cenc::RowRec (with the IV's place), uint64 in the second family
    void* d_tile_first = nullptr;                     // uint32[n_streams + 1]
    void* d_tile_units = nullptr;                     // uint64[n_tiles]: a tile's units, then (the tile scan) those in front of it
    void* d_chunk_first = nullptr;                    // uint64[n_streams + 1]: the stream's first chunk slot
    void* d_nunits = nullptr;                         // uint64[n_streams]: the stream's units
};
static_assert(sizeof(ohgpu_cenc_stream_desc) == 112 && sizeof(ohgpu_cenc_stream_result) == 208 && sizeof(ohgpu_cenc_stream_desc) == sizeof(cenc::Stream) &&
              sizeof(ohgpu_cenc_stream_result) == sizeof(cenc::Result) && offsetof(ohgpu_cenc_stream_desc, key_flags) == offsetof(cenc::Stream, key_flags) &&
              offsetof(ohgpu_cenc_stream_desc, kid) == offsetof(cenc::Stream, kid) && offsetof(ohgpu_cenc_stream_desc, key) == offsetof(cenc::Stream, key) &&
              offsetof(ohgpu_cenc_stream_result, entry) == offsetof(cenc::Result, x) && offsetof(ohgpu_cenc_stream_result, kid) == offsetof(cenc::Result, x) + offsetof(cenc::Extra, kid) &&
              offsetof(ohgpu_cenc_stream_result, blocks) == offsetof(cenc::Result, x) + offsetof(cenc::Extra, blocks) && mp4frag::kNoKey == OHGPU_CENC_NO_KEY &&
              cenc::kHaveKey == OHGPU_CENC_HAVE_KEY && mp4box::kMaxBoxes == OHGPU_MP4_MAX_BOXES, "protected MPEG-4 layouts");

// ---- protected fragmented MPEG-4, the second family (csrc/cbcs_kernel.hip): a CencState (d_cstreams holds cbcs::Stream,
// the schedules are cbcs::kKeyWords words a stream, the units are work units) and what the subsample entries need.
struct CbcsState : CencState {
    size_t n_subsamples = 0;
    void* d_more = nullptr;                           // cbcs::More[n_streams]
    void* d_subs = nullptr;                           // cbcs::SubRow[n_subsamples]
    void* d_samprecs = nullptr;                       // cbcs::SampleRec[n_packets]
    void* d_cipher_blocks = nullptr;                  // uint64[n_streams]: the cipher blocks of the gathered rows
    void* d_sub_first = nullptr;                      // uint32[n_streams]: the stream's first row of the subsample table
};
static_assert(sizeof(ohgpu_cbcs_stream_desc) == 120 && sizeof(ohgpu_cbcs_stream_result) == 232 && sizeof(ohgpu_cbcs_stream_desc) == sizeof(cbcs::Stream) &&
              sizeof(ohgpu_cbcs_stream_result) == sizeof(cbcs::Result) && offsetof(ohgpu_cbcs_stream_desc, subsample_first) == offsetof(cbcs::Stream, sub_first) &&
              offsetof(ohgpu_cbcs_stream_desc, key) == offsetof(cbcs::Stream, c) + offsetof(cenc::Stream, key) &&
              offsetof(ohgpu_cbcs_stream_result, crypt_blocks) == offsetof(cbcs::Result, m) && offsetof(ohgpu_cbcs_stream_result, constant_iv) == offsetof(cbcs::Result, m) + offsetof(cbcs::More, civ) &&
              offsetof(ohgpu_cbcs_stream_result, subsamples) == offsetof(cbcs::Result, m) + offsetof(cbcs::More, subsamples) && cbcs::kSchemeCbcs == OHGPU_CBCS_SCHEME_CBCS &&
              cbcs::kSchemeCenc == OHGPU_CBCS_SCHEME_CENC, "cbcs layouts");

// ---- the two file layers: PCM files (csrc/iff_pcm_kernel.hip) and DSD files (csrc/dsd_file_kernel.hip, DESIGN.md
// 5.18).  One state for both (api_file.h has the plan, the run and the C ABI's bodies over it): the descriptors, the list of the
// conversion's workgroups, the walk's record of each stream's run and the results of the last run, each in the family's own layout
// (iffchunk:: or dsdfile:: Stream / Result / Rec).  The batch's d_descs holds nothing.
constexpr uint32_t kIffGroupPieces = 1024;            // the pieces one workgroup of the PCM conversion takes: tests/test_gpu_iff_textbook.py restates it
constexpr uint32_t kDsdFileGroupPieces = 2;           // the pieces (of dsdfile::kPieceChunks chunks, a wave each) one workgroup of the DSD conversion takes: tests/test_gpu_dsd_file_textbook.py restates both
struct PieceGroup { uint32_t stream, group; };        // one workgroup's share: pieces [group x k*GroupPieces, + k*GroupPieces) of a stream's run
struct FileState : RunState {
    size_t n_streams = 0;
    uint32_t n_groups = 0;
    bool plain = false;                               // created under kernel variant 1: one launch, a lane per stream
    bool writes = false;                              // some stream has room in the destination arena (PCM: a byte; DSD: a sample block): either route needs the arena
    void* d_streams = nullptr;                        // Stream[n_streams]
    void* d_results = nullptr;                        // Result[n_streams]
    void* d_recs = nullptr;                           // Rec[n_streams]
    void* d_groups = nullptr;                         // PieceGroup[n_groups]
};
static_assert(sizeof(ohgpu_iff_stream_desc) == sizeof(iffchunk::Stream) && sizeof(ohgpu_iff_stream_result) == sizeof(iffchunk::Result) &&
              offsetof(ohgpu_iff_stream_desc, max_bit_depth) == offsetof(iffchunk::Stream, max_bit_depth) &&
              offsetof(ohgpu_iff_stream_result, error_offset) == offsetof(iffchunk::Result, error_offset) &&
              offsetof(ohgpu_iff_stream_result, frames_written) == offsetof(iffchunk::Result, frames_written), "IFF layouts");
static_assert(sizeof(ohgpu_dsd_file_stream_desc) == sizeof(dsdfile::Stream) && sizeof(ohgpu_dsd_file_stream_result) == sizeof(dsdfile::Result) &&
              offsetof(ohgpu_dsd_file_stream_desc, pad_bytes_per_chunk) == offsetof(dsdfile::Stream, pad_bytes_per_chunk) &&
              offsetof(ohgpu_dsd_file_stream_result, error_offset) == offsetof(dsdfile::Result, error_offset) &&
              offsetof(ohgpu_dsd_file_stream_result, bytes_written) == offsetof(dsdfile::Result, bytes_written) &&
              dsdfile::kDsf == OHGPU_DSD_DSF && dsdfile::kDff == OHGPU_DSD_DFF && dsdfile::kDsf == OHGPU_DSD_FILE_KIND_DSF && dsdfile::kDff == OHGPU_DSD_FILE_KIND_DFF &&
              dsdfile::kFillByte == OHGPU_DSD_SILENCE_BYTE && dsdfile::kMaxChunks == OHGPU_DSD_FILE_MAX_CHUNKS, "DSD file layouts");

// ---- Vorbis packets (csrc/vorbis_kernel.hip): the descriptors and the table, the setup images as the caller gave them,
// the transform's tables by block size, the records and floors of the last run, and the scratch: a spectrum row and a windowed block per
// packet and channel, and the entropy phase's classification bytes.  The batch's d_descs holds nothing.
struct VorbisTab { uint32_t a, b, w, slope, cos8; };  // where the tables of one block size begin in d_tables, in floats (cos8: the plain route's)
struct VorbisState : RunState {
    std::vector<vorbiscore::Stream> streams;
    std::vector<vorbiscore::Packet> packets;
    bool     plain = false;                           // created under kernel variant 1: the direct-form transform
    uint32_t max_channels = 0, max_block = 0;
    VorbisTab tabs[14] = {};                          // by log2 of the block size
    void* d_images = nullptr;                         // uint32: the images' blob
    void* d_streams = nullptr;                        // vorbiscore::Stream[n]
    void* d_packets = nullptr;                        // vorbiscore::Packet[n_packets]
    void* d_recs = nullptr;                           // vorbiscore::Rec[n_packets]
    void* d_floors = nullptr;                         // vorbiscore::FloorOut[n_packets][kMaxChannels]
    void* d_rows = nullptr; size_t rows_bytes = 0;    // float: per stream, packet and channel a row of bs1 / 2
    void* d_blocks = nullptr;                         // float: ... and a block of bs1
    void* d_cls = nullptr;                            // uint8: per packet its stream's class_bytes
    void* d_tables = nullptr;                         // float: the dB table (256), then the sizes' tables
};
static_assert(sizeof(ohgpu_vorbis_stream_desc) == 64 && sizeof(ohgpu_vorbis_packet_result) == sizeof(vorbiscore::Rec) && sizeof(ohgpu_vorbis_stream_result) == 24 &&
              sizeof(ohgpu_vorbis_info) == 32 && offsetof(ohgpu_vorbis_packet_result, position) == offsetof(vorbiscore::Rec, position) &&
              offsetof(ohgpu_vorbis_packet_result, reserved) == offsetof(vorbiscore::Rec, prev_block) && vorbiscore::kMaxCoupling == OHGPU_VORBIS_MAX_COUPLING_STEPS &&
              vorbiscore::kMaxImageBytes == OHGPU_VORBIS_MAX_IMAGE_BYTES && vorbiscore::kMaxClassBytes == OHGPU_VORBIS_MAX_CLASS_BYTES, "Vorbis layouts");

enum BatchKind { kBatchPcm = 1, kBatchSrc = 2, kBatchFmt = 3, kBatchFlywheel = 4, kBatchOhm = 5, kBatchSrcPull = 6, kBatchDsd = 7, kBatchFlac = 8, kBatchDsdPcm = 9, kBatchAlac = 10, kBatchRaop = 11, kBatchOhmRx = 12, kBatchOgg = 13, kBatchMp4 = 14, kBatchIff = 15, kBatchDsdFile = 16, kBatchMp4f = 17, kBatchCenc = 18, kBatchRaopRx = 19, kBatchTs = 20, kBatchAdts = 21, kBatchVorbis = 22, kBatchCbcs = 23 };

}  // namespace ohgpu

namespace ohgpu {
// Device blocks of the batches' descriptors and plan arrays, kept by the context between batches: a batch that is destroyed gives
// its blocks back (by size class, 256 B << c), the next one of that size takes them -- a steady caller (the StarvationRamper's
// rescue: three batch objects per starving period) allocates on the device once.  Blocks above the largest class go straight to
// hipMalloc / hipFree.  `device_allocs` counts the hipMalloc calls made through it (ohgpu_device_allocations).
struct DevCache {
    static constexpr int kClasses = 15;                // 256 B .. 4 MiB
    std::mutex m;
    std::vector<void*> idle[kClasses];
    std::unordered_map<void*, int> cls;                // every block handed out or idle -> its class (-1: not cached)
    uint64_t device_allocs = 0;
};
}  // namespace ohgpu

namespace ohgpu {
// What the host-buffer calls (ohgpu_*_process_host: a driver thread's period with host memory on its side of the boundary) keep
// from call to call: the two device arenas the audio passes through and a pinned bounce buffer, each grown with headroom when a
// call needs more -- so that a steady caller allocates nothing per period -- and the bytes those calls moved over the link.
struct HostStage {
    void*  d_src = nullptr;    size_t src_cap = 0;
    void*  d_dst = nullptr;    size_t dst_cap = 0;
    void*  h_bounce = nullptr; size_t bounce_cap = 0;
    uint64_t h2d_bytes = 0, d2h_bytes = 0, calls = 0, src_calls = 0;
};
}  // namespace ohgpu

struct ohgpu_ctx {
    ohgpu::DevCache cache;
    ohgpu::HostStage stage;
    int          device;
    hipStream_t  stream;          // the context's own stream (used when the caller passes NULL)
    uint16_t*    d_ramp_table;    // 512 x u16 (RampArray.h:7-74)
    int          variant;         // kernel selection, 0 = best
    int          num_cus;
    char         name[128];
};

struct ohgpu_src {
    uint32_t L, M, T;
    int64_t  max_sum_abs;         // largest sum|c| over the phases, Q28 (the lean kernel's rounding bias needs < 2^29)
    bool     halfband;            // L = 1, M = 2, T = 64 and every odd tap but tap T/2 - 1 zero (host_design.cpp's 2:1 decimator): the
                                  // lean kernel's half-band instantiations multiply by the 33 taps that are not
    double*  d_coef;              // [L][T] exact integer-valued doubles (Q28)
    int32_t* d_coef_q28;          // [L][T] int32
    // the matrix-pipe tables (T = 32 filters whose ratio the 16-output tiling holds, and half-band filters; null otherwise), made for
    // blocks of mf_L_blk outputs
    uint8_t* d_mf_amat = nullptr; // the steps' A operands, lane-linear: [step][4 digits][64 lanes][16 bytes] (build_mfma_images)
    ohgpu::MfStep* d_mf_steps = nullptr;
    uint32_t mf_L_blk = 0;
    bool     mf_halfband = false; // ... in the half-band form: one coefficient image for every step (build_mfma_halfband)
    // a pulled filter (ohgpu_src_pull_create): T taps, 2^phases_log2 phases, the (P + 1) x T Q28 table; L = M = 0 and no fixed-ratio
    // tables.  The fixed-ratio calls refuse it, the pulled ones refuse anything else.
    bool     pulled = false;
    uint32_t phases_log2 = 0;
    int32_t* d_pull_table = nullptr;
};

struct ohgpu_dsd_pcm {
    uint32_t D, T, N;
    int32_t* d_coef = nullptr;    // [N] Q28
    int32_t* d_tables = nullptr;  // [N / 8][256]: byte b of an output's window (its oldest eight bits first) -> its share of the sum; null when N > kDsdPcmTableTaps
};

namespace ohgpu {
// Host arrays of tens of megabytes that are written once, by several threads: 2 MiB-aligned and advised to the kernel as huge-page
// material, so that filling them costs a page fault per 2 MiB instead of one per 4 KiB (seven thousand of them for the headline's
// half a million descriptors, a third of the time their conversion took).
struct HostFree { void operator()(void* p) const { free(p); } };
inline void* host_alloc_huge(size_t bytes)
{
    const size_t huge = (size_t)2 << 20;
    if (bytes < huge) return malloc(bytes ? bytes : 1);
    const size_t len = (bytes + huge - 1) & ~(huge - 1);
    void* p = aligned_alloc(huge, len);
    if (p) (void)madvise(p, len, MADV_HUGEPAGE);
    return p;
}
}  // namespace ohgpu

struct ohgpu_batch {
    int      kind;
    size_t   n;
    void*    d_descs;             // ohgpu_msg_desc[] or DevSrcDesc[] (every message, generic kernels)
    std::unique_ptr<ohgpu::DevSrcDesc[], ohgpu::HostFree> host_descs;   // kBatchSrc: the same on the host (n of them); d_descs is made from it when the generic kernel first runs the whole batch
    mutable std::mutex lazy;      // ... under this
    const ohgpu_src* src;         // kBatchSrc only
    uint64_t src_arena_bytes, dst_arena_bytes;
    uint64_t in_frames, out_frames, src_bytes_touched, dst_bytes_written;
    uint32_t max_frames;          // largest n_frames in the batch
    bool     uniform;             // every descriptor has the same format fields
    bool     src_planar = false;  // resampled batches: the (uniform) source layout is OHGPU_FLAG_SRC_PLANAR32
    uint8_t  channels, src_bits, src_endian, dst_bits, dst_endian;
    ohgpu::SrcFastPlan fast;      // kBatchSrc only
    ohgpu::PcmLinePlan line;      // kBatchPcm only
    ohgpu::FlywheelPlan fly;      // kBatchFlywheel only
    ohgpu::FmtLinePlan fmtline;   // kBatchFmt only
    ohgpu::OhmPlan ohm;           // kBatchOhm only
    ohgpu::DsdPlan dsd;           // kBatchDsd only
    ohgpu::DsdPcmPlan dsdpcm;     // kBatchDsdPcm only
    const ohgpu_dsd_pcm* dsdpcm_filter = nullptr;
    ohgpu::FlacState* flac = nullptr;   // kBatchFlac only (what a run changes lives behind the pointer: a run takes a const batch)
    ohgpu::AlacState* alac = nullptr;   // kBatchAlac and kBatchRaop (likewise)
    ohgpu::RaopState* raop = nullptr;   // kBatchRaop only
    ohgpu::OhmRxState* ohmrx = nullptr; // kBatchOhmRx only
    ohgpu::OggState* ogg = nullptr;     // kBatchOgg only
    ohgpu::Mp4State* mp4 = nullptr;     // kBatchMp4 only
    ohgpu::FileState* file = nullptr;   // kBatchIff and kBatchDsdFile
    ohgpu::Mp4fState* mp4f = nullptr;   // kBatchMp4f only
    ohgpu::CencState* cenc = nullptr;   // kBatchCenc only
    ohgpu::RaopRxState* raoprx = nullptr;   // kBatchRaopRx only
    ohgpu::TsState* ts = nullptr;       // kBatchTs only
    ohgpu::AdtsState* adts = nullptr;   // kBatchAdts only
    ohgpu::VorbisState* vorbis = nullptr;   // kBatchVorbis only
    ohgpu::CbcsState* cbcs = nullptr;   // kBatchCbcs only
    void*    d_pull_tiles = nullptr;   // kBatchSrcPull: PullTile[n_pull_tiles] on the device (d_descs holds the messages)
    uint32_t n_pull_tiles = 0;
    // kBatchSrc whose messages differ in layout: one uniform batch per layout (each with its own block-kernel plan), run one
    // after the other; this batch keeps every descriptor for the generic kernel (ohgpu_set_kernel_variant(1)).
    std::vector<ohgpu_batch*> parts;
    // A resampled batch's unit counters and a flywheel batch's workspace belong to ONE launch at a time.  Launches on the same
    // stream queue behind each other; a launch on another stream while the last one is still running is refused
    // (ohgpu_*_batch_run, OHGPU_ERR_INVALID) instead of silently sharing them.
    mutable hipStream_t last_stream = nullptr;
    mutable hipEvent_t  last_done = nullptr;
    // (the last launch carried the CALLER's events on its dispatch -- ohgpu_src_batch_run_timed -- and not last_done: "has it finished"
    // is then asked of last_stream itself)
    mutable bool last_untracked = false;
};

namespace ohgpu {

int set_error(int code, const char* fmt, ...);

#define OHGPU_HIP_TRY(expr)                                                                         \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) return ::ohgpu::set_error(OHGPU_ERR_DEVICE, "%s failed: %s", #expr,  \
                                                        hipGetErrorString(e_));                     \
    } while (0)
// OHGPU_HIP_TRY_ALLOC: the same for the plans' calls, which allocate -- out of device memory is OHGPU_ERR_NOMEM, any other failure
// OHGPU_ERR_DEVICE (hip_code alone where the caller has a text of its own)
inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? OHGPU_ERR_NOMEM : OHGPU_ERR_DEVICE; }
#define OHGPU_HIP_TRY_ALLOC(expr)                                                                                              \
    do {                                                                                                                       \
        const hipError_t e_ = (expr);                                                                                          \
        if (e_ != hipSuccess) return ::ohgpu::set_error(::ohgpu::hip_code(e_), "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// OHGPU_TRY: the same for a call of the library's own that has set the error already
#define OHGPU_TRY(expr)                          \
    do {                                         \
        const int err_ = (expr);                 \
        if (err_ != OHGPU_OK) return err_;       \
    } while (0)

// The release functions (free_pcm_line, free_fmt_line, free_dsd_line, free_dsd_pcm, raop_free, free_flywheel, free_src_fast, free_ohm): what
// ohgpu_batch_destroy's table calls (csrc/ohgpu_api.hip).  Each takes a PARTLY BUILT batch -- null pointers, a plan that was never
// made -- and leaves the plan reset: a create that fails at any point hands its batch to ohgpu_batch_destroy and returns.
// The families whose state is a RunState (flac, alac, ohmrx, ogg, mp4, mp4f, file, ts, adts) have no function of their own: the table calls
// state_free (api_common.h) on the batch's pointer -- if it is set: state_release, which frees whatever block the state's registry
// names and destroys whatever event exists, then delete, then null the pointer --, and raop_free calls it twice with its key wipe in
// front.  Such a family names no block twice: dev_array in its plan is the one place.
// kernels
hipError_t launch_fmt_v1(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
hipError_t launch_pcm_v1(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
hipError_t launch_pcm_line(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
int plan_pcm_line(ohgpu_ctx* ctx, ohgpu_batch* b, const ohgpu_msg_desc* descs, size_t n,
                  const MsgPrefix* prefixes = nullptr, const uint8_t* blob = nullptr, size_t blob_bytes = 0);
// ohgpu_pcm_batch_create with a prefix per message (csrc/api_pcm.hip; not part of the C ABI: the Songcast frame batch is its one user).
// (*out)->line.prefixed tells whether the line kernel took them; if not, nobody writes them.
int pcm_batch_create_prefixed(ohgpu_ctx* ctx, const ohgpu_msg_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes,
                              const MsgPrefix* prefixes, const uint8_t* blob, size_t blob_bytes, ohgpu_batch** out);
void free_pcm_line(ohgpu_ctx* ctx, ohgpu_batch* b);
int plan_fmt_line(ohgpu_ctx* ctx, ohgpu_batch* b, const ohgpu_fmt_desc* descs, size_t n);
void free_fmt_line(ohgpu_ctx* ctx, ohgpu_batch* b);
hipError_t launch_fmt_line(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
int plan_dsd_line(ohgpu_ctx* ctx, ohgpu_batch* b, const ohgpu_dsd_desc* descs, size_t n);   // csrc/dsd_line_kernel.hip
void free_dsd_line(ohgpu_ctx* ctx, ohgpu_batch* b);
hipError_t launch_dsd_line(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
hipError_t launch_dsd_v1(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
// csrc/dsd_pcm_kernel.hip
void build_dsd_pcm_tables(const int32_t* coef_q28, uint32_t N, std::vector<int32_t>* tables);
int  plan_dsd_pcm(ohgpu_ctx* ctx, ohgpu_batch* b, const ohgpu_dsd_pcm_msg_desc* descs, size_t n);
void free_dsd_pcm(ohgpu_ctx* ctx, ohgpu_batch* b);
hipError_t launch_dsd_pcm_table(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
hipError_t launch_dsd_pcm_v1(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
// csrc/flac_frame_kernel.hip
int  flac_plan(ohgpu_ctx* ctx, ohgpu_batch* b);                       // the device side of a validated batch (b->flac->streams is filled)
int  flac_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s, bool plain);
int  flac_results(ohgpu_ctx* ctx, const ohgpu_batch* b, ohgpu_flac_stream_result* out);
int  flac_frames(ohgpu_ctx* ctx, const ohgpu_batch* b, ohgpu_flac_frame* out, size_t capacity, size_t* n_frames);
// csrc/alac_packet_kernel.hip
int  alac_plan(ohgpu_ctx* ctx, ohgpu_batch* b);                       // the device side of a validated batch (b->alac->streams / packets are filled)
int  alac_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
int  alac_results(ohgpu_ctx* ctx, const ohgpu_batch* b, ohgpu_alac_packet_result* out);     // every packet's, in the table's order
// csrc/raop_decrypt_kernel.hip
const raopcore::Tables& raop_tables();                                // the host's copy of the computed tables (the key schedule is made on the host)
int  raop_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const raopcore::Job* jobs, size_t n_jobs);   // pieces, keys and scratch onto the device (b->raop is filled)
void raop_free(ohgpu_ctx* ctx, ohgpu_batch* b);                       // clears the keys, then state_free of its own state and of the AlacState
int  raop_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);   // the decrypt phase alone
// csrc/ohm_rx_kernel.hip
int  ohm_rx_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const ohmrx::Stream* streams, const ohmrx::Datagram* datagrams);   // tables and result arrays onto the device (b->ohmrx holds the counts)
int  ohm_rx_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
uint32_t ohm_rx_gather_blocks(uint32_t n_datagrams, uint32_t cus);   // the gather launch's size: the rule tests/test_gpu_ohm_rx_many_trips.py restates
// csrc/raop_rx_kernel.hip
int  raop_rx_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const raoprx::Stream* streams, const raoprx::Datagram* datagrams);   // tables and result arrays onto the device (b->raoprx holds the counts and the route)
int  raop_rx_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, hipStream_t s);
// csrc/ts_packet_kernel.hip.  The gather is persistent (a wave a tile of 64 destination pieces, ts_wave_blocks workgroups); parse is a lane
// a grid packet, tables and sums a workgroup a stream; the ADTS map a workgroup a tile, its chain a wave a stream.  The plain routes: a lane a stream.
int  ts_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const tspkt::Stream* streams);
int  ts_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
uint32_t ts_wave_blocks(uint64_t tiles, uint32_t cus);   // the gather launch's size: the rule tests/test_gpu_ts_textbook.py restates
int  adts_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const adts::Stream* streams);
int  adts_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, hipStream_t s);
// csrc/vorbis_kernel.hip.  No launch is persistent: a lane a packet (head, entropy), a lane a stream (the positions), a workgroup a packet
// and channel (synthesis), a workgroup 256 samples of a packet (store).
int  vorbis_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const void* images, uint64_t images_bytes);   // b->vorbis->streams / packets are filled
int  vorbis_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
// csrc/ogg_page_kernel.hip
int  ogg_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const oggpage::Stream* streams);   // tiles, lists and result arrays onto the device (b->ogg holds the counts)
int  ogg_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
uint32_t ogg_wave_blocks(uint64_t items, uint32_t cus);   // the verify and gather launches' size: the rule tests/test_gpu_ogg_textbook.py restates
// csrc/mp4_table_kernel.hip.  No launch is persistent: a workgroup a tile (sums, expand), a wave a stream (carries), a lane a stream (walk).
int  mp4_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const mp4box::Stream* streams);   // tiles, carries and tables onto the device (b->mp4 holds the counts)
int  mp4_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, hipStream_t s);
// csrc/mp4_frag_kernel.hip.  The run sums and the gather are persistent (a wave a run slot, mp4f_wave_blocks workgroups); the rest is a
// lane a stream (walk, carries, finish) or a workgroup a tile (expand).
int  mp4f_plan(ohgpu_ctx* ctx, Mp4fState& g, const mp4frag::Stream* streams, const char* who);   // the slot map, the tiles and the tables onto the device (g holds the counts)
int  mp4f_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
int  mp4f_fill(const Mp4fState& g, hipStream_t s);   // the head of a run of the three families: the run, packet and sample tables back to their fill, on the run's stream
int  mp4f_tables(const Mp4fState& g, const uint8_t* src, hipStream_t s);   // behind a walk: ev[1], run sums, ev[2], carries, ev[3], expand, ev[4], finish, ev[5]
uint32_t mp4f_wave_blocks(uint64_t slots, uint32_t cus);   // the persistent launches' size: the rule tests/test_gpu_mp4f_textbook.py restates
// csrc/cenc_kernel.hip and csrc/cbcs_kernel.hip, over csrc/protected_shell.h.  The walk under the family's Protection (cbcs: with the
// subsample chain), mp4f_tables, then the decrypt-gather: a workgroup a tile (the rows and their unit prefixes), a lane a stream (the
// tiles' prefixes), and the persistent launch (a wave per chunk of 64 units of a stream: keystream blocks, or cbcs's work units).
int  cenc_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const cenc::Stream* streams);
int  cenc_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
int  cbcs_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const cbcs::Stream* streams);
int  cbcs_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
// csrc/iff_pcm_kernel.hip.  No launch is persistent: a lane a stream (walk), a workgroup per kIffGroupPieces pieces of a run (convert).
int  iff_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const iffchunk::Stream* streams);   // the descriptors and the workgroup list onto the device
int  iff_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
// csrc/dsd_file_kernel.hip.  No launch is persistent: a lane a stream (walk), a wave per piece of dsdfile::kPieceChunks chunks (convert).
int  dsd_file_plan(ohgpu_ctx* ctx, ohgpu_batch* b, const dsdfile::Stream* streams);   // the descriptors and the workgroup list onto the device
int  dsd_file_run(ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
// csrc/ohm_frame_kernel.hip: the two wire channels of streams wider than stereo (Sender::DoProcessFragment), one record per fragment
OhmSelRec wide_record(uint64_t src_off, uint64_t dst_off, uint32_t n_frames, uint32_t channels, uint32_t sb, bool little, uint64_t src_arena_bytes);
hipError_t launch_ohm_wide(const ohgpu_ctx* ctx, const void* d_recs, uint32_t n_recs, const uint8_t* src, uint8_t* dst, const uint8_t* prefix, hipStream_t s);
int plan_flywheel(ohgpu_ctx* ctx, ohgpu_batch* b, const ohgpu_flywheel_desc* descs, size_t n);
void free_flywheel(ohgpu_ctx* ctx, ohgpu_batch* b);
hipError_t ctx_dev_alloc(ohgpu_ctx* ctx, void** p, size_t bytes);     // csrc/ohgpu_api.hip: DevCache
void ctx_dev_free(ohgpu_ctx* ctx, void* p);
// The body of every ohgpu_*_process_host (csrc/ohgpu_api.hip; api_common.h's process_host wraps it): src_host goes to the context's
// source arena, `run` launches on the context's stream with the two device arenas, and the bytes the call's outputs cover --
// `ranges` = (dst_offset, bytes) per output, any order -- come back: in one copy straight into dst_host when they tile a span of it,
// through the pinned bounce buffer run by run otherwise.  dst_host bytes no output covers are never written.  Synchronises.
int host_roundtrip(ohgpu_ctx* ctx, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                   std::vector<std::pair<uint64_t, uint64_t>>& ranges, const std::function<int(const void* d_src, void* d_dst)>& run);
hipError_t launch_flywheel(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
hipError_t launch_src_v1(const ohgpu_ctx* ctx, const void* d_descs, size_t n, const ohgpu_src* src_filter,
                         const uint8_t* src, uint8_t* dst, hipStream_t s);
hipError_t launch_src_block(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
hipError_t launch_src_lean(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);
// (`query`: nothing is launched; the instantiation the batch would run is asked what the device grants it -- ohgpu_src_batch_occupancy)
// (`start` / `stop`: the launch itself carries the two events -- hipExtLaunchKernelGGL: its dispatch's own timestamps, no packet more
// in the queue -- ohgpu_src_batch_run_timed)
struct WgOccupancy { bool query = true; int groups_per_cu = 0, designed_for = 0; uint32_t lds_bytes = 0; hipEvent_t start = nullptr, stop = nullptr; };
hipError_t launch_src_mfma_wg(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s, WgOccupancy* query = nullptr);   // csrc/src_mfma_wg_kernel.hip
bool src_mfma_wg_supported(uint32_t L_blk, uint32_t M_blk, uint32_t ch, uint32_t sb, uint32_t db, bool planar, bool halfband);
bool src_mfma_wg_unit_inside(int64_t src_row0, uint32_t row_src_bytes, uint64_t src_arena_bytes, uint32_t ch, uint32_t sb, uint32_t unit_rows, bool planar, uint64_t plane_stride, bool halfband);
bool build_mfma_halfband(const int32_t* coef_q28, uint32_t L_blk, std::vector<MfStep>* steps, std::vector<uint8_t>* amat);   // csrc/src_mfma_kernel.hip
bool build_mfma_tables(uint32_t L, uint32_t M, uint32_t T, const int32_t* coef_q28, uint32_t L_blk, uint32_t kb_cap,
                       std::vector<uint8_t>* adig, std::vector<MfStep>* steps);
void build_mfma_images(const std::vector<uint8_t>& adig, const std::vector<MfStep>& steps, uint32_t L, std::vector<uint8_t>* amat);
bool src_mfma_supported(uint32_t T, uint32_t ch, uint32_t sb, uint32_t db);
uint32_t src_block_outputs(uint32_t L, uint32_t fb_dst);      // outputs per block (0: no block length fits): whole phase periods, >= 128, whole 64-byte lines
hipError_t launch_ramp_planes(const ohgpu_ctx* ctx, const void* d_jobs, uint32_t n_jobs, void* d_planes, hipStream_t s);   // csrc/ramp_plane_kernel.hip
hipError_t load_ramp_plane_kernel();
bool src_lean_geometry(uint32_t L, uint32_t T, bool halfband, uint32_t ch, uint32_t sb, uint32_t db, uint32_t out_per_drain,
                       uint32_t* rows, uint32_t* in_blocks, uint32_t* stage_frames, uint32_t* ring_bytes, uint32_t* coef_lds_bytes,
                       uint32_t* wave_lds_bytes, uint32_t* max_waves);
bool src_block_supported(uint32_t T, uint32_t ch, uint32_t sb, uint32_t src_le, uint32_t db, uint32_t dst_le);
bool src_block_built(uint32_t T, uint32_t ch, uint32_t sb, uint32_t src_le, uint32_t db, uint32_t dst_le);   // ... and round 1's kernel itself is in this library for the layout (the fallback list)
bool src_lean_only_supported(uint32_t T, uint32_t ch, uint32_t sb, uint32_t src_le, uint32_t db, uint32_t dst_le);
bool src_lean_halfband_supported(uint32_t T, uint32_t ch, uint32_t sb, uint32_t src_le, uint32_t db, uint32_t dst_le);
bool src_block_geometry(uint32_t L, uint32_t T, uint32_t ch, uint32_t sb, uint32_t db, uint32_t out_per_drain,
                        uint32_t* rows, uint32_t* ring_bytes, uint32_t* coef_lds_bytes, uint32_t* wave_lds_bytes, uint32_t* max_waves);

// The pulled resampler (csrc/src_pull_kernel.hip): a batch is cut on the host into tiles of up to kPullTile consecutive outputs of
// one message whose input window fits the workgroup's LDS window; a persistent grid loops over them.
constexpr uint32_t kPullTile = 256;
struct PullTile {             // 32 bytes
    uint32_t msg;             // index into the batch's descriptors
    uint32_t j0;              // first output of the tile within its message
    uint32_t count;           // outputs, 1 .. kPullTile
    uint32_t win_frames;      // input frames staged: [win_first, win_first + win_frames)
    int64_t  win_first;       // absolute input frame (negative at a stream start: those frames are zeros)
    uint64_t reserved;
};
static_assert(sizeof(PullTile) == 32, "PullTile");
static_assert(sizeof(ohgpu_src_pull_msg_desc) == 80, "ohgpu_src_pull_msg_desc layout");
uint32_t src_pull_window_cap(uint32_t T);                     // LDS window of a tile, in subsamples
uint32_t src_pull_lds_bytes(uint32_t T, uint32_t phases_log2);  // table + window
hipError_t launch_src_pull(const ohgpu_ctx* ctx, const ohgpu_batch* b, const uint8_t* src, uint8_t* dst, hipStream_t s);

// host helpers
void build_ramp_table(uint16_t out[512]);
int  design_src_pull(uint32_t rate_in, uint32_t rate_out, uint32_t T, uint32_t phases_log2, double beta, double f_pass,
                     double max_pull, std::vector<int32_t>* coef_q28);
int  check_src_pull_table(uint32_t T, uint32_t phases_log2, const int32_t* coef_q28, const char* who);
int  design_dsd_pcm(uint32_t dsd_rate, uint32_t pcm_rate, uint32_t T, double beta, double f_pass, double gain,
                    std::vector<int32_t>* coef_q28, uint32_t* D);       // (coef_q28 null: D only)
int  check_dsd_pcm_filter(uint32_t D, uint32_t T, const int32_t* coef_q28, const char* who);   // the (D, T) rule; with coefficients, sum|c| < 2^30
int  design_src(uint32_t rate_in, uint32_t rate_out, uint32_t T, double beta, double f_pass,
                std::vector<int32_t>* coef_q28, uint32_t* L, uint32_t* M);
void free_src_fast(ohgpu_ctx* ctx, ohgpu_batch* b);
// a batch's last launch: still running on a stream other than `s`?  /  wait for it
// (after a timed run nothing of the library's marks the launch's end, and the caller's stream may be gone by the time anyone asks:
// the device as a whole is waited for instead -- a diagnostic's price, paid only by a destroy, a rewrite of the ramps or a change of
// stream right behind a timed run)
inline bool batch_busy_on_another_stream(const ohgpu_batch* b, hipStream_t s)
{
    if (b->last_stream == s) return false;
    if (b->last_untracked) { (void)hipDeviceSynchronize(); b->last_untracked = false; return false; }
    return b->last_done != nullptr && hipEventQuery(b->last_done) == hipErrorNotReady;
}
inline hipError_t batch_wait_last_launch(const ohgpu_batch* b)
{
    if (b->last_untracked) { b->last_untracked = false; return hipDeviceSynchronize(); }
    return b->last_done ? hipEventSynchronize(b->last_done) : hipSuccess;
}
void free_ohm(ohgpu_ctx* ctx, ohgpu_batch* b);

}  // namespace ohgpu
