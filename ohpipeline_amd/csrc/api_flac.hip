// api_flac.hip -- the C ABI's FLAC frame decoder (ohgpu_flac_*).
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace ohgpu {

// What a stream decoded, home: a chain's frames are consecutive, so one run of samples (per plane; packed output is one plane)
int flac_download_decoded(ohgpu_ctx* ctx, const char* who, const ohgpu_flac_stream_desc& d, const ohgpu_flac_stream_result& r, void* dst_host)
{
    if (r.frames == 0) return OHGPU_OK;
    const bool packed = d.flags & OHGPU_FLAC_OUT_PACKED_BE;
    return download_planes(ctx, who, dst_host, d.dst_offset, d.dst_plane_stride, packed ? 1u : d.channels, packed ? (uint64_t)d.channels * (d.bits / 8u) : 4u,
                           r.first_sample_decoded - d.first_sample, r.samples);
}

}  // namespace ohgpu

extern "C" {

static int flac_check_desc(const ohgpu_flac_stream_desc& d, size_t i, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (d.channels < 1 || d.channels > OHGPU_MAX_CHANNELS) return set_error(OHGPU_ERR_INVALID, "flac desc %zu: channels %u outside 1..8", i, d.channels);
    if (d.bits != 8 && d.bits != 16 && d.bits != 24) return set_error(OHGPU_ERR_UNSUPPORTED, "flac desc %zu: bit depth %u (8/16/24 only, Codec/Flac.cpp:386-409)", i, d.bits);
    if (d.flags & ~(OHGPU_FLAC_FLAG_AT_FRAME | OHGPU_FLAC_OUT_PACKED_BE)) return set_error(OHGPU_ERR_INVALID, "flac desc %zu: unknown flags 0x%x", i, d.flags);
    for (uint8_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "flac desc %zu: reserved bytes must be zero", i);
    if (d.max_blocksize < 16 || d.max_blocksize > 65535 || d.blocksize > d.max_blocksize)
        return set_error(OHGPU_ERR_INVALID, "flac desc %zu: block size %u, maximum %u (16..65535)", i, d.blocksize, d.max_blocksize);
    if (d.sample_rate == 0 || d.sample_rate > 655350) return set_error(OHGPU_ERR_INVALID, "flac desc %zu: sample rate %u", i, d.sample_rate);
    if (d.src_bytes >= (1ull << 31)) return set_error(OHGPU_ERR_INVALID, "flac desc %zu: a range of %llu bytes (below 2^31)", i, (unsigned long long)d.src_bytes);
    if (d.first_sample >= (1ull << 62)) return set_error(OHGPU_ERR_INVALID, "flac desc %zu: first_sample out of range", i);
    const int err = arena_span("flac desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
    if (err != OHGPU_OK) return err;
    return decoded_dst_check("flac desc", i, d.channels, d.max_samples, (d.flags & OHGPU_FLAC_OUT_PACKED_BE) ? (uint64_t)d.channels * (d.bits / 8u) : 0u,
                             d.dst_offset, d.dst_plane_stride, dst_arena_bytes);
}

int ohgpu_flac_streaminfo(const void* bytes, size_t n, ohgpu_flac_streaminfo_t* info, uint64_t* audio_offset)
{
    const uint8_t* p = (const uint8_t*)bytes;
    if (!p || !info) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_streaminfo: null argument");
    if (n < 4 || memcmp(p, "fLaC", 4) != 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_streaminfo: the stream does not start with fLaC");
    size_t at = 4;
    bool have = false;
    for (;;) {
        if (n - at < 4) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_streaminfo: %zu bytes end inside the metadata", n);
        const uint32_t type = p[at] & 0x7fu, last = p[at] >> 7;
        const size_t len = ((size_t)p[at + 1] << 16) | ((size_t)p[at + 2] << 8) | p[at + 3];
        at += 4;
        if (n - at < len) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_streaminfo: %zu bytes end inside the metadata", n);
        if (!have) {
            // the format puts STREAMINFO first
            if (type != 0 || len != 34) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_streaminfo: the first metadata block (type %u, %zu bytes) is not STREAMINFO", type, len);
            const uint8_t* b = p + at;
            uint64_t v = 0;
            for (int k = 10; k < 18; k++) v = (v << 8) | b[k];
            memset(info, 0, sizeof(*info));
            info->min_blocksize = ((uint32_t)b[0] << 8) | b[1];
            info->max_blocksize = ((uint32_t)b[2] << 8) | b[3];
            info->min_framesize = ((uint32_t)b[4] << 16) | ((uint32_t)b[5] << 8) | b[6];
            info->max_framesize = ((uint32_t)b[7] << 16) | ((uint32_t)b[8] << 8) | b[9];
            info->sample_rate = (uint32_t)(v >> 44);
            info->channels = (uint8_t)(((v >> 41) & 7u) + 1u);
            info->bits = (uint8_t)(((v >> 36) & 31u) + 1u);
            info->total_samples = v & ((1ull << 36) - 1ull);
            memcpy(info->md5, b + 18, 16);
            have = true;
        }
        at += len;
        if (last) break;
    }
    if (audio_offset) *audio_offset = at;
    return OHGPU_OK;
}

int ohgpu_flac_batch_check(const ohgpu_flac_stream_desc* descs, size_t n, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_batch_check: null argument");
    if (n > 0x00ffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_batch_check: too many descriptors");
    for (size_t i = 0; i < n; i++) {
        const int err = flac_check_desc(descs[i], i, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
    }
    return OHGPU_OK;
}

int ohgpu_flac_batch_create(ohgpu_ctx* ctx, const ohgpu_flac_stream_desc* descs, size_t n,
                            uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_flac_batch_create");
    BatchPtr b;     // (the descriptors' pointer and count are ohgpu_flac_batch_check's to refuse)
    int err = batch_begin(ctx, "ohgpu_flac_batch_create", kBatchFlac, true, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_flac_batch_check(descs, n, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->flac = new (std::nothrow) FlacState();
    if (!b->flac) return set_error(OHGPU_ERR_NOMEM, "ohgpu_flac_batch_create: out of host memory");
    b->flac->streams.resize(n);
    for (size_t i = 0; i < n; i++) {
        const ohgpu_flac_stream_desc& d = descs[i];
        flaccore::Stream& s = b->flac->streams[i];
        memset(&s, 0, sizeof(s));
        s.src_offset = d.src_offset; s.dst_offset = d.dst_offset; s.dst_plane_stride = d.dst_plane_stride; s.first_sample = d.first_sample;
        s.src_bytes = (uint32_t)d.src_bytes; s.max_samples = d.max_samples; s.sample_rate = d.sample_rate; s.blocksize = d.blocksize;
        s.max_blocksize = d.max_blocksize; s.channels = d.channels; s.bits = d.bits; s.flags = d.flags;
        b->src_bytes_touched += d.src_bytes;
    }
    err = flac_plan(ctx, b.get());
    return batch_done(err, b, out);
}

int ohgpu_flac_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_flac_batch_run", batch, kBatchFlac, false, true, src_base, dst_base);
    if (go <= 0) return go;
    return flac_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream), ctx->variant == 1);
}

int ohgpu_flac_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_flac_stream_result* results, size_t n)
{
    CTX_GUARD("ohgpu_flac_batch_results");
    if (!batch || batch->kind != kBatchFlac) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_batch_results: not a FLAC batch");
    if (n != batch->n || (n && !results)) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_batch_results: room for %zu results, the batch has %zu streams", n, batch->n);
    return flac_results(ctx, batch, results);
}

int ohgpu_flac_batch_frames(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_flac_frame* frames, size_t capacity, size_t* n_frames)
{
    CTX_GUARD("ohgpu_flac_batch_frames");
    if (!batch || batch->kind != kBatchFlac || (capacity && !frames)) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_batch_frames: bad argument");
    return flac_frames(ctx, batch, frames, capacity, n_frames);
}

int ohgpu_flac_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4])
{
    CTX_GUARD("ohgpu_flac_batch_phase_ms");
    if (!batch || batch->kind != kBatchFlac || !ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_flac_batch_phase_ms: bad argument");
    return phase_ms("ohgpu_flac_batch_phase_ms", batch->flac->ran, batch->flac->ev, 4, ms);
}

int ohgpu_flac_process_host(ohgpu_ctx* ctx, const ohgpu_flac_stream_desc* descs, size_t n,
                            const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                            ohgpu_flac_stream_result* results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    const char* const who = "ohgpu_flac_process_host";
    std::vector<ohgpu_flac_stream_result> res;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_flac_batch_create(ctx, descs, n, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            res = std::vector<ohgpu_flac_stream_result>(n);
            int e = ohgpu_flac_batch_run(ctx, b, d_src, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_flac_batch_results(ctx, b, res.data(), n);
            if (e == OHGPU_OK && (frames || n_frames)) e = ohgpu_flac_batch_frames(ctx, b, frames, frames ? frames_capacity : 0, n_frames);
            return e;
        },
        [&] {   // only what was decoded comes back
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++) e = flac_download_decoded(ctx, who, descs[i], res[i], dst_host);
            return e;
        });
    if (err == OHGPU_OK && results) memcpy(results, res.data(), n * sizeof(ohgpu_flac_stream_result));
    return err;
}

}  // extern "C"
