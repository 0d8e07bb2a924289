// api_cenc.hip -- the C ABI's protected fragmented MPEG-4 layer (ohgpu_cenc_*): the validation of the descriptors, the
// key schedules (made here, on the host), the results joined from their two arrays, and the head of a stream on the host.  The batch's
// life around csrc/cenc_kernel.hip's launches, the three tables, the host-buffer call and the two calls that put the FLAC and the Apple
// Lossless decoder behind it are csrc/api_frag.h's bodies, shared with the two sibling families, over the traits below.
#include "api_frag.h"

using namespace ohgpu;

namespace {

struct CencFamily : FragStateOf<CencState, &ohgpu_batch::cenc> {
    using Desc = ohgpu_cenc_stream_desc;
    using Res = ohgpu_cenc_stream_result;
    static constexpr BatchKind kind = kBatchCenc;
    static constexpr const char* noun = "a protected MPEG-4";
    static const ohgpu_mp4f_stream_result& head(const Res& r) { return r.mp4f; }
    static std::array<ResultPart, 2> result_parts(const State& g)
    {
        return {{{g.d_results, sizeof(mp4frag::Result), offsetof(Res, mp4f)}, {g.d_extras, sizeof(cenc::Extra), offsetof(Res, entry)}}};
    }
    static const void* packet_table(const State& g) { return g.d_rows; }
    static uint32_t launch_blocks(const State& g) { return g.crypt_blocks; }      // (the launch that carries the bytes; the run sums' is the sibling's rule)
    static int check(const Desc* descs, const FragCounts& c, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
    {
        return ohgpu_cenc_batch_check(descs, c.n, c.n_packets, c.n_runs, src_arena_bytes, dst_arena_bytes);
    }
    static void keys(State& g, const Desc* descs, const FragCounts& c)
    {
        g.keys.assign(c.n * cenc::kScheduleWords, 0u);
        for (size_t i = 0; i < c.n; i++)
            if (descs[i].key_flags & OHGPU_CENC_HAVE_KEY) raopcore::expand_encrypt_key(descs[i].key, &g.keys[i * cenc::kScheduleWords], raop_tables());
    }
    static int plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Desc* descs) { return cenc_plan(ctx, b, (const cenc::Stream*)descs); }
    static constexpr auto run = cenc_run;
    static int create(ohgpu_ctx* ctx, const Desc* descs, const FragCounts& c, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
    {
        return ohgpu_cenc_batch_create(ctx, descs, c.n, c.n_packets, c.n_runs, src_arena_bytes, dst_arena_bytes, out);
    }
    static constexpr auto run_c = ohgpu_cenc_batch_run;
    static constexpr auto results = ohgpu_cenc_batch_results;
    static constexpr auto runs = ohgpu_cenc_batch_runs;
    static constexpr auto packets = ohgpu_cenc_batch_packets;
    static constexpr auto samples = ohgpu_cenc_batch_samples;
};

}  // namespace

extern "C" {

int ohgpu_cenc_batch_check(const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_cenc_batch_check: null argument");
    if (n > 0x00ffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_cenc_batch_check: too many descriptors");
    std::vector<ohgpu_mp4f_stream_desc> plain(n);
    for (size_t i = 0; i < n; i++) {
        OHGPU_TRY(protected_desc_check("cenc desc", descs[i], i));
        memcpy(&plain[i], &descs[i], sizeof(plain[i]));
    }
    return ohgpu_mp4f_batch_check(plain.data(), n, n_packets, n_runs, src_arena_bytes, dst_arena_bytes);       // (the fields the two families share)
}

int ohgpu_cenc_batch_create(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    return frag_batch_create<CencFamily>(ctx, "ohgpu_cenc_batch_create", descs, {n, n_packets, n_runs, 0}, src_arena_bytes, dst_arena_bytes, out);
}

int ohgpu_cenc_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    return frag_batch_run<CencFamily>(ctx, "ohgpu_cenc_batch_run", batch, src_base, dst_base, stream);
}

int ohgpu_cenc_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_cenc_stream_result* results, size_t n)
{
    return frag_batch_results<CencFamily>(ctx, "ohgpu_cenc_batch_results", batch, results, n);
}

int ohgpu_cenc_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs)
{
    return frag_fetch<CencFamily>(ctx, "ohgpu_cenc_batch_runs", batch, 0, runs, n_runs);
}

int ohgpu_cenc_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets)
{
    return frag_fetch<CencFamily>(ctx, "ohgpu_cenc_batch_packets", batch, 1, packets, n_packets);
}

int ohgpu_cenc_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets)
{
    return frag_fetch<CencFamily>(ctx, "ohgpu_cenc_batch_samples", batch, 2, samples, n_packets);
}

int ohgpu_cenc_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6])
{
    return frag_batch_phase_ms<CencFamily>(ctx, "ohgpu_cenc_batch_phase_ms", batch, ms);
}

int ohgpu_cenc_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks)
{
    return frag_batch_paths<CencFamily>("ohgpu_cenc_batch_paths", batch, route, tiles, wave_blocks);
}

int ohgpu_cenc_head(const void* bytes, size_t n, ohgpu_cenc_stream_result* result)
{
    OHGPU_TRY(frag_head_args("ohgpu_cenc_head", bytes, n, result));
    cenc::Stream s = {};
    s.s.src_bytes = (uint32_t)n;
    s.s.codecs = OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC;
    mp4frag::Rec rec;
    cenc::Result* const r = (cenc::Result*)result;
    cenc::walk(s, (const uint8_t*)bytes, true, &r->r, &r->x, &rec, nullptr);
    return OHGPU_OK;
}

int ohgpu_cenc_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, const void* src_host, uint64_t src_bytes,
                            void* dst_host, uint64_t dst_bytes, ohgpu_cenc_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    return frag_process_host<CencFamily>(ctx, "ohgpu_cenc_process_host", descs, {n, n_packets, n_runs, 0}, src_host, src_bytes, dst_host, dst_bytes, results, runs, packets,
                                         samples);
}

int ohgpu_cenc_flac_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* cenc_descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cenc_stream_result* cenc_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    return frag_flac_process_host<CencFamily>(ctx, "ohgpu_cenc_flac_process_host", cenc_descs, flac_descs, {n, n_packets, n_runs, 0}, src_host, src_bytes, mid_bytes, dst_host, dst_bytes,
                                              cenc_results, runs, packets, samples, flac_results, frames, frames_capacity, n_frames);
}

int ohgpu_cenc_alac_process_host(ohgpu_ctx* ctx, const ohgpu_cenc_stream_desc* cenc_descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cenc_stream_result* cenc_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    return frag_alac_process_host<CencFamily>(ctx, "ohgpu_cenc_alac_process_host", cenc_descs, alac_descs, {n, n_packets, n_runs, 0}, src_host, src_bytes, mid_bytes, dst_host, dst_bytes,
                                              cenc_results, runs, packets, samples, alac_results, packet_results);
}

}  // extern "C"
