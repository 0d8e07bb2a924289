// api_cbcs.hip -- the C ABI's second protected fragmented MPEG-4 layer (ohgpu_cbcs_*): the validation of the descriptors
// (the subsample rows are its own), the key schedules (both of them, made here, on the host), the results joined from their three
// arrays, and the head of a stream on the host.  The batch's life around csrc/cbcs_kernel.hip's launches, the three tables, the
// host-buffer call and the two decoder calls are csrc/api_frag.h's bodies, shared with the two sibling families, over the traits below.
#include "api_frag.h"

using namespace ohgpu;

namespace {

struct CbcsFamily : FragStateOf<CbcsState, &ohgpu_batch::cbcs> {
    using Desc = ohgpu_cbcs_stream_desc;
    using Res = ohgpu_cbcs_stream_result;
    static constexpr BatchKind kind = kBatchCbcs;
    static constexpr const char* noun = "a cbcs-protected MPEG-4";
    static const ohgpu_mp4f_stream_result& head(const Res& r) { return r.cenc.mp4f; }
    static std::array<ResultPart, 3> result_parts(const State& g)
    {
        return {{{g.d_results, sizeof(mp4frag::Result), offsetof(Res, cenc) + offsetof(ohgpu_cenc_stream_result, mp4f)},
                 {g.d_extras, sizeof(cenc::Extra), offsetof(Res, cenc) + offsetof(ohgpu_cenc_stream_result, entry)},
                 {g.d_more, sizeof(cbcs::More), offsetof(Res, crypt_blocks)}}};
    }
    static const void* packet_table(const State& g) { return g.d_rows; }
    static uint32_t launch_blocks(const State& g) { return g.crypt_blocks; }
    static int check(const Desc* descs, const FragCounts& c, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
    {
        return ohgpu_cbcs_batch_check(descs, c.n, c.n_packets, c.n_runs, c.n_subsamples, src_arena_bytes, dst_arena_bytes);
    }
    static void keys(State& g, const Desc* descs, const FragCounts& c)
    {
        g.n_subsamples = c.n_subsamples;
        g.keys.assign(c.n * cbcs::kKeyWords, 0u);
        for (size_t i = 0; i < c.n; i++) {
            if (!(descs[i].key_flags & OHGPU_CENC_HAVE_KEY)) continue;
            // the scheme is the stream's to say: the cipher's schedule for `cenc`, the inverse cipher's for `cbcs`
            raopcore::expand_encrypt_key(descs[i].key, &g.keys[i * cbcs::kKeyWords], raop_tables());
            raopcore::expand_decrypt_key(descs[i].key, &g.keys[i * cbcs::kKeyWords + raopcore::kRoundKeyWords], raop_tables());
        }
    }
    static int plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Desc* descs) { return cbcs_plan(ctx, b, (const cbcs::Stream*)descs); }
    static constexpr auto run = cbcs_run;
    static int create(ohgpu_ctx* ctx, const Desc* descs, const FragCounts& c, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
    {
        return ohgpu_cbcs_batch_create(ctx, descs, c.n, c.n_packets, c.n_runs, c.n_subsamples, src_arena_bytes, dst_arena_bytes, out);
    }
    static constexpr auto run_c = ohgpu_cbcs_batch_run;
    static constexpr auto results = ohgpu_cbcs_batch_results;
    static constexpr auto runs = ohgpu_cbcs_batch_runs;
    static constexpr auto packets = ohgpu_cbcs_batch_packets;
    static constexpr auto samples = ohgpu_cbcs_batch_samples;
};

}  // namespace

extern "C" {

int ohgpu_cbcs_batch_check(const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, uint64_t src_arena_bytes,
                           uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_batch_check: null argument");
    if (n > 0x00ffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_batch_check: too many descriptors");
    if (n_subsamples > 0xffffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_cbcs_batch_check: %zu subsample rows are more than one batch takes", n_subsamples);
    std::vector<ohgpu_mp4f_stream_desc> plain(n);
    std::vector<std::pair<uint64_t, uint64_t>> shares;
    for (size_t i = 0; i < n; i++) {
        const ohgpu_cbcs_stream_desc& d = descs[i];
        OHGPU_TRY(protected_desc_check("cbcs desc", d, i));
        if ((uint64_t)d.subsample_first + d.subsample_capacity > n_subsamples)
            return set_error(OHGPU_ERR_INVALID, "cbcs desc %zu: subsample rows [%u, +%u) beyond the table's %zu", i, d.subsample_first, d.subsample_capacity, n_subsamples);
        if (d.subsample_capacity) shares.emplace_back(d.subsample_first, d.subsample_capacity);
        memcpy(&plain[i], &d, sizeof(plain[i]));
    }
    OHGPU_TRY(ohgpu_mp4f_batch_check(plain.data(), n, n_packets, n_runs, src_arena_bytes, dst_arena_bytes));       // (the fields the fragmented families share)
    return ranges_disjoint("ohgpu_cbcs_batch_check", "subsample", shares);
}

int ohgpu_cbcs_batch_create(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    return frag_batch_create<CbcsFamily>(ctx, "ohgpu_cbcs_batch_create", descs, {n, n_packets, n_runs, n_subsamples}, src_arena_bytes, dst_arena_bytes, out);
}

int ohgpu_cbcs_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    return frag_batch_run<CbcsFamily>(ctx, "ohgpu_cbcs_batch_run", batch, src_base, dst_base, stream);
}

int ohgpu_cbcs_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_cbcs_stream_result* results, size_t n)
{
    return frag_batch_results<CbcsFamily>(ctx, "ohgpu_cbcs_batch_results", batch, results, n);
}

int ohgpu_cbcs_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs)
{
    return frag_fetch<CbcsFamily>(ctx, "ohgpu_cbcs_batch_runs", batch, 0, runs, n_runs);
}

int ohgpu_cbcs_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets)
{
    return frag_fetch<CbcsFamily>(ctx, "ohgpu_cbcs_batch_packets", batch, 1, packets, n_packets);
}

int ohgpu_cbcs_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets)
{
    return frag_fetch<CbcsFamily>(ctx, "ohgpu_cbcs_batch_samples", batch, 2, samples, n_packets);
}

int ohgpu_cbcs_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6])
{
    return frag_batch_phase_ms<CbcsFamily>(ctx, "ohgpu_cbcs_batch_phase_ms", batch, ms);
}

int ohgpu_cbcs_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks)
{
    return frag_batch_paths<CbcsFamily>("ohgpu_cbcs_batch_paths", batch, route, tiles, wave_blocks);
}

int ohgpu_cbcs_head(const void* bytes, size_t n, ohgpu_cbcs_stream_result* result)
{
    OHGPU_TRY(frag_head_args("ohgpu_cbcs_head", bytes, n, result));
    cbcs::Stream s = {};
    s.c.s.src_bytes = (uint32_t)n;
    s.c.s.codecs = OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC;
    mp4frag::Rec rec;
    uint32_t rows_cap;
    cbcs::Result* const r = (cbcs::Result*)result;
    cbcs::walk(s, (const uint8_t*)bytes, true, nullptr, nullptr, &r->c.r, &r->c.x, &r->m, &rec, nullptr, &rows_cap);
    return OHGPU_OK;
}

int ohgpu_cbcs_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, size_t n_subsamples, const void* src_host,
                            uint64_t src_bytes, void* dst_host, uint64_t dst_bytes, ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets,
                            ohgpu_mp4_sample* samples)
{
    return frag_process_host<CbcsFamily>(ctx, "ohgpu_cbcs_process_host", descs, {n, n_packets, n_runs, n_subsamples}, src_host, src_bytes, dst_host, dst_bytes, results, runs,
                                         packets, samples);
}

int ohgpu_cbcs_flac_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 size_t n_subsamples, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    return frag_flac_process_host<CbcsFamily>(ctx, "ohgpu_cbcs_flac_process_host", descs, flac_descs, {n, n_packets, n_runs, n_subsamples}, src_host, src_bytes, mid_bytes, dst_host,
                                              dst_bytes, results, runs, packets, samples, flac_results, frames, frames_capacity, n_frames);
}

int ohgpu_cbcs_alac_process_host(ohgpu_ctx* ctx, const ohgpu_cbcs_stream_desc* descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 size_t n_subsamples, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_cbcs_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    return frag_alac_process_host<CbcsFamily>(ctx, "ohgpu_cbcs_alac_process_host", descs, alac_descs, {n, n_packets, n_runs, n_subsamples}, src_host, src_bytes, mid_bytes, dst_host,
                                              dst_bytes, results, runs, packets, samples, alac_results, packet_results);
}

}  // extern "C"
