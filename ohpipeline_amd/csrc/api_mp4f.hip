// api_mp4f.hip -- the C ABI's fragmented MPEG-4 layer (ohgpu_mp4f_*): the validation of the descriptors, the results,
// the head of a stream on the host, and the call that puts the Apple Lossless decoder behind it, which decodes the packets where they
// lie.  The batch's life around csrc/mp4_frag_kernel.hip's launches, the three tables, the host-buffer call and the call in front of
// the FLAC decoder are csrc/api_frag.h's bodies, shared with the two protected families, over the traits below.
#include "api_frag.h"

using namespace ohgpu;

namespace {

int mp4f_check_desc(const ohgpu_mp4f_stream_desc& d, size_t i, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: reserved words must be zero", i);
    if (d.flags & ~OHGPU_MP4F_GATHER) return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: unknown flags 0x%x", i, d.flags);
    if (!d.codecs || (d.codecs & ~(OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC))) return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: codecs 0x%x names no codec, or an unknown one", i, d.codecs);
    if (d.src_bytes >= 0x80000000u) return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: src_bytes %u is 2^31 or more", i, d.src_bytes);
    if (d.packet_capacity && (d.packet_first > n_packets || d.packet_capacity > n_packets - d.packet_first))
        return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: rows [%u, +%u) of tables of %zu", i, d.packet_first, d.packet_capacity, n_packets);
    if (d.run_capacity && (d.run_first > n_runs || d.run_capacity > n_runs - d.run_first))
        return set_error(OHGPU_ERR_INVALID, "mp4f desc %zu: runs [%u, +%u) of a table of %zu", i, d.run_first, d.run_capacity, n_runs);
    const int err = arena_span("mp4f desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
    if (err != OHGPU_OK || !(d.flags & OHGPU_MP4F_GATHER)) return err;
    return arena_span("mp4f desc", i, "gathers into", d.dst_offset, d.dst_capacity, dst_arena_bytes, "destination");
}

struct Mp4fFamily : FragStateOf<Mp4fState, &ohgpu_batch::mp4f> {
    using Desc = ohgpu_mp4f_stream_desc;
    using Res = ohgpu_mp4f_stream_result;
    static constexpr BatchKind kind = kBatchMp4f;
    static constexpr const char* noun = "a fragmented MPEG-4";
    static const ohgpu_mp4f_stream_result& head(const Res& r) { return r; }
    static const void* packet_table(const State& g) { return g.d_packets; }
    static uint32_t launch_blocks(const State& g) { return g.wave_blocks; }
    static int check(const Desc* descs, const FragCounts& c, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
    {
        return ohgpu_mp4f_batch_check(descs, c.n, c.n_packets, c.n_runs, src_arena_bytes, dst_arena_bytes);
    }
    static void keys(State&, const Desc*, const FragCounts&) {}
    static int plan(ohgpu_ctx* ctx, ohgpu_batch* b, const Desc* descs) { return mp4f_plan(ctx, *b->mp4f, (const mp4frag::Stream*)descs, "ohgpu_mp4f_batch_create"); }
    static constexpr auto run = mp4f_run;
    static int create(ohgpu_ctx* ctx, const Desc* descs, const FragCounts& c, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
    {
        return ohgpu_mp4f_batch_create(ctx, descs, c.n, c.n_packets, c.n_runs, src_arena_bytes, dst_arena_bytes, out);
    }
    static constexpr auto run_c = ohgpu_mp4f_batch_run;
    static constexpr auto results = ohgpu_mp4f_batch_results;
    static constexpr auto runs = ohgpu_mp4f_batch_runs;
    static constexpr auto packets = ohgpu_mp4f_batch_packets;
    static constexpr auto samples = ohgpu_mp4f_batch_samples;
};

}  // namespace

extern "C" {

int ohgpu_mp4f_batch_check(const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4f_batch_check: null argument");
    if (n > 0x00ffffffull || n_packets > 0x0fffffffull || n_runs > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_mp4f_batch_check: too many descriptors");
    std::vector<std::pair<uint64_t, uint64_t>> rows, runs, gathers;
    for (size_t i = 0; i < n; i++) {
        const int err = mp4f_check_desc(descs[i], i, n_packets, n_runs, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        if (descs[i].packet_capacity) rows.emplace_back(descs[i].packet_first, descs[i].packet_capacity);
        if (descs[i].run_capacity) runs.emplace_back(descs[i].run_first, descs[i].run_capacity);
        if ((descs[i].flags & OHGPU_MP4F_GATHER) && descs[i].dst_capacity) gathers.emplace_back(descs[i].dst_offset, descs[i].dst_capacity);
    }
    int err = ranges_disjoint("ohgpu_mp4f_batch_check", "row", rows);
    if (err == OHGPU_OK) err = ranges_disjoint("ohgpu_mp4f_batch_check", "run", runs);
    if (err == OHGPU_OK) err = ranges_disjoint("ohgpu_mp4f_batch_check", "gather", gathers);
    return err;
}

int ohgpu_mp4f_batch_create(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, uint64_t src_arena_bytes,
                            uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    return frag_batch_create<Mp4fFamily>(ctx, "ohgpu_mp4f_batch_create", descs, {n, n_packets, n_runs, 0}, src_arena_bytes, dst_arena_bytes, out);
}

int ohgpu_mp4f_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    return frag_batch_run<Mp4fFamily>(ctx, "ohgpu_mp4f_batch_run", batch, src_base, dst_base, stream);
}

int ohgpu_mp4f_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_stream_result* results, size_t n)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_mp4f_batch_results", batch, kBatchMp4f, "a fragmented MPEG-4"));
    const Mp4fState& g = *batch->mp4f;
    return fetch_results("ohgpu_mp4f_batch_results", g, n, g.n_streams, results, g.d_results, sizeof(*results));
}

int ohgpu_mp4f_batch_runs(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4f_run* runs, size_t n_runs)
{
    return frag_fetch<Mp4fFamily>(ctx, "ohgpu_mp4f_batch_runs", batch, 0, runs, n_runs);
}

int ohgpu_mp4f_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_packet* packets, size_t n_packets)
{
    return frag_fetch<Mp4fFamily>(ctx, "ohgpu_mp4f_batch_packets", batch, 1, packets, n_packets);
}

int ohgpu_mp4f_batch_samples(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_mp4_sample* samples, size_t n_packets)
{
    return frag_fetch<Mp4fFamily>(ctx, "ohgpu_mp4f_batch_samples", batch, 2, samples, n_packets);
}

int ohgpu_mp4f_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[6])
{
    return frag_batch_phase_ms<Mp4fFamily>(ctx, "ohgpu_mp4f_batch_phase_ms", batch, ms);
}

int ohgpu_mp4f_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* tiles, uint32_t* wave_blocks)
{
    return frag_batch_paths<Mp4fFamily>("ohgpu_mp4f_batch_paths", batch, route, tiles, wave_blocks);
}

int ohgpu_mp4f_head(const void* bytes, size_t n, ohgpu_mp4f_stream_result* result)
{
    OHGPU_TRY(frag_head_args("ohgpu_mp4f_head", bytes, n, result));
    mp4frag::Stream s = {};
    s.src_bytes = (uint32_t)n;
    s.codecs = OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC;
    mp4frag::Rec rec;
    mp4frag::walk(s, (const uint8_t*)bytes, true, (mp4frag::Result*)result, &rec, nullptr);
    return OHGPU_OK;
}

int ohgpu_mp4f_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* descs, size_t n, size_t n_packets, size_t n_runs, const void* src_host, uint64_t src_bytes,
                            void* dst_host, uint64_t dst_bytes, ohgpu_mp4f_stream_result* results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples)
{
    return frag_process_host<Mp4fFamily>(ctx, "ohgpu_mp4f_process_host", descs, {n, n_packets, n_runs, 0}, src_host, src_bytes, dst_host, dst_bytes, results, runs, packets,
                                         samples);
}

int ohgpu_mp4f_flac_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* mp4f_descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_mp4f_stream_result* mp4f_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    return frag_flac_process_host<Mp4fFamily>(ctx, "ohgpu_mp4f_flac_process_host", mp4f_descs, flac_descs, {n, n_packets, n_runs, 0}, src_host, src_bytes, mid_bytes, dst_host, dst_bytes,
                                              mp4f_results, runs, packets, samples, flac_results, frames, frames_capacity, n_frames);
}

int ohgpu_mp4f_alac_process_host(ohgpu_ctx* ctx, const ohgpu_mp4f_stream_desc* mp4f_descs, const ohgpu_alac_stream_desc* alac_descs, size_t n, size_t n_packets, size_t n_runs,
                                 const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                                 ohgpu_mp4f_stream_result* mp4f_results, ohgpu_mp4f_run* runs, ohgpu_alac_packet* packets, ohgpu_mp4_sample* samples,
                                 ohgpu_alac_stream_result* alac_results, ohgpu_alac_packet_result* packet_results)
{
    const char* const who = "ohgpu_mp4f_alac_process_host";
    if (n && (!mp4f_descs || !alac_descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    for (size_t i = 0; i < n; i++)
        if (mp4f_descs[i].flags & OHGPU_MP4F_GATHER) return set_error(OHGPU_ERR_INVALID, "%s: stream %zu gathers: the packets are decoded where they lie", who, i);
    std::vector<ohgpu_mp4f_stream_result> mres(n);
    std::vector<ohgpu_alac_packet> table(n_packets), dense;
    std::vector<ohgpu_alac_stream_desc> adescs(alac_descs, alac_descs + n);
    std::vector<ohgpu_alac_stream_result> ares(n);
    std::vector<ohgpu_alac_packet_result> pres;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_mp4f_batch_create(ctx, mp4f_descs, n, n_packets, n_runs, src_bytes, 0, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            int e = frag_run_fetch<Mp4fFamily>(ctx, b, d_src, nullptr, {n, n_packets, n_runs, 0}, mres.data(), runs, table.data(), samples);   // the one small read between the layers
            if (e != OHGPU_OK) return e;
            // the Apple Lossless table has the streams' leading accepted rows one after the other without gaps
            for (size_t i = 0; i < n; i++) {
                ohgpu_alac_stream_desc& a = adescs[i];
                const bool ok = mres[i].status == OHGPU_MP4F_OK && mres[i].codec == mp4box::fourcc('a', 'l', 'a', 'c');
                const uint32_t rows = ok ? mres[i].samples_available : 0u;
                // (a stream that brings no packets still stands in the Apple Lossless batch: see ohgpu_mp4_alac_process_host)
                const ohgpu_alac_config none = {1, 0, 16, 0, 0, 1, 1, 0, 0, 0, 0};
                a.config = ok ? mres[i].config : none;
                a.first_packet = (uint32_t)dense.size();
                a.n_packets = rows;
                if (!ok && !a.flags) a.dst_plane_stride = 0;
                dense.insert(dense.end(), table.begin() + mp4f_descs[i].packet_first, table.begin() + mp4f_descs[i].packet_first + rows);
            }
            pres.resize(dense.size());
            if (dense.empty()) return (int)OHGPU_OK;
            ohgpu_batch* ab = nullptr;
            e = ohgpu_alac_batch_create(ctx, adescs.data(), n, dense.data(), dense.size(), src_bytes, dst_bytes, &ab);
            if (e != OHGPU_OK) return e;
            const BatchPtr own(ab, BatchDeleter{ctx});
            e = ohgpu_alac_batch_run(ctx, ab, d_src, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_alac_batch_results(ctx, ab, ares.data(), n, pres.data(), pres.size());
            return e;
        },
        [&] {   // only what was decoded comes back, as in ohgpu_alac_process_host
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (adescs[i].n_packets) e = alac_download_decoded(ctx, who, adescs[i], pres.data() + adescs[i].first_packet, dst_host);
            return e;
        });
    if (err != OHGPU_OK) return err;
    if (mp4f_results && n) memcpy(mp4f_results, mres.data(), n * sizeof(mres[0]));
    if (packets && n_packets) memcpy(packets, table.data(), n_packets * sizeof(table[0]));
    if (alac_results && n) memcpy(alac_results, ares.data(), n * sizeof(ares[0]));
    if (packet_results && n_packets) {
        memset(packet_results, 0, n_packets * sizeof(*packet_results));
        for (size_t i = 0; i < n; i++)
            if (adescs[i].n_packets) memcpy(packet_results + mp4f_descs[i].packet_first, pres.data() + adescs[i].first_packet, adescs[i].n_packets * sizeof(pres[0]));
    }
    return OHGPU_OK;
}

}  // extern "C"
