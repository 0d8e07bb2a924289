// api_vorbis.hip -- the C ABI's Vorbis I decoder (ohgpu_vorbis_*, include/ohgpu_vorbis.h).
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

// A descriptor's image: inside the blob, whole words, and every table of it walked (vorbiscore::image_valid).
int vorbis_check_image(size_t i, const ohgpu_vorbis_stream_desc& d, const void* images, uint64_t images_bytes, const vorbiscore::Image** out)
{
    if (d.image_offset % 4 != 0 || d.image_bytes % 4 != 0 || d.image_bytes < sizeof(vorbiscore::Image) || d.image_offset > images_bytes || d.image_bytes > images_bytes - d.image_offset)
        return set_error(OHGPU_ERR_INVALID, "vorbis desc %zu: image [%llu, +%u) outside the %llu bytes of images", i, (unsigned long long)d.image_offset, d.image_bytes, (unsigned long long)images_bytes);
    const vorbiscore::Image* im = (const vorbiscore::Image*)((const uint8_t*)images + d.image_offset);
    const bool ok = vorbiscore::image_valid((const uint32_t*)im, d.image_bytes);
    if (!ok) return set_error(OHGPU_ERR_INVALID, "vorbis desc %zu: not a setup image of ohgpu_vorbis_setup_parse", i);
    *out = im;
    return OHGPU_OK;
}

// Of dst_host what each stream wrote (queued on the context's stream): the body of both host-buffer calls' download.
int vorbis_download_written(ohgpu_ctx* ctx, const char* who, const ohgpu_vorbis_stream_desc* descs, size_t n, const void* images, const ohgpu_vorbis_stream_result* sres, void* dst_host)
{
    int e = OHGPU_OK;
    for (size_t i = 0; i < n && e == OHGPU_OK; i++) {
        if (!sres[i].samples) continue;
        const vorbiscore::Image& im = *(const vorbiscore::Image*)((const uint8_t*)images + descs[i].image_offset);
        const bool planes = (descs[i].flags & OHGPU_VORBIS_OUT_PLANAR32) != 0;
        e = download_planes(ctx, who, dst_host, descs[i].dst_offset, descs[i].dst_plane_stride, planes ? im.channels : 1u, planes ? 4u : im.channels * 2u, 0, sres[i].samples);
    }
    return e;
}

}  // namespace

extern "C" {

int ohgpu_vorbis_codewords(const uint8_t* lengths, size_t n, uint32_t* codewords)
{
    if (n && (!lengths || !codewords)) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_codewords: null argument");
    if (vorbiscore::assign_codewords(lengths, n, codewords) != vorbiscore::kParseOk)
        return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_codewords: over-specified tree or a length above 32");
    return OHGPU_OK;
}

int ohgpu_vorbis_setup_parse(const void* id_packet, size_t id_bytes, const void* setup_packet, size_t setup_bytes, void* image, size_t image_capacity, ohgpu_vorbis_info* info)
{
    if (!id_packet || !setup_packet || !info) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_setup_parse: null argument");
    std::vector<uint32_t> words;
    vorbiscore::ParsedInfo pi = {};
    const char* why = "";
    const int rc = vorbiscore::parse_setup((const uint8_t*)id_packet, id_bytes, (const uint8_t*)setup_packet, setup_bytes, &words, &pi, &why);
    if (rc != vorbiscore::kParseOk) return set_error(rc, "ohgpu_vorbis_setup_parse: %s", why);
    memset(info, 0, sizeof(*info));
    info->channels = pi.channels; info->sample_rate = pi.rate; info->blocksize_short = pi.bs0; info->blocksize_long = pi.bs1;
    info->image_bytes = (uint32_t)(words.size() * 4u); info->codebooks = pi.books; info->modes = pi.modes;
    if (!image) return OHGPU_OK;
    if (image_capacity < info->image_bytes) return set_error(OHGPU_ERR_BOUNDS, "ohgpu_vorbis_setup_parse: the image takes %u bytes, there is room for %zu", info->image_bytes, image_capacity);
    memcpy(image, words.data(), info->image_bytes);
    return OHGPU_OK;
}

int ohgpu_vorbis_batch_check(const ohgpu_vorbis_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                             const void* images, uint64_t images_bytes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if ((n && !descs) || (n_packets && !packets) || (n && !images)) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_check: null argument");
    if (n > 0x00ffffffull || n_packets > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_check: too many descriptors");
    if (images_bytes % 4 != 0 || images_bytes > 0xffffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_check: %llu bytes of images (whole words, below 4 GiB)", (unsigned long long)images_bytes);
    uint64_t next = 0;
    for (size_t i = 0; i < n; i++) {
        const ohgpu_vorbis_stream_desc& d = descs[i];
        const vorbiscore::Image* im = nullptr;
        OHGPU_TRY(vorbis_check_image(i, d, images, images_bytes, &im));
        if (d.flags & ~OHGPU_VORBIS_OUT_PLANAR32) return set_error(OHGPU_ERR_INVALID, "vorbis desc %zu: unknown flags 0x%x", i, d.flags);
        for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "vorbis desc %zu: reserved words must be zero", i);
        if (d.first_packet != next || d.n_packets > n_packets - next)
            return set_error(OHGPU_ERR_INVALID, "vorbis desc %zu: packets [%u, +%u) where the table goes on at %llu of %zu", i, d.first_packet, d.n_packets, (unsigned long long)next, n_packets);
        if (d.max_samples > (1ull << 40)) return set_error(OHGPU_ERR_INVALID, "vorbis desc %zu: max_samples out of range", i);
        for (uint32_t k = 0; k < d.n_packets; k++) {
            const ohgpu_alac_packet& p = packets[d.first_packet + k];
            if (p.reserved) return set_error(OHGPU_ERR_INVALID, "vorbis desc %zu: packet %u: reserved word must be zero", i, k);
            OHGPU_TRY(arena_span("vorbis desc", i, "reads", p.src_offset, p.bytes, src_arena_bytes, "source"));
        }
        OHGPU_TRY(decoded_dst_check("vorbis desc", i, im->channels, d.max_samples, (d.flags & OHGPU_VORBIS_OUT_PLANAR32) ? 0u : (uint64_t)im->channels * 2u,
                                    d.dst_offset, d.dst_plane_stride, dst_arena_bytes));
        next += d.n_packets;
    }
    if (next != n_packets) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_check: the descriptors take %llu packets of a table of %zu", (unsigned long long)next, n_packets);
    return OHGPU_OK;
}

int ohgpu_vorbis_batch_create(ohgpu_ctx* ctx, const ohgpu_vorbis_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                              const void* images, uint64_t images_bytes, uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_vorbis_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_vorbis_batch_create", kBatchVorbis, true, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_vorbis_batch_check(descs, n, packets, n_packets, images, images_bytes, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->vorbis = new (std::nothrow) VorbisState();
    if (!b->vorbis) return set_error(OHGPU_ERR_NOMEM, "ohgpu_vorbis_batch_create: out of host memory");
    VorbisState& v = *b->vorbis;
    v.plain = ctx->variant == 1;
    v.streams.resize(n);
    v.packets.resize(n_packets);
    for (size_t i = 0; i < n; i++) {
        const ohgpu_vorbis_stream_desc& d = descs[i];
        const vorbiscore::Image& im = *(const vorbiscore::Image*)((const uint8_t*)images + d.image_offset);
        vorbiscore::Stream& s = v.streams[i];
        memset(&s, 0, sizeof(s));
        s.dst_offset = d.dst_offset; s.dst_plane_stride = d.dst_plane_stride; s.max_samples = d.max_samples; s.image_word = d.image_offset / 4u;
        s.first_packet = d.first_packet; s.n_packets = d.n_packets; s.flags = d.flags;
        s.channels = im.channels; s.bs0 = im.bs0; s.bs1 = im.bs1; s.class_bytes = im.class_bytes;
        for (uint32_t k = 0; k < d.n_packets; k++) {
            vorbiscore::Packet& p = v.packets[d.first_packet + k];
            memset(&p, 0, sizeof(p));
            p.src_offset = packets[d.first_packet + k].src_offset; p.bytes = packets[d.first_packet + k].bytes; p.stream = (uint32_t)i; p.index = k;
            b->src_bytes_touched += p.bytes;
        }
    }
    err = vorbis_plan(ctx, b.get(), images, images_bytes);
    return batch_done(err, b, out);
}

int ohgpu_vorbis_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_vorbis_batch_run", batch, kBatchVorbis, batch && batch->kind == kBatchVorbis && batch->vorbis->packets.empty(), true, src_base, dst_base);
    if (go <= 0) return go;
    return vorbis_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_vorbis_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_vorbis_stream_result* streams, size_t n,
                               ohgpu_vorbis_packet_result* packets, size_t n_packets)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_vorbis_batch_results", batch, kBatchVorbis, "a Vorbis"));
    const VorbisState& v = *batch->vorbis;
    if ((streams || n) && (n != batch->n || !streams)) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_results: room for %zu results, the batch has %zu streams", n, batch->n);
    if ((packets || n_packets) && (n_packets != v.packets.size() || !packets))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_results: room for %zu packet results, the batch has %zu packets", n_packets, v.packets.size());
    std::vector<ohgpu_vorbis_packet_result> all(v.packets.size());
    if (!all.empty()) OHGPU_TRY(fetch_after_run("ohgpu_vorbis_batch_results", v, all.data(), v.d_recs, all.size() * sizeof(all[0])));
    for (ohgpu_vorbis_packet_result& r : all) r.reserved = 0;         // (the later phases' notes)
    if (packets && !all.empty()) memcpy(packets, all.data(), all.size() * sizeof(all[0]));
    for (size_t i = 0; streams && i < batch->n; i++) {
        const vorbiscore::Stream& s = v.streams[i];
        ohgpu_vorbis_stream_result r = {0, 0, 0, 0};
        const ohgpu_vorbis_packet_result* pres = all.data() + s.first_packet;
        while (r.packets_ok < s.n_packets && pres[r.packets_ok].status == OHGPU_VORBIS_OK) r.packets_ok++;
        if (r.packets_ok < s.n_packets) r.first_bad_status = pres[r.packets_ok].status;
        for (uint32_t k = 0; k < s.n_packets; k++) r.samples += pres[k].samples;
        streams[i] = r;
    }
    return OHGPU_OK;
}

int ohgpu_vorbis_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4])
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_vorbis_batch_phase_ms", batch, kBatchVorbis, "a Vorbis"));
    if (!ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_phase_ms: bad argument");
    return phase_ms("ohgpu_vorbis_batch_phase_ms", batch->vorbis->ran, batch->vorbis->ev, 4, ms);
}

int ohgpu_vorbis_batch_paths(const ohgpu_batch* batch, uint32_t* route, uint32_t* blocks)
{
    if (!batch || batch->kind != kBatchVorbis) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_paths: not a Vorbis batch");
    const VorbisState& v = *batch->vorbis;
    if (route) *route = v.plain ? 2u : 1u;
    if (blocks) *blocks = (uint32_t)v.packets.size() * v.max_channels;
    return OHGPU_OK;
}

int ohgpu_vorbis_batch_spectrum(ohgpu_ctx* ctx, const ohgpu_batch* batch, size_t packet, uint32_t channel, float* out, size_t n_values)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_vorbis_batch_spectrum", batch, kBatchVorbis, "a Vorbis"));
    const VorbisState& v = *batch->vorbis;
    if (packet >= v.packets.size() || !out) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_spectrum: packet %zu of %zu", packet, v.packets.size());
    const vorbiscore::Packet& p = v.packets[packet];
    const vorbiscore::Stream& s = v.streams[p.stream];
    if (channel >= s.channels || n_values > s.bs1 / 2u) return set_error(OHGPU_ERR_INVALID, "ohgpu_vorbis_batch_spectrum: channel %u, %zu values (the stream has %u channels and rows of %u)", channel, n_values, s.channels, s.bs1 / 2u);
    const float* row = (const float*)v.d_rows + s.row_base + ((uint64_t)p.index * s.channels + channel) * (s.bs1 / 2u);
    return fetch_after_run("ohgpu_vorbis_batch_spectrum", v, out, row, n_values * sizeof(float));
}

int ohgpu_vorbis_process_host(ohgpu_ctx* ctx, const ohgpu_vorbis_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                              const void* images, uint64_t images_bytes, const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                              ohgpu_vorbis_stream_result* stream_results, ohgpu_vorbis_packet_result* packet_results)
{
    const char* const who = "ohgpu_vorbis_process_host";
    std::vector<ohgpu_vorbis_stream_result> sres(n);
    std::vector<ohgpu_vorbis_packet_result> pres(n_packets);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_vorbis_batch_create(ctx, descs, n, packets, n_packets, images, images_bytes, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n_packets) return (int)OHGPU_OK;
            const int e = ohgpu_vorbis_batch_run(ctx, b, d_src, d_dst, nullptr);
            return e != OHGPU_OK ? e : ohgpu_vorbis_batch_results(ctx, b, n ? sres.data() : nullptr, n, pres.data(), n_packets);
        },
        [&] { return vorbis_download_written(ctx, who, descs, n, images, sres.data(), dst_host); });
    if (err == OHGPU_OK && stream_results && n) memcpy(stream_results, sres.data(), n * sizeof(sres[0]));
    if (err == OHGPU_OK && packet_results && n_packets) memcpy(packet_results, pres.data(), n_packets * sizeof(pres[0]));
    return err;
}

int ohgpu_vorbis_head(const void* bytes, size_t n, void* image, size_t image_capacity, ohgpu_vorbis_info* info, uint32_t* serial,
                      uint64_t* audio_page_offset, uint32_t* audio_segment, uint32_t* audio_seq)
{
    const char* const who = "ohgpu_vorbis_head";
    if (!bytes || !info || !serial || !audio_page_offset || !audio_segment || !audio_seq) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    if (n >= 0x80000000ull) n = 0x7fffffffu;                          // (the head of a stream is asked for: what lies behind 2 GiB is not it)
    static const oggpage::Tables tables = [] { oggpage::Tables t; oggpage::make_tables(&t); return t; }();
    // the walk of csrc/ogg_page_core.h on the host, every page's checksum run as it comes
    oggpage::Stream s = {};
    s.src_bytes = (uint32_t)n;
    s.dst_capacity = n;
    s.flags = oggpage::kAnySeq | oggpage::kAnySerial;
    s.packet_capacity = (uint32_t)std::min<size_t>(n, 65536);
    std::vector<oggpage::Packet> packets(s.packet_capacity);
    std::vector<oggpage::Piece> pieces(oggpage::piece_capacity(s));
    auto good = [&](uint32_t, const uint8_t* page, uint32_t page_bytes) { return oggpage::crc_run(tables.byte, page, 0, page_bytes) == oggpage::stored_crc(page); };
    oggpage::Result r;
    uint32_t n_pieces = 0;
    oggpage::walk(s, 0, (const uint8_t*)bytes, packets.data(), pieces.data(), good, &r, &n_pieces);
    const uint32_t recorded = std::min(r.packets, s.packet_capacity);
    if (recorded < 3 || packets[0].page_offset != 0) return set_error(OHGPU_ERR_INVALID, "%s: %u packets where an Ogg Vorbis stream begins with three headers (walk status %u)", who, recorded, r.status);
    std::vector<uint8_t> run(r.bytes_delivered);
    for (uint32_t k = 0; k < n_pieces; k++) memcpy(run.data() + pieces[k].run_pos, (const uint8_t*)bytes + pieces[k].src_pos, pieces[k].bytes);
    for (uint32_t k = 0; k < 3; k++) {
        const uint8_t* p = run.data() + packets[k].run_pos;
        if (packets[k].bytes < 7 || p[0] != 1u + 2u * k || memcmp(p + 1, "vorbis", 6) != 0) return set_error(OHGPU_ERR_INVALID, "%s: packet %u is not a Vorbis header of type %u", who, k, 1u + 2u * k);
    }
    const int err = ohgpu_vorbis_setup_parse(run.data() + packets[0].run_pos, packets[0].bytes, run.data() + packets[2].run_pos, packets[2].bytes, image, image_capacity, info);
    if (err != OHGPU_OK) return err;
    *serial = r.serial;
    if (recorded > 3) { *audio_page_offset = packets[3].page_offset; *audio_segment = packets[3].segment; *audio_seq = packets[3].page_seq; return OHGPU_OK; }
    if (r.status != OHGPU_OGG_OK) return set_error(OHGPU_ERR_INVALID, "%s: the pages stop (status %u) before the audio begins", who, r.status);
    *audio_page_offset = r.bytes_consumed; *audio_segment = r.resume_segment; *audio_seq = r.next_seq;      // the audio begins where the walk would go on
    return OHGPU_OK;
}

int ohgpu_ogg_vorbis_process_host(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* ogg_descs, const ohgpu_vorbis_stream_desc* vorbis_descs, size_t n, size_t n_packets,
                                  const void* images, uint64_t images_bytes, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes,
                                  void* dst_host, uint64_t dst_bytes, ohgpu_ogg_stream_result* ogg_results, ohgpu_ogg_packet* packets,
                                  ohgpu_vorbis_stream_result* stream_results, ohgpu_vorbis_packet_result* packet_results)
{
    const char* const who = "ohgpu_ogg_vorbis_process_host";
    if (n && (!ogg_descs || !vorbis_descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    for (size_t i = 0; i < n; i++)
        if (ogg_descs[i].flags & OHGPU_OGG_FLAC_MAPPING) return set_error(OHGPU_ERR_INVALID, "%s: stream %zu: the Ogg FLAC mapping in front of the Vorbis decoder", who, i);
    std::vector<ohgpu_ogg_stream_result> ores(n);
    std::vector<ohgpu_ogg_packet> orecs(n_packets);
    std::vector<ohgpu_vorbis_stream_desc> vdescs(vorbis_descs, vorbis_descs + n);
    std::vector<ohgpu_alac_packet> rows;
    std::vector<size_t> row_record;                                    // per row: its place in the Ogg packet table
    std::vector<ohgpu_vorbis_stream_result> sres(n);
    std::vector<ohgpu_vorbis_packet_result> pres;
    void* d_mid = nullptr;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_ogg_batch_create(ctx, ogg_descs, n, n_packets, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, &d_mid, mid_bytes ? mid_bytes : 1));      // the middle arena: the demuxed bytes never leave the device
            int e = ohgpu_ogg_batch_run(ctx, b, d_src, d_mid, nullptr);
            if (e == OHGPU_OK) e = ohgpu_ogg_batch_results(ctx, b, ores.data(), n);             // the one small read between the layers: results ...
            if (e == OHGPU_OK) e = ohgpu_ogg_batch_packets(ctx, b, n_packets ? orecs.data() : nullptr, n_packets);   // ... and packet records
            if (e != OHGPU_OK) return e;
            for (size_t i = 0; i < n; i++) {
                const uint32_t count = std::min(ores[i].packets, ogg_descs[i].packet_capacity);
                vdescs[i].first_packet = (uint32_t)rows.size(); vdescs[i].n_packets = count;
                for (uint32_t k = 0; k < count; k++) {
                    const ohgpu_ogg_packet& o = orecs[ogg_descs[i].packet_first + k];
                    rows.push_back(ohgpu_alac_packet{ogg_descs[i].dst_offset + o.run_pos, o.bytes, 0u});
                    row_record.push_back(ogg_descs[i].packet_first + k);
                }
            }
            pres.resize(rows.size());
            ohgpu_batch* vb = nullptr;
            e = ohgpu_vorbis_batch_create(ctx, vdescs.data(), n, rows.data(), rows.size(), images, images_bytes, mid_bytes, dst_bytes, &vb);
            if (e != OHGPU_OK) return e;
            const BatchPtr own(vb, BatchDeleter{ctx});
            if (rows.empty()) return (int)OHGPU_OK;
            e = ohgpu_vorbis_batch_run(ctx, vb, d_mid, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_vorbis_batch_results(ctx, vb, sres.data(), n, pres.data(), pres.size());
            return e;
        },
        [&] { return vorbis_download_written(ctx, who, vdescs.data(), n, images, sres.data(), dst_host); });
    if (d_mid) { (void)hipStreamSynchronize(ctx->stream); ctx_dev_free(ctx, d_mid); }
    if (err != OHGPU_OK) return err;
    if (ogg_results && n) memcpy(ogg_results, ores.data(), n * sizeof(ores[0]));
    if (packets && n_packets) memcpy(packets, orecs.data(), n_packets * sizeof(orecs[0]));
    if (stream_results && n) memcpy(stream_results, sres.data(), n * sizeof(sres[0]));
    if (packet_results && n_packets) {
        memset(packet_results, 0, n_packets * sizeof(*packet_results));
        for (size_t k = 0; k < pres.size(); k++) packet_results[row_record[k]] = pres[k];
    }
    return OHGPU_OK;
}

int ohgpu_ogg_vorbis_links_process_host(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* ogg_descs, const ohgpu_vorbis_stream_desc* vorbis_descs, const uint64_t* dst_capacity_bytes,
                                        size_t n, size_t n_packets, const void* images, uint64_t images_bytes, const void* src_host, uint64_t src_bytes, uint64_t mid_bytes,
                                        void* dst_host, uint64_t dst_bytes, ohgpu_ogg_stream_result* ogg_results, ohgpu_ogg_packet* packets,
                                        ohgpu_vorbis_link* links, size_t links_capacity, size_t* n_links, ohgpu_vorbis_packet_result* packet_results)
{
    const char* const who = "ohgpu_ogg_vorbis_links_process_host";
    if (n_links) *n_links = 0;
    if (n && (!ogg_descs || !vorbis_descs || !dst_capacity_bytes || !images)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    if (links_capacity && !links) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    if (images_bytes % 4 != 0) return set_error(OHGPU_ERR_INVALID, "%s: %llu bytes of images (whole words)", who, (unsigned long long)images_bytes);
    std::vector<ohgpu_ogg_stream_desc> odescs(ogg_descs, ogg_descs + n);
    for (size_t i = 0; i < n; i++) {
        ohgpu_ogg_stream_desc& o = odescs[i];
        if (o.flags & OHGPU_OGG_FLAC_MAPPING) return set_error(OHGPU_ERR_INVALID, "%s: stream %zu: the Ogg FLAC mapping in front of the Vorbis decoder", who, i);
        if (!(o.flags & OHGPU_OGG_FOLLOW_LINKS)) {                      // (a caller's own magic stays; without the flag the words were to be zero)
            for (uint32_t r : o.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "%s: stream %zu: reserved words must be zero", who, i);
            o.flags |= OHGPU_OGG_FOLLOW_LINKS;
            o.link.bytes = 7;
            memcpy(o.link.magic, "\x01vorbis", 7);
        }
        const vorbiscore::Image* im = nullptr;
        OHGPU_TRY(vorbis_check_image(i, vorbis_descs[i], images, images_bytes, &im));
        if (vorbis_descs[i].dst_offset % 4 != 0) return set_error(OHGPU_ERR_INVALID, "%s: stream %zu: dst_offset must be a multiple of 4", who, i);
        OHGPU_TRY(arena_span("vorbis links stream", i, "writes", vorbis_descs[i].dst_offset, dst_capacity_bytes[i], dst_bytes, "destination"));
    }
    std::vector<ohgpu_ogg_stream_result> ores(n);
    std::vector<ohgpu_ogg_packet> orecs(n_packets);
    std::vector<ohgpu_vorbis_link> rows_out;                          // the link rows, stream by stream
    std::vector<size_t> link_desc;                                     // per link row: its descriptor in vdescs, or SIZE_MAX (not decoded)
    std::vector<ohgpu_vorbis_stream_desc> vdescs;
    std::vector<uint8_t> blob((const uint8_t*)images, (const uint8_t*)images + (n ? images_bytes : 0));   // the caller's images, then the links'
    std::vector<ohgpu_alac_packet> rows;
    std::vector<size_t> row_record;
    std::vector<ohgpu_vorbis_stream_result> sres;
    std::vector<ohgpu_vorbis_packet_result> pres;
    void* d_mid = nullptr;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_ogg_batch_create(ctx, odescs.data(), n, n_packets, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, &d_mid, mid_bytes ? mid_bytes : 1));
            int e = ohgpu_ogg_batch_run(ctx, b, d_src, d_mid, nullptr);
            if (e == OHGPU_OK) e = ohgpu_ogg_batch_results(ctx, b, ores.data(), n);             // the one small read between the layers
            if (e == OHGPU_OK) e = ohgpu_ogg_batch_packets(ctx, b, n_packets ? orecs.data() : nullptr, n_packets);
            if (e != OHGPU_OK) return e;
            for (size_t i = 0; i < n; i++) {
                const ohgpu_ogg_stream_desc& o = odescs[i];
                const ohgpu_vorbis_stream_desc& v0 = vorbis_descs[i];
                const uint8_t* const bytes = (const uint8_t*)src_host + o.src_offset;
                const uint32_t count = std::min(ores[i].packets, o.packet_capacity);
                const ohgpu_ogg_packet* recs = orecs.data() + o.packet_first;
                const bool planes = (v0.flags & OHGPU_VORBIS_OUT_PLANAR32) != 0;
                uint64_t cursor = v0.dst_offset;
                const uint64_t region_end = v0.dst_offset + dst_capacity_bytes[i];
                bool full = false;
                std::vector<uint32_t> cut{0u};                         // link j's records are [cut[j], cut[j + 1]); the continued link may have none
                for (uint32_t k = 0; k < count; k++) {
                    if (recs[k].page_offset > o.src_bytes || o.src_bytes - recs[k].page_offset < (uint64_t)oggpage::kHeaderBytes)
                        return set_error(OHGPU_ERR_DEVICE, "%s: stream %zu: packet record %u begins outside the stream", who, i, k);
                    if (recs[k].flags & OHGPU_OGG_PACKET_LINK) cut.push_back(k);
                }
                cut.push_back(count);
                for (size_t link = 0; link + 1 < cut.size(); link++) {
                    const uint32_t k0 = cut[link], k1 = cut[link + 1], link_packets = k1 - k0;
                    ohgpu_vorbis_link row;
                    memset(&row, 0, sizeof(row));
                    row.stream = (uint32_t)i; row.first_packet = o.packet_first + k0; row.n_packets = link_packets;
                    ohgpu_vorbis_stream_desc d = v0;
                    if (link == 0) {
                        const vorbiscore::Image& im = *(const vorbiscore::Image*)((const uint8_t*)images + v0.image_offset);
                        row.serial = link_packets ? oggpage::le32(bytes + recs[k0].page_offset + 14) : o.serial;
                        row.page_offset = OHGPU_VORBIS_LINK_CONTINUED; row.head = OHGPU_OK;
                        row.channels = im.channels; row.sample_rate = im.rate; row.blocksize_short = im.bs0; row.blocksize_long = im.bs1;
                    } else {
                        row.page_offset = recs[k0].page_offset;
                        row.serial = oggpage::le32(bytes + row.page_offset + 14);
                        // the link's bytes end where the next link's first page begins; its head, on the page its fourth packet begins on
                        uint64_t end = k1 < count ? recs[k1].page_offset : o.src_bytes;
                        if (link_packets > 3) {
                            oggpage::Page pg;
                            const uint64_t at = recs[k0 + 3].page_offset;
                            if (oggpage::parse_page(bytes + at, (uint32_t)(o.src_bytes - at), &pg) == 1) end = at + pg.bytes;
                        }
                        ohgpu_vorbis_info info;
                        uint32_t serial = 0, seg = 0, seq = 0;
                        uint64_t audio = 0;
                        const bool open = link_packets < 3 && k1 == count && ores[i].status == OHGPU_OGG_OK;
                        int head = open ? (int)OHGPU_VORBIS_LINK_HEAD_OPEN : ohgpu_vorbis_head(bytes + row.page_offset, end - row.page_offset, nullptr, 0, &info, &serial, &audio, &seg, &seq);
                        if (head == OHGPU_OK) {
                            const size_t at = blob.size();
                            blob.resize(at + info.image_bytes);
                            head = ohgpu_vorbis_head(bytes + row.page_offset, end - row.page_offset, blob.data() + at, info.image_bytes, &info, &serial, &audio, &seg, &seq);
                            d.image_offset = at; d.image_bytes = info.image_bytes;
                            row.channels = info.channels; row.sample_rate = info.sample_rate; row.blocksize_short = info.blocksize_short; row.blocksize_long = info.blocksize_long;
                        }
                        row.head = head;
                    }
                    // the link's place in the stream's region: sized before the run, cut to what is left, nothing behind a link that was cut
                    row.dst_offset = cursor;
                    size_t mine = SIZE_MAX;
                    if (row.head == OHGPU_OK) {
                        const uint64_t frame = (uint64_t)row.channels * (planes ? 4u : 2u);
                        uint64_t bound = (uint64_t)link_packets * (row.blocksize_long / 2u);
                        if (link == 0) bound = std::min<uint64_t>(bound, v0.max_samples);
                        const uint64_t left = full || cursor >= region_end ? 0 : (region_end - cursor) / frame;
                        if (bound > left) { bound = left; full = true; }
                        if (bound && link_packets) {
                            d.dst_offset = cursor; d.max_samples = bound; d.dst_plane_stride = planes ? bound * 4u : 0u;
                            d.first_packet = (uint32_t)rows.size(); d.n_packets = link_packets;
                            for (uint32_t k = k0; k < k1; k++) {
                                rows.push_back(ohgpu_alac_packet{o.dst_offset + recs[k].run_pos, recs[k].bytes, 0u});
                                row_record.push_back(o.packet_first + k);
                            }
                            mine = vdescs.size();
                            vdescs.push_back(d);
                            cursor += (bound * frame + 3u) & ~(uint64_t)3u;
                        }
                    }
                    rows_out.push_back(row);
                    link_desc.push_back(mine);
                }
            }
            pres.resize(rows.size());
            sres.resize(vdescs.size());
            if (vdescs.empty()) return (int)OHGPU_OK;
            ohgpu_batch* vb = nullptr;
            e = ohgpu_vorbis_batch_create(ctx, vdescs.data(), vdescs.size(), rows.data(), rows.size(), blob.data(), blob.size(), mid_bytes, dst_bytes, &vb);
            if (e != OHGPU_OK) return e;
            const BatchPtr own(vb, BatchDeleter{ctx});
            e = ohgpu_vorbis_batch_run(ctx, vb, d_mid, d_dst, nullptr);                       // one batch over every link of every stream
            if (e == OHGPU_OK) e = ohgpu_vorbis_batch_results(ctx, vb, sres.data(), sres.size(), pres.data(), pres.size());
            return e;
        },
        [&] { return vorbis_download_written(ctx, who, vdescs.data(), vdescs.size(), blob.data(), sres.data(), dst_host); });
    if (d_mid) { (void)hipStreamSynchronize(ctx->stream); ctx_dev_free(ctx, d_mid); }
    if (err != OHGPU_OK) return err;
    for (size_t k = 0; k < rows_out.size(); k++)
        if (link_desc[k] != SIZE_MAX) rows_out[k].samples = sres[link_desc[k]].samples;
    if (n_links) *n_links = rows_out.size();
    if (links) memcpy(links, rows_out.data(), std::min(rows_out.size(), links_capacity) * sizeof(rows_out[0]));
    if (ogg_results && n) memcpy(ogg_results, ores.data(), n * sizeof(ores[0]));
    if (packets && n_packets) memcpy(packets, orecs.data(), n_packets * sizeof(orecs[0]));
    if (packet_results && n_packets) {
        memset(packet_results, 0, n_packets * sizeof(*packet_results));
        for (size_t k = 0; k < pres.size(); k++) packet_results[row_record[k]] = pres[k];
    }
    return OHGPU_OK;
}

}  // extern "C"
