// api_ogg.hip -- the C ABI's Ogg page layer (ohgpu_ogg_*): the validation of the descriptors, the batch's life
// around csrc/ogg_page_kernel.hip's four launches, the results and the packet table, the host-buffer call, the checksum.
#include <algorithm>
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

int ogg_check_desc(const ohgpu_ogg_stream_desc& d, size_t i, size_t n_packets, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (d.flags & ~(uint32_t)oggpage::kKnownFlags) return set_error(OHGPU_ERR_INVALID, "ogg desc %zu: unknown flags 0x%x", i, d.flags);
    if (d.flags & OHGPU_OGG_FOLLOW_LINKS) {
        if (d.link.bytes > (uint32_t)oggpage::kMaxMagicBytes) return set_error(OHGPU_ERR_INVALID, "ogg desc %zu: a link magic of %u bytes where 8 is the most", i, d.link.bytes);
        for (uint32_t k = d.link.bytes; k < (uint32_t)oggpage::kMaxMagicBytes; k++)
            if (d.link.magic[k]) return set_error(OHGPU_ERR_INVALID, "ogg desc %zu: the link magic has a non-zero byte beyond its %u bytes", i, d.link.bytes);
    } else
        for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "ogg desc %zu: reserved words must be zero", i);
    if (d.src_bytes >= 0x80000000u) return set_error(OHGPU_ERR_INVALID, "ogg desc %zu: src_bytes %u is 2^31 or more", i, d.src_bytes);
    if (d.first_page_segment > 255u) return set_error(OHGPU_ERR_INVALID, "ogg desc %zu: first_page_segment %u where a page has at most 255 segments", i, d.first_page_segment);
    if (d.packet_capacity && (d.packet_first > n_packets || d.packet_capacity > n_packets - d.packet_first))
        return set_error(OHGPU_ERR_INVALID, "ogg desc %zu: packets [%u, +%u) of a table of %zu", i, d.packet_first, d.packet_capacity, n_packets);
    int err = arena_span("ogg desc", i, "reads", d.src_offset, d.src_bytes, src_arena_bytes, "source");
    if (err == OHGPU_OK) err = arena_span("ogg desc", i, "writes", d.dst_offset, d.dst_capacity, dst_arena_bytes, "destination");
    if (err != OHGPU_OK) return err;
    if (d.dst_capacity < d.src_bytes)
        return set_error(OHGPU_ERR_BOUNDS, "ogg desc %zu: dst_capacity %llu where the stream has %u bytes", i, (unsigned long long)d.dst_capacity, d.src_bytes);
    return OHGPU_OK;
}

}  // namespace

extern "C" {

int ohgpu_ogg_batch_check(const ohgpu_ogg_stream_desc* descs, size_t n, size_t n_packets, uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if (n && !descs) return set_error(OHGPU_ERR_INVALID, "ohgpu_ogg_batch_check: null argument");
    if (n > 0x00ffffffull || n_packets > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_ogg_batch_check: too many descriptors");
    std::vector<std::pair<uint64_t, uint64_t>> ranges;                 // (first, capacity) of the streams that record packets
    for (size_t i = 0; i < n; i++) {
        const int err = ogg_check_desc(descs[i], i, n_packets, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        if (descs[i].packet_capacity) ranges.emplace_back(descs[i].packet_first, descs[i].packet_capacity);
    }
    return ranges_disjoint("ohgpu_ogg_batch_check", "packet", ranges);
}

int ohgpu_ogg_batch_create(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* descs, size_t n, size_t n_packets, uint64_t src_arena_bytes, uint64_t dst_arena_bytes,
                           ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_ogg_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_ogg_batch_create", kBatchOgg, n == 0 || descs, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_ogg_batch_check(descs, n, n_packets, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->ogg = new (std::nothrow) OggState();
    if (!b->ogg) return set_error(OHGPU_ERR_NOMEM, "ohgpu_ogg_batch_create: out of host memory");
    b->ogg->n_streams = n;
    b->ogg->n_packets = n_packets;
    for (size_t i = 0; i < n; i++) b->src_bytes_touched += descs[i].src_bytes;
    err = ogg_plan(ctx, b.get(), (const oggpage::Stream*)descs);
    return batch_done(err, b, out);
}

int ohgpu_ogg_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const bool empty = batch && batch->kind == kBatchOgg && batch->ogg->n_streams == 0;
    const int go = run_guard(ctx, "ohgpu_ogg_batch_run", batch, kBatchOgg, empty, true, src_base, dst_base);
    if (go <= 0) return go;
    return ogg_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_ogg_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ogg_stream_result* results, size_t n)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_ogg_batch_results", batch, kBatchOgg, "an Ogg"));
    const OggState& g = *batch->ogg;
    return fetch_results("ohgpu_ogg_batch_results", g, n, g.n_streams, results, g.d_results, sizeof(*results));
}

int ohgpu_ogg_batch_packets(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_ogg_packet* packets, size_t n_packets)
{
    OHGPU_TRY(state_guard(ctx, "ohgpu_ogg_batch_packets", batch, kBatchOgg, "an Ogg"));
    const OggState& g = *batch->ogg;
    return fetch_table("ohgpu_ogg_batch_packets", g, "records, the batch's table has", "", n_packets, g.n_packets, g.n_streams, packets, g.d_packets, sizeof(*packets));
}

int ohgpu_ogg_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4])
{
    CTX_GUARD("ohgpu_ogg_batch_phase_ms");
    if (!batch || batch->kind != kBatchOgg || !ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_ogg_batch_phase_ms: bad argument");
    return phase_ms("ohgpu_ogg_batch_phase_ms", batch->ogg->ran, batch->ogg->ev, 4, ms);
}

int ohgpu_ogg_process_host(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* descs, size_t n, size_t n_packets, const void* src_host, uint64_t src_bytes,
                           void* dst_host, uint64_t dst_bytes, ohgpu_ogg_stream_result* results, ohgpu_ogg_packet* packets)
{
    const char* const who = "ohgpu_ogg_process_host";
    std::vector<ohgpu_ogg_stream_result> sres(n);
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_ogg_batch_create(ctx, descs, n, n_packets, src_bytes, dst_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            int e = ohgpu_ogg_batch_run(ctx, b, d_src, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_ogg_batch_results(ctx, b, n ? sres.data() : nullptr, n);
            if (e == OHGPU_OK && packets) e = ohgpu_ogg_batch_packets(ctx, b, n_packets ? packets : nullptr, n_packets);
            return e;
        },
        [&] {   // only what was delivered comes back (as one "plane" of one-byte samples per stream)
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++)
                if (sres[i].bytes_delivered) e = download_planes(ctx, who, dst_host, descs[i].dst_offset, 0, 1, 1, 0, sres[i].bytes_delivered);
            return e;
        });
    if (err == OHGPU_OK && results && n) memcpy(results, sres.data(), n * sizeof(sres[0]));
    return err;
}

int ohgpu_ogg_flac_head(const void* bytes, size_t n, ohgpu_flac_streaminfo_t* info, uint32_t* serial, uint64_t* audio_page_offset, uint32_t* audio_segment,
                        uint32_t* audio_seq)
{
    const char* const who = "ohgpu_ogg_flac_head";
    if (!bytes || !info || !serial || !audio_page_offset || !audio_segment || !audio_seq) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    if (n >= 0x80000000ull) n = 0x7fffffffu;                          // (the head of a stream is asked for: what lies behind 2 GiB is not it)
    static const oggpage::Tables tables = [] { oggpage::Tables t; oggpage::make_tables(&t); return t; }();
    // the walk of csrc/ogg_page_core.h on the host, every page's checksum run as it comes
    oggpage::Stream s = {};
    s.src_bytes = (uint32_t)n;
    s.dst_capacity = n;
    s.flags = oggpage::kAnySeq | oggpage::kAnySerial | oggpage::kFlacMapping;
    s.packet_capacity = (uint32_t)std::min<size_t>(n, 65536);
    std::vector<oggpage::Packet> packets(s.packet_capacity);
    std::vector<oggpage::Piece> pieces(oggpage::piece_capacity(s));
    auto good = [&](uint32_t, const uint8_t* page, uint32_t page_bytes) { return oggpage::crc_run(tables.byte, page, 0, page_bytes) == oggpage::stored_crc(page); };
    oggpage::Result r;
    uint32_t n_pieces = 0;
    oggpage::walk(s, 0, (const uint8_t*)bytes, packets.data(), pieces.data(), good, &r, &n_pieces);
    if (r.packets == 0 || !(packets[0].flags & oggpage::kPacketMappingHeader) || packets[0].page_offset != 0)
        return set_error(OHGPU_ERR_INVALID, "%s: no Ogg FLAC mapping header in the first packet (walk status %u)", who, r.status);
    std::vector<uint8_t> run(r.bytes_delivered);
    for (uint32_t k = 0; k < n_pieces; k++) memcpy(run.data() + pieces[k].run_pos, (const uint8_t*)bytes + pieces[k].src_pos, pieces[k].bytes);
    uint64_t audio = 0;
    const int err = ohgpu_flac_streaminfo(run.data(), run.size(), info, &audio);
    if (err != OHGPU_OK) return err;
    *serial = r.serial;
    if (audio == r.bytes_delivered) {                                 // every delivered packet is metadata: the audio begins where the walk would go on
        if (r.status != OHGPU_OGG_OK) return set_error(OHGPU_ERR_INVALID, "%s: the pages stop (status %u) before the audio begins", who, r.status);
        *audio_page_offset = r.bytes_consumed; *audio_segment = r.resume_segment; *audio_seq = r.next_seq;
        return OHGPU_OK;
    }
    const uint32_t recorded = std::min(r.packets, s.packet_capacity);
    for (uint32_t k = 0; k < recorded; k++)
        if (packets[k].run_pos == audio && (packets[k].bytes || k + 1 == recorded || packets[k + 1].run_pos != audio)) {
            *audio_page_offset = packets[k].page_offset; *audio_segment = packets[k].segment; *audio_seq = packets[k].page_seq;
            return OHGPU_OK;
        }
    return set_error(OHGPU_ERR_UNSUPPORTED, "%s: the metadata ends at byte %llu of the packets' bytes, inside a packet", who, (unsigned long long)audio);
}

int ohgpu_ogg_flac_process_host(ohgpu_ctx* ctx, const ohgpu_ogg_stream_desc* ogg_descs, const ohgpu_flac_stream_desc* flac_descs, size_t n, size_t n_packets,
                                const void* src_host, uint64_t src_bytes, uint64_t mid_bytes, void* dst_host, uint64_t dst_bytes,
                                ohgpu_ogg_stream_result* ogg_results, ohgpu_ogg_packet* packets,
                                ohgpu_flac_stream_result* flac_results, ohgpu_flac_frame* frames, size_t frames_capacity, size_t* n_frames)
{
    const char* const who = "ohgpu_ogg_flac_process_host";
    if (n && (!ogg_descs || !flac_descs)) return set_error(OHGPU_ERR_INVALID, "%s: null argument", who);
    for (size_t i = 0; i < n; i++)
        if (flac_descs[i].src_offset != ogg_descs[i].dst_offset)
            return set_error(OHGPU_ERR_INVALID, "%s: stream %zu: the FLAC descriptor reads at %llu where the Ogg descriptor delivers at %llu", who, i,
                             (unsigned long long)flac_descs[i].src_offset, (unsigned long long)ogg_descs[i].dst_offset);
    if (n_frames) *n_frames = 0;
    std::vector<ohgpu_ogg_stream_result> ores(n);
    std::vector<ohgpu_flac_stream_result> fres(n);
    std::vector<ohgpu_flac_stream_desc> fdescs(flac_descs, flac_descs + n);
    void* d_mid = nullptr;
    const int err = decoder_process_host(ctx, who, src_host, src_bytes, dst_host, dst_bytes,
        [&](ohgpu_batch** b) { return ohgpu_ogg_batch_create(ctx, ogg_descs, n, n_packets, src_bytes, mid_bytes, b); },
        [&](const ohgpu_batch* b, const void* d_src, void* d_dst) {
            if (!n) return (int)OHGPU_OK;
            OHGPU_HIP_TRY_ALLOC(ctx_dev_alloc(ctx, &d_mid, mid_bytes ? mid_bytes : 1));      // the middle arena: the demuxed bytes never leave the device
            int e = ohgpu_ogg_batch_run(ctx, b, d_src, d_mid, nullptr);
            if (e == OHGPU_OK) e = ohgpu_ogg_batch_results(ctx, b, ores.data(), n);             // the one small read between the layers
            if (e == OHGPU_OK && packets) e = ohgpu_ogg_batch_packets(ctx, b, n_packets ? packets : nullptr, n_packets);
            if (e != OHGPU_OK) return e;
            for (size_t i = 0; i < n; i++) fdescs[i].src_bytes = ores[i].bytes_delivered;
            ohgpu_batch* fb = nullptr;
            e = ohgpu_flac_batch_create(ctx, fdescs.data(), n, mid_bytes, dst_bytes, &fb);
            if (e != OHGPU_OK) return e;
            const BatchPtr own(fb, BatchDeleter{ctx});
            e = ohgpu_flac_batch_run(ctx, fb, d_mid, d_dst, nullptr);
            if (e == OHGPU_OK) e = ohgpu_flac_batch_results(ctx, fb, fres.data(), n);
            if (e == OHGPU_OK && (frames || n_frames)) e = ohgpu_flac_batch_frames(ctx, fb, frames, frames ? frames_capacity : 0, n_frames);
            return e;
        },
        [&] {   // only what was decoded comes back, as in ohgpu_flac_process_host
            int e = OHGPU_OK;
            for (size_t i = 0; i < n && e == OHGPU_OK; i++) e = flac_download_decoded(ctx, who, fdescs[i], fres[i], dst_host);
            return e;
        });
    if (d_mid) { (void)hipStreamSynchronize(ctx->stream); ctx_dev_free(ctx, d_mid); }
    if (err == OHGPU_OK && ogg_results && n) memcpy(ogg_results, ores.data(), n * sizeof(ores[0]));
    if (err == OHGPU_OK && flac_results && n) memcpy(flac_results, fres.data(), n * sizeof(fres[0]));
    return err;
}

uint32_t ohgpu_ogg_crc(const void* bytes, size_t n)
{
    static const oggpage::Tables tables = [] { oggpage::Tables t; oggpage::make_tables(&t); return t; }();
    return bytes ? oggpage::crc_bytes(tables, (const uint8_t*)bytes, n) : 0u;
}

}  // extern "C"
