// api_alac.hip -- the C ABI's Apple Lossless packet decoder (ohgpu_alac_*).
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace ohgpu {

int alac_check_desc(const ohgpu_alac_stream_desc& d, size_t i, const ohgpu_alac_packet* packets, uint64_t next_packet, size_t n_packets,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    const ohgpu_alac_config& c = d.config;
    if (c.channels < 1 || c.channels > OHGPU_MAX_CHANNELS) return set_error(OHGPU_ERR_INVALID, "alac desc %zu: channels %u outside 1..8", i, c.channels);
    if (c.frame_length < 1 || c.frame_length > OHGPU_ALAC_MAX_FRAME_LENGTH) return set_error(OHGPU_ERR_INVALID, "alac desc %zu: frame length %u outside 1..16384", i, c.frame_length);
    if (c.compatible_version != 0) return set_error(OHGPU_ERR_INVALID, "alac desc %zu: compatible version %u", i, c.compatible_version);
    if (c.bit_depth != 16 && c.bit_depth != 20 && c.bit_depth != 24 && c.bit_depth != 32)
        return set_error(OHGPU_ERR_UNSUPPORTED, "alac desc %zu: bit depth %u (16/24/32; 20 is accepted and every packet of it UNSUPPORTED)", i, c.bit_depth);
    if (d.flags != 0 && d.flags != OHGPU_ALAC_OUT_PACKED_LE && d.flags != OHGPU_ALAC_OUT_PACKED_BE) return set_error(OHGPU_ERR_INVALID, "alac desc %zu: unknown flags 0x%x", i, d.flags);
    for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "alac desc %zu: reserved words must be zero", i);
    if (d.first_packet != next_packet || d.n_packets > n_packets - next_packet)
        return set_error(OHGPU_ERR_INVALID, "alac desc %zu: packets [%u, +%u) where the table goes on at %llu of %zu", i, d.first_packet, d.n_packets, (unsigned long long)next_packet, n_packets);
    const uint64_t most = (uint64_t)c.frame_length * c.channels * 5u + 64u;
    for (uint32_t k = 0; k < d.n_packets; k++) {
        const ohgpu_alac_packet& p = packets[d.first_packet + k];
        if (p.reserved) return set_error(OHGPU_ERR_INVALID, "alac desc %zu: packet %u: reserved word must be zero", i, k);
        if (p.bytes > most) return set_error(OHGPU_ERR_INVALID, "alac desc %zu: packet %u of %u bytes (at most frame length x channels x 5 + 64 = %llu)", i, k, p.bytes, (unsigned long long)most);
        const int err = arena_span("alac desc", i, "reads", p.src_offset, p.bytes, src_arena_bytes, "source");
        if (err != OHGPU_OK) return err;
    }
    return decoded_dst_check("alac desc", i, c.channels, (uint64_t)d.n_packets * c.frame_length, d.flags ? (uint64_t)c.channels * (c.bit_depth / 8u) : 0u,
                             d.dst_offset, d.dst_plane_stride, dst_arena_bytes);
}

void alac_add_stream(AlacState& a, size_t i, const ohgpu_alac_stream_desc& d)
{
    alaccore::Stream& s = a.streams[i];
    memset(&s, 0, sizeof(s));
    s.dst_offset = d.dst_offset; s.dst_plane_stride = d.dst_plane_stride; s.first_packet = d.first_packet; s.n_packets = d.n_packets;
    s.frame_length = d.config.frame_length; s.sample_rate = d.config.sample_rate; s.max_run = d.config.max_run;
    s.bit_depth = d.config.bit_depth; s.pb = d.config.pb; s.mb = d.config.mb; s.kb = d.config.kb; s.channels = d.config.channels;
    s.flags = (uint8_t)d.flags;
}

int alac_download_decoded(ohgpu_ctx* ctx, const char* who, const ohgpu_alac_stream_desc& d, const ohgpu_alac_packet_result* pres, void* dst_host)
{
    const uint32_t fl = d.config.frame_length;
    const uint64_t unit = d.flags ? (uint64_t)d.config.channels * (d.config.bit_depth / 8u) : 4u;
    for (uint32_t k = 0; k < d.n_packets;) {
        if (pres[k].status != OHGPU_ALAC_OK) { k++; continue; }
        const uint32_t k0 = k;
        uint64_t samples = 0;
        for (;;) {
            const uint32_t got = pres[k].samples;
            samples = (uint64_t)(k - k0) * fl + got;
            k++;
            if (got != fl || k == d.n_packets || pres[k].status != OHGPU_ALAC_OK) break;
        }
        if (samples == 0) continue;
        const int err = download_planes(ctx, who, dst_host, d.dst_offset, d.dst_plane_stride, d.flags ? 1u : d.config.channels, unit, (uint64_t)k0 * fl, samples);
        if (err != OHGPU_OK) return err;
    }
    return OHGPU_OK;
}

void alac_summarise(const ohgpu_alac_packet_result* pres, uint32_t n_packets, ohgpu_alac_stream_result* out)
{
    ohgpu_alac_stream_result r = {0, 0, 0};
    while (r.packets_ok < n_packets && pres[r.packets_ok].status == OHGPU_ALAC_OK) r.samples += pres[r.packets_ok++].samples;
    if (r.packets_ok < n_packets) r.first_bad_status = pres[r.packets_ok].status;
    *out = r;
}

}  // namespace ohgpu

extern "C" {

int ohgpu_alac_config_parse(const void* bytes, size_t n, ohgpu_alac_config* config)
{
    const uint8_t* p = (const uint8_t*)bytes;
    if (!p || !config) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_config_parse: null argument");
    // older files wrap the configuration: a 'frma' atom, then an 'alac' atom's header, 12 bytes each
    for (const char* name : {"frma", "alac"})
        if (n >= 12 && memcmp(p + 4, name, 4) == 0) { p += 12; n -= 12; }
    if (n < 24) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_config_parse: %zu bytes where the configuration takes 24", n);
    const auto be32 = [](const uint8_t* q) { return ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3]; };
    if (p[4] != 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_config_parse: compatible version %u (0 only)", p[4]);
    memset(config, 0, sizeof(*config));
    config->frame_length = be32(p);
    config->compatible_version = p[4]; config->bit_depth = p[5]; config->pb = p[6]; config->mb = p[7]; config->kb = p[8]; config->channels = p[9];
    config->max_run = (uint16_t)(((uint32_t)p[10] << 8) | p[11]);
    config->max_frame_bytes = be32(p + 12); config->avg_bit_rate = be32(p + 16); config->sample_rate = be32(p + 20);
    return OHGPU_OK;
}

int ohgpu_alac_batch_check(const ohgpu_alac_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if ((n && !descs) || (n_packets && !packets)) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_batch_check: null argument");
    if (n > 0x00ffffffull || n_packets > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_batch_check: too many descriptors");
    uint64_t next = 0;
    for (size_t i = 0; i < n; i++) {
        const int err = alac_check_desc(descs[i], i, packets, next, n_packets, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        next += descs[i].n_packets;
    }
    if (next != n_packets) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_batch_check: the descriptors take %llu packets of a table of %zu", (unsigned long long)next, n_packets);
    return OHGPU_OK;
}

int ohgpu_alac_batch_create(ohgpu_ctx* ctx, const ohgpu_alac_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                            uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_alac_batch_create");
    BatchPtr b;     // (the descriptors' and the table's pointers and counts are ohgpu_alac_batch_check's to refuse)
    int err = batch_begin(ctx, "ohgpu_alac_batch_create", kBatchAlac, true, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_alac_batch_check(descs, n, packets, n_packets, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->alac = new (std::nothrow) AlacState();
    if (!b->alac) return set_error(OHGPU_ERR_NOMEM, "ohgpu_alac_batch_create: out of host memory");
    AlacState& a = *b->alac;
    a.plain = ctx->variant == 1;
    a.streams.resize(n);
    a.packets.resize(n_packets);
    for (size_t i = 0; i < n; i++) {
        const ohgpu_alac_stream_desc& d = descs[i];
        alac_add_stream(a, i, d);
        for (uint32_t k = 0; k < d.n_packets; k++) {
            alaccore::Packet& p = a.packets[d.first_packet + k];
            memset(&p, 0, sizeof(p));
            p.src_offset = packets[d.first_packet + k].src_offset; p.bytes = packets[d.first_packet + k].bytes; p.stream = (uint32_t)i; p.index = k;
            b->src_bytes_touched += p.bytes;
        }
    }
    err = alac_plan(ctx, b.get());
    return batch_done(err, b, out);
}

int ohgpu_alac_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_alac_batch_run", batch, kBatchAlac, batch && batch->kind == kBatchAlac && batch->alac->packets.empty(), true, src_base, dst_base);
    if (go <= 0) return go;
    return alac_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, pick_stream(ctx, stream));
}

int ohgpu_alac_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_stream_result* streams, size_t n,
                             ohgpu_alac_packet_result* packets, size_t n_packets)
{
    CTX_GUARD("ohgpu_alac_batch_results");
    if (!batch || batch->kind != kBatchAlac) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_batch_results: not an Apple Lossless batch");
    const AlacState& a = *batch->alac;
    if ((streams || n) && (n != batch->n || !streams)) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_batch_results: room for %zu results, the batch has %zu streams", n, batch->n);
    if ((packets || n_packets) && (n_packets != a.packets.size() || !packets))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_batch_results: room for %zu packet results, the batch has %zu packets", n_packets, a.packets.size());
    std::vector<ohgpu_alac_packet_result> all(a.packets.size());
    const int err = alac_results(ctx, batch, all.data());
    if (err != OHGPU_OK) return err;
    if (packets && !all.empty()) memcpy(packets, all.data(), all.size() * sizeof(all[0]));
    for (size_t i = 0; streams && i < batch->n; i++) {
        const alaccore::Stream& s = a.streams[i];
        alac_summarise(all.data() + s.first_packet, s.n_packets, &streams[i]);
    }
    return OHGPU_OK;
}

int ohgpu_alac_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[3])
{
    CTX_GUARD("ohgpu_alac_batch_phase_ms");
    if (!batch || batch->kind != kBatchAlac || !ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_alac_batch_phase_ms: bad argument");
    return phase_ms("ohgpu_alac_batch_phase_ms", batch->alac->ran, batch->alac->ev, 3, ms);
}

int ohgpu_alac_process_host(ohgpu_ctx* ctx, const ohgpu_alac_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                            const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                            ohgpu_alac_stream_result* stream_results, ohgpu_alac_packet_result* packet_results)
{
    const char* const who = "ohgpu_alac_process_host";
    return alac_process_host(ctx, who, n, n_packets, src_host, src_bytes, dst_host, dst_bytes, stream_results, packet_results,
        [&](ohgpu_batch** b) { return ohgpu_alac_batch_create(ctx, descs, n, packets, n_packets, src_bytes, dst_bytes, b); }, ohgpu_alac_batch_run, ohgpu_alac_batch_results,
        // per stream, each run of packets that decoded (whole ones, then perhaps a short one) in one copy per plane
        [&](size_t i, const ohgpu_alac_packet_result* pres) { return alac_download_decoded(ctx, who, descs[i], pres + descs[i].first_packet, dst_host); });
}

}  // extern "C"
