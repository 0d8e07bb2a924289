// api_raop.hip -- the C ABI's RAOP audio path (ohgpu_raop_*): the decrypt phase of csrc/raop_decrypt_kernel.hip in front
// of the Apple Lossless phases of csrc/alac_packet_kernel.hip.  A RAOP batch holds an AlacState like an Apple Lossless batch's, made
// of its decoding streams alone with their packets rewritten to the plaintext scratch, and a RaopState with the rest.
#include <cstring>

#include "api_common.h"

using namespace ohgpu;

namespace {

bool plaintext(const ohgpu_raop_stream_desc& d) { return d.alac.flags == OHGPU_RAOP_OUT_PLAINTEXT; }

int raop_check_desc(const ohgpu_raop_stream_desc& rd, size_t i, const ohgpu_alac_packet* packets, uint64_t next_packet, size_t n_packets,
                    uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    const ohgpu_alac_stream_desc& d = rd.alac;
    if (!plaintext(rd)) {
        const int err = alac_check_desc(d, i, packets, next_packet, n_packets, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
    } else {
        for (uint32_t r : d.reserved) if (r) return set_error(OHGPU_ERR_INVALID, "raop desc %zu: reserved words must be zero", i);
        if (d.first_packet != next_packet || d.n_packets > n_packets - next_packet)
            return set_error(OHGPU_ERR_INVALID, "raop desc %zu: packets [%u, +%u) where the table goes on at %llu of %zu", i, d.first_packet, d.n_packets, (unsigned long long)next_packet, n_packets);
        if (d.dst_offset % 4 != 0 || d.dst_plane_stride != 0) return set_error(OHGPU_ERR_INVALID, "raop desc %zu: plaintext output takes a dst_offset that is a multiple of 4 and no dst_plane_stride", i);
        uint64_t end = 0;
        for (uint32_t k = 0; k < d.n_packets; k++) {
            const ohgpu_alac_packet& p = packets[d.first_packet + k];
            if (p.reserved) return set_error(OHGPU_ERR_INVALID, "raop desc %zu: packet %u: reserved word must be zero", i, k);
            const int err = arena_span("raop desc", i, "reads", p.src_offset, p.bytes, src_arena_bytes, "source");
            if (err != OHGPU_OK) return err;
            if (k && p.src_offset < end) return set_error(OHGPU_ERR_INVALID, "raop desc %zu: packet %u at %llu where its predecessor ends at %llu (plaintext output: the packets ascend without overlap)", i, k, (unsigned long long)p.src_offset, (unsigned long long)end);
            end = p.src_offset + p.bytes;
        }
        if (d.n_packets) {
            const int err = arena_span("raop desc", i, "writes", d.dst_offset, end - packets[d.first_packet].src_offset, dst_arena_bytes, "destination");
            if (err != OHGPU_OK) return err;
        }
    }
    for (uint32_t k = 0; k < d.n_packets; k++)
        if (packets[d.first_packet + k].src_offset % 4 != 0)
            return set_error(OHGPU_ERR_INVALID, "raop desc %zu: packet %u: src_offset %llu is no multiple of 4", i, k, (unsigned long long)packets[d.first_packet + k].src_offset);
    return OHGPU_OK;
}

bool decimal(const char* p, const char* end, uint64_t* out)
{
    if (p == end || end - p > 10) return false;
    uint64_t v = 0;
    for (; p != end; p++) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (uint64_t)(*p - '0');
    }
    *out = v;
    return true;
}

}  // namespace

extern "C" {

int ohgpu_raop_fmtp_parse(const char* fmtp, size_t n, ohgpu_alac_config* config)
{
    if (!fmtp || !config) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_fmtp_parse: null argument");
    static const uint64_t kMost[12] = {0xffffffffull, 0xffffffffull, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xffff, 0xffffffffull, 0xffffffffull, 0xffffffffull};
    uint64_t f[12];
    const char* p = fmtp;
    const char* const end = fmtp + n;
    for (int k = 0; k < 12; k++) {
        while (p != end && *p == ' ') p++;
        const char* q = p;
        while (q != end && *q != ' ') q++;
        if (p == q) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_fmtp_parse: %d fields where the string has twelve", k);
        if (!decimal(p, q, &f[k])) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_fmtp_parse: field %d is no decimal number", k);
        if (f[k] > kMost[k]) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_fmtp_parse: field %d: %llu does not fit (the reference would truncate it)", k, (unsigned long long)f[k]);
        p = q;
    }
    if (f[2] != 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_fmtp_parse: compatible version %llu (0 only)", (unsigned long long)f[2]);
    memset(config, 0, sizeof(*config));
    config->frame_length = (uint32_t)f[1]; config->compatible_version = (uint8_t)f[2]; config->bit_depth = (uint8_t)f[3];
    config->pb = (uint8_t)f[4]; config->mb = (uint8_t)f[5]; config->kb = (uint8_t)f[6]; config->channels = (uint8_t)f[7];
    config->max_run = (uint16_t)f[8]; config->max_frame_bytes = (uint32_t)f[9]; config->avg_bit_rate = (uint32_t)f[10]; config->sample_rate = (uint32_t)f[11];
    return OHGPU_OK;
}

int ohgpu_raop_batch_check(const ohgpu_raop_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                           uint64_t src_arena_bytes, uint64_t dst_arena_bytes)
{
    if ((n && !descs) || (n_packets && !packets)) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_check: null argument");
    if (n > 0x00ffffffull || n_packets > 0x0fffffffull) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_check: too many descriptors");
    uint64_t next = 0;
    for (size_t i = 0; i < n; i++) {
        const int err = raop_check_desc(descs[i], i, packets, next, n_packets, src_arena_bytes, dst_arena_bytes);
        if (err != OHGPU_OK) return err;
        next += descs[i].alac.n_packets;
    }
    if (next != n_packets) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_check: the descriptors take %llu packets of a table of %zu", (unsigned long long)next, n_packets);
    return OHGPU_OK;
}

int ohgpu_raop_batch_create(ohgpu_ctx* ctx, const ohgpu_raop_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                            uint64_t src_arena_bytes, uint64_t dst_arena_bytes, ohgpu_batch** out)
{
    CTX_GUARD("ohgpu_raop_batch_create");
    BatchPtr b;
    int err = batch_begin(ctx, "ohgpu_raop_batch_create", kBatchRaop, true, n, UINT64_MAX, src_arena_bytes, dst_arena_bytes, out, &b);
    if (err == OHGPU_OK) err = ohgpu_raop_batch_check(descs, n, packets, n_packets, src_arena_bytes, dst_arena_bytes);
    if (err != OHGPU_OK) return err;
    b->alac = new (std::nothrow) AlacState();
    b->raop = new (std::nothrow) RaopState();
    if (!b->alac || !b->raop) return set_error(OHGPU_ERR_NOMEM, "ohgpu_raop_batch_create: out of host memory");
    AlacState& a = *b->alac;
    RaopState& r = *b->raop;
    a.plain = ctx->variant == 1;
    // the plan of the decrypt phase: a job per packet, in the table's order (the descriptors' ranges tile it)
    std::vector<raopcore::StreamIn> ins(n);
    r.keys.assign(n * raopcore::kKeyWords, 0u);
    r.plaintext.resize(n); r.first_packet.resize(n); r.n_packets.resize(n); r.alac_first.assign(n, 0u);
    for (size_t i = 0; i < n; i++) {
        const ohgpu_alac_stream_desc& d = descs[i].alac;
        ins[i] = raopcore::StreamIn{d.first_packet, d.n_packets, d.dst_offset, plaintext(descs[i]) ? 1u : 0u, 0u};
        r.plaintext[i] = plaintext(descs[i]); r.first_packet[i] = d.first_packet; r.n_packets[i] = d.n_packets;
        raopcore::expand_decrypt_key(descs[i].aes_key, &r.keys[i * raopcore::kKeyWords], raop_tables());
        raopcore::load_iv(descs[i].aes_iv, &r.keys[i * raopcore::kKeyWords + raopcore::kRoundKeyWords]);
    }
    static_assert(sizeof(raopcore::PacketIn) == sizeof(ohgpu_alac_packet), "the packet table is read as it is");
    std::vector<raopcore::Job> jobs;
    jobs.reserve(n_packets);
    r.plain_bytes = (size_t)raopcore::plan_jobs(ins.data(), n, (const raopcore::PacketIn*)packets, &jobs);
    // the Apple Lossless part: the decoding streams, their packets where the decrypt phase leaves them
    r.alac_packet.assign(n_packets, -1);
    for (size_t i = 0; i < n; i++) {
        if (r.plaintext[i]) continue;
        ohgpu_alac_stream_desc d = descs[i].alac;
        const uint32_t first = d.first_packet;
        d.first_packet = (uint32_t)a.packets.size();
        r.alac_first[i] = d.first_packet;
        a.streams.resize(a.streams.size() + 1);
        alac_add_stream(a, a.streams.size() - 1, d);
        for (uint32_t k = 0; k < d.n_packets; k++) {
            alaccore::Packet p;
            memset(&p, 0, sizeof(p));
            p.src_offset = jobs[first + k].dst_offset; p.bytes = packets[first + k].bytes; p.stream = (uint32_t)(a.streams.size() - 1); p.index = k;
            r.alac_packet[first + k] = (int64_t)a.packets.size();
            a.packets.push_back(p);
        }
    }
    for (size_t k = 0; k < n_packets; k++) b->src_bytes_touched += packets[k].bytes;
    err = alac_plan(ctx, b.get());
    if (err == OHGPU_OK) err = raop_plan(ctx, b.get(), jobs.data(), jobs.size());
    return batch_done(err, b, out);
}

int ohgpu_raop_batch_run(ohgpu_ctx* ctx, const ohgpu_batch* batch, const void* src_base, void* dst_base, void* stream)
{
    const int go = run_guard(ctx, "ohgpu_raop_batch_run", batch, kBatchRaop, batch && batch->kind == kBatchRaop && batch->raop->alac_packet.empty(), true, src_base, dst_base);
    if (go <= 0) return go;
    if ((uintptr_t)src_base % 4 != 0 || (uintptr_t)dst_base % 4 != 0) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_run: src_base and dst_base must be 4-byte aligned");
    hipStream_t s = pick_stream(ctx, stream);
    const int err = raop_run(ctx, batch, (const uint8_t*)src_base, (uint8_t*)dst_base, s);
    if (err != OHGPU_OK) return err;
    return alac_run(ctx, batch, (const uint8_t*)batch->raop->d_plain, (uint8_t*)dst_base, s);
}

int ohgpu_raop_batch_results(ohgpu_ctx* ctx, const ohgpu_batch* batch, ohgpu_alac_stream_result* streams, size_t n,
                             ohgpu_alac_packet_result* packets, size_t n_packets)
{
    CTX_GUARD("ohgpu_raop_batch_results");
    if (!batch || batch->kind != kBatchRaop) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_results: not a RAOP batch");
    const AlacState& a = *batch->alac;
    const RaopState& r = *batch->raop;
    if ((streams || n) && (n != batch->n || !streams)) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_results: room for %zu results, the batch has %zu streams", n, batch->n);
    if ((packets || n_packets) && (n_packets != r.alac_packet.size() || !packets))
        return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_results: room for %zu packet results, the batch has %zu packets", n_packets, r.alac_packet.size());
    if (r.alac_packet.empty()) {
        for (size_t i = 0; streams && i < batch->n; i++) streams[i] = ohgpu_alac_stream_result{0, 0, 0};
        return OHGPU_OK;
    }
    if (!a.ran) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_results: the batch has not run");
    OHGPU_HIP_TRY(hipEventSynchronize(a.end_event()));
    std::vector<ohgpu_alac_packet_result> decoded(a.packets.size()), all(r.alac_packet.size());
    const int err = alac_results(ctx, batch, decoded.data());
    if (err != OHGPU_OK) return err;
    for (size_t k = 0; k < all.size(); k++) all[k] = r.alac_packet[k] < 0 ? ohgpu_alac_packet_result{OHGPU_ALAC_OK, 0} : decoded[(size_t)r.alac_packet[k]];
    if (packets) memcpy(packets, all.data(), all.size() * sizeof(all[0]));
    for (size_t i = 0; streams && i < batch->n; i++) alac_summarise(all.data() + r.first_packet[i], r.n_packets[i], &streams[i]);
    return OHGPU_OK;
}

int ohgpu_raop_batch_phase_ms(ohgpu_ctx* ctx, const ohgpu_batch* batch, float ms[4])
{
    CTX_GUARD("ohgpu_raop_batch_phase_ms");
    if (!batch || batch->kind != kBatchRaop || !ms) return set_error(OHGPU_ERR_INVALID, "ohgpu_raop_batch_phase_ms: bad argument");
    const AlacState& a = *batch->alac;
    const hipEvent_t ev[5] = {batch->raop->ev[0], a.ev[0], a.ev[1], a.ev[2], a.ev[3]};
    return phase_ms("ohgpu_raop_batch_phase_ms", a.ran, ev, 4, ms);
}

int ohgpu_raop_process_host(ohgpu_ctx* ctx, const ohgpu_raop_stream_desc* descs, size_t n, const ohgpu_alac_packet* packets, size_t n_packets,
                            const void* src_host, uint64_t src_bytes, void* dst_host, uint64_t dst_bytes,
                            ohgpu_alac_stream_result* stream_results, ohgpu_alac_packet_result* packet_results)
{
    const char* const who = "ohgpu_raop_process_host";
    return alac_process_host(ctx, who, n, n_packets, src_host, src_bytes, dst_host, dst_bytes, stream_results, packet_results,
        [&](ohgpu_batch** b) { return ohgpu_raop_batch_create(ctx, descs, n, packets, n_packets, src_bytes, dst_bytes, b); }, ohgpu_raop_batch_run, ohgpu_raop_batch_results,
        [&](size_t i, const ohgpu_alac_packet_result* pres) {
            const ohgpu_alac_stream_desc& d = descs[i].alac;
            if (!plaintext(descs[i])) return alac_download_decoded(ctx, who, d, pres + d.first_packet, dst_host);
            // a plaintext stream: its packets, runs of touching ones in one copy
            for (uint32_t k = 0; k < d.n_packets;) {
                const uint64_t from = packets[d.first_packet + k].src_offset;
                uint64_t to = from + packets[d.first_packet + k].bytes;
                for (k++; k < d.n_packets && packets[d.first_packet + k].src_offset == to; k++) to += packets[d.first_packet + k].bytes;
                if (to == from) continue;
                // (as one "plane" of one-byte samples: the run's bytes from its offset in the stream's window)
                const int err = download_planes(ctx, who, dst_host, d.dst_offset, 0, 1, 1, from - packets[d.first_packet].src_offset, to - from);
                if (err != OHGPU_OK) return err;
            }
            return (int)OHGPU_OK;
        });
}

}  // extern "C"
