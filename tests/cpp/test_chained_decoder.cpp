// test_chained_decoder.cpp -- a chained Ogg stream through the host element (ohpipeline_amd/host/VorbisDecoder.h, OggVorbisBatchDecoder
// across links; DESIGN.md 5.23's addendum).
// `test_chained_decoder cpu <chain.ogg> <truth> <step> [<first>]` needs no device: the file is pushed <step> bytes at a time (the first
// push <first> bytes, where given) and, between
// CollectLinks and ApplyLinks, a stand-in answers what the links call answers for the bytes at hand, from the truth file the models
// write: per link where it begins and what its head says, per packet where it begins, at which byte of the file it is whole, its granule
// position and flags and what the model says it delivers.  The stand-in's rules are the call's: the packets that are whole; a link none
// of whose packets is whole is not there yet; fewer than three of them is OHGPU_VORBIS_LINK_HEAD_OPEN; the first audio packet of a link's
// range primes.  Printed, for tests/test_chained_host_cpp.py to hold against the models: the events in the order the sink and the
// comment observer got them -- S<channels>:<rate> a decoded-stream message, M<bytes> a comment packet, A<samples> audio (runs joined) --
// and how many HEAD_OPEN rows were served.  Checked here: pieces of whole samples within DecodedAudio::kMaxBytes, track offsets that run on.
// `test_chained_decoder gpu <chain.ogg> <plain.ogg> <step> <out chain> <out plain>`: the two files as two lanes of the same Tick(), the
// device doing the work; the events of both, and the bytes that reached a processor written to the two output files.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/Msg.h"
#include "../../ohpipeline_amd/host/VorbisDecoder.h"

using namespace OpenHome;
using namespace OpenHome::Media;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)

static std::vector<TByte> ReadFile(const std::string& aPath)
{
    std::ifstream in(aPath, std::ios::binary);
    return std::vector<TByte>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

// The sink and the observer write one log: what came, in the order it came.
class Log : public IPipelineElementDownstream, public IVorbisCommentObserver {
public:
    void Push(Msg* aMsg) override
    {
        if (KindOf(aMsg) == MsgKind::AudioPcm) {                      // counted as it comes, its bytes read at the tick's end
            MsgAudioPcm* m = static_cast<MsgAudioPcm*>(aMsg);
            TEST(m->NumChannels() == iChannels && m->Jiffies() % (Jiffies::kPerSecond / m->SampleRate()) == 0);
            iRun += m->Jiffies() / (Jiffies::kPerSecond / m->SampleRate());
            iAudio.push_back(m);
            return;
        }
        if (KindOf(aMsg) == MsgKind::DecodedStream) {
            Flush();
            const DecodedStreamInfo& info = static_cast<MsgDecodedStream*>(aMsg)->StreamInfo();
            iChannels = info.iNumChannels;
            iText += "S" + std::to_string(info.iNumChannels) + ":" + std::to_string(info.iSampleRate) + " ";
        }
        aMsg->RemoveRef();
    }
    void NotifyVorbisComment(const Brx& aPacket) override
    {
        Flush();
        TEST(aPacket.Bytes() >= 7 && aPacket.Ptr()[0] == 3 && memcmp(aPacket.Ptr() + 1, "vorbis", 6) == 0);
        iText += "M" + std::to_string(aPacket.Bytes()) + " ";
    }
    // the audio messages so far: their sizes into the log, their bytes to aBatch's processors (or nowhere)
    void Drain(PlayableBatch* aBatch, std::vector<TByte>* aGot)
    {
        std::vector<std::unique_ptr<ProcessorPcmBufTest>> procs;
        while (!iAudio.empty()) {
            MsgAudioPcm* m = iAudio.front();
            iAudio.pop_front();
            TEST(m->TrackOffset() == iJiffies);
            iJiffies += m->Jiffies();
            MsgPlayable* p = m->CreatePlayable();
            TEST(p->Bytes() > 0 && p->Bytes() <= DecodedAudio::kMaxBytes && p->Bytes() % 2u == 0);
            if (aBatch) { procs.emplace_back(new ProcessorPcmBufTest()); aBatch->Add(p, *procs.back()); }
            else p->RemoveRef();
        }
        if (aBatch && !procs.empty()) {
            aBatch->Run();
            for (auto& pr : procs) { const Brn b = pr->Buf(); aGot->insert(aGot->end(), b.Ptr(), b.Ptr() + b.Bytes()); }
        }
    }
    void Flush() { if (iRun) iText += "A" + std::to_string(iRun) + " "; iRun = 0; }
    std::deque<MsgAudioPcm*> iAudio;
    std::string iText;
    TUint iChannels = 0;
    TUint64 iRun = 0, iJiffies = 0;
};

struct Truth {
    struct Link { uint64_t page_offset; uint32_t serial, channels, rate, bs0, bs1; };
    struct Packet { uint32_t link; uint64_t page_offset; uint32_t segment, seq; uint64_t whole_at; int64_t granule; uint32_t flags, samples, audio; };
    std::vector<Link> links;
    std::vector<Packet> packets;
};

static Truth ReadTruth(const std::string& aPath)
{
    Truth t;
    std::ifstream in(aPath);
    size_t np = 0, nl = 0;
    in >> np >> nl;
    t.links.resize(nl);
    t.packets.resize(np);
    for (auto& l : t.links) in >> l.page_offset >> l.serial >> l.channels >> l.rate >> l.bs0 >> l.bs1;
    for (auto& p : t.packets) in >> p.link >> p.page_offset >> p.segment >> p.seq >> p.whole_at >> p.granule >> p.flags >> p.samples >> p.audio;
    return t;
}

struct Answer {
    ohgpu_ogg_stream_result demuxed;
    std::vector<ohgpu_ogg_packet> records;
    std::vector<ohgpu_vorbis_packet_result> decoded;
    std::vector<ohgpu_vorbis_link> links;
};

// What the links call answers for what the decoder has at hand.
static void StandIn(const OggVorbisBatchDecoder& d, const Truth& t, size_t aFileBytes, const ohgpu_ogg_stream_desc& aOgg, const ohgpu_vorbis_stream_desc& aVorbis, Answer& a, TUint& aOpen)
{
    memset(&a.demuxed, 0, sizeof(a.demuxed));
    a.records.clear(); a.decoded.clear(); a.links.clear();
    const uint64_t from = d.ConsumedBytes(), have = from + d.PendingBytes();
    size_t k0 = 0;
    while (k0 < t.packets.size() && !(t.packets[k0].page_offset == from && t.packets[k0].segment == aOgg.first_page_segment)) k0++;
    TEST(k0 < t.packets.size() && t.packets[k0].seq == aOgg.expect_seq && t.links[t.packets[k0].link].serial == aOgg.serial);
    if (k0 >= t.packets.size()) return;
    size_t k1 = k0;
    while (k1 < t.packets.size() && t.packets[k1].whole_at <= have && k1 - k0 < aOgg.packet_capacity) k1++;
    uint64_t cursor = aVorbis.dst_offset;
    for (size_t k = k0; k < k1; ) {
        const uint32_t link = t.packets[k].link;
        size_t e = k;
        while (e < k1 && t.packets[e].link == link) e++;
        const Truth::Link& l = t.links[link];
        ohgpu_vorbis_link row;
        memset(&row, 0, sizeof(row));
        row.serial = l.serial; row.first_packet = aOgg.packet_first + (uint32_t)(k - k0); row.n_packets = (uint32_t)(e - k);
        row.page_offset = k == k0 ? OHGPU_VORBIS_LINK_CONTINUED : l.page_offset - from;
        row.channels = l.channels; row.sample_rate = l.rate; row.blocksize_short = l.bs0; row.blocksize_long = l.bs1;
        row.head = (k != k0 && e - k < 3 && e == k1) ? OHGPU_VORBIS_LINK_HEAD_OPEN : OHGPU_OK;
        if (row.head != OHGPU_OK) aOpen++;
        row.dst_offset = cursor;
        bool primed = false;
        for (size_t p = k; p < e; p++) {
            const Truth::Packet& tp = t.packets[p];
            ohgpu_ogg_packet r;
            memset(&r, 0, sizeof(r));
            r.page_offset = tp.page_offset - from; r.segment = tp.segment; r.page_seq = tp.seq; r.granule = tp.granule;
            r.flags = tp.flags | ((p == k && k != k0) ? (OHGPU_OGG_PACKET_LINK | OHGPU_OGG_PACKET_BOS) : 0u);
            a.records.push_back(r);
            ohgpu_vorbis_packet_result pr;
            memset(&pr, 0, sizeof(pr));
            if (row.head == OHGPU_OK) {
                pr.status = tp.audio ? OHGPU_VORBIS_OK : OHGPU_VORBIS_HEADER;
                if (tp.audio) { pr.samples = primed ? tp.samples : 0; primed = true; }
            }
            row.samples += pr.samples;
            a.decoded.push_back(pr);
        }
        if (row.head == OHGPU_OK) cursor += ((uint64_t)row.n_packets * (l.bs1 / 2u) * l.channels * 2u + 3u) & ~(uint64_t)3u;
        a.links.push_back(row);
        k = e;
    }
    if (a.links.empty() || a.links[0].page_offset != OHGPU_VORBIS_LINK_CONTINUED) {   // (every stream has its continued link)
        ohgpu_vorbis_link row;
        memset(&row, 0, sizeof(row));
        row.page_offset = OHGPU_VORBIS_LINK_CONTINUED; row.serial = aOgg.serial; row.dst_offset = aVorbis.dst_offset;
        a.links.insert(a.links.begin(), row);
    }
    a.demuxed.packets = (uint32_t)(k1 - k0);
    a.demuxed.serial = t.links[t.packets[k1 - 1].link].serial;
    // what the page layer read: up to the next packet's page, or, behind a link's last packet, up to the next link's first page
    uint64_t consumed = have;
    if (k1 < t.packets.size()) consumed = std::min<uint64_t>(have, t.packets[k1].page_offset);
    else consumed = std::min<uint64_t>(have, aFileBytes);
    a.demuxed.bytes_consumed = consumed - from;
}

static void TestWithAStandIn(MsgFactory& f, const std::vector<TByte>& aOgg, const Truth& t, size_t aStep, size_t aFirst)
{
    OggVorbisBatchDecoder d;
    Log log;
    d.SetCommentObserver(&log);
    CodecController controller(f, log, Jiffies::kPerSecond);
    TUint64 trackOffset = 0;
    TUint open = 0, ticks = 0;
    std::vector<TByte> arena;
    for (size_t at = 0, n = 0; at < aOgg.size(); at += n) {
        n = std::min(at == 0 && aFirst ? aFirst : aStep, aOgg.size() - at);
        d.Push(Brn(aOgg.data() + at, (TUint)n));
        ohgpu_ogg_stream_desc og;
        ohgpu_vorbis_stream_desc vo;
        TUint64 region = 0;
        if (!d.CollectLinks(0, 0, 0, 0, 0, og, vo, region)) continue;
        TEST(og.src_bytes == d.PendingBytes() && og.serial == d.Serial() && vo.image_bytes == d.Image().size() && region >= OggVorbisBatchDecoder::kMinRegionBytes);
        Answer a;
        StandIn(d, t, aOgg.size(), og, vo, a, open);
        if (a.records.empty()) continue;
        arena.assign((size_t)region, 0);
        TEST(d.ApplyLinks(og, vo, region, a.demuxed, a.records.data(), a.decoded.data(), a.links.data(), a.links.size(), arena.data(), controller, trackOffset));
        log.Drain(nullptr, nullptr);
        ticks++;
    }
    log.Flush();
    TEST(d.Finished() && d.PendingBytes() == 0 && !d.Corrupt() && trackOffset == log.iJiffies);
    TEST(d.Serial() == t.links.back().serial && d.Info().channels == t.links.back().channels);
    printf("events: %s\nopen: %u ticks: %u samples: %llu\n", log.iText.c_str(), open, ticks, (unsigned long long)d.SamplesOutput());
}

static void TestTwoLanesThroughTheDevice(MsgFactory& f, const std::vector<TByte>& aChain, const std::vector<TByte>& aPlain, size_t aStep, const char* aOutChain, const char* aOutPlain)
{
    OggVorbisBatchDecoder d[2];
    Log log[2];
    CodecController c0(f, log[0], Jiffies::kPerSecond), c1(f, log[1], Jiffies::kPerSecond);
    OggVorbisBatchDecoder::Lane lanes[2] = {{&d[0], &c0, 0}, {&d[1], &c1, 0}};
    const std::vector<TByte>* files[2] = {&aChain, &aPlain};
    PlayableBatch batch(f);
    std::vector<TByte> got[2];
    for (size_t at = 0; at < std::max(aChain.size(), aPlain.size()); at += aStep) {
        for (int i = 0; i < 2; i++) {
            d[i].SetCommentObserver(&log[i]);
            if (at < files[i]->size()) d[i].Push(Brn(files[i]->data() + at, (TUint)std::min(aStep, files[i]->size() - at)));
        }
        uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
        const bool anything = (d[0].PendingBytes() != 0 && !d[0].Finished()) || (d[1].PendingBytes() != 0 && !d[1].Finished());
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        OggVorbisBatchDecoder::Tick(f, lanes, 2);
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + (anything ? 1 : 0));                                 // one fused call a tick, both lanes in it
        for (int i = 0; i < 2; i++) log[i].Drain(&batch, &got[i]);
    }
    const char* outs[2] = {aOutChain, aOutPlain};
    for (int i = 0; i < 2; i++) {
        log[i].Flush();
        TEST(d[i].Finished() && !d[i].Corrupt() && lanes[i].trackOffset == log[i].iJiffies);
        std::ofstream(outs[i], std::ios::binary).write((const char*)got[i].data(), (std::streamsize)got[i].size());
        printf("lane %d events: %s\n", i, log[i].iText.c_str());
    }
}

int main(int argc, char** argv)
{
    if (argc < 5) { printf("usage: test_chained_decoder cpu chain.ogg truth step | gpu chain.ogg plain.ogg step out_chain out_plain\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    if (gpu && argc < 7) return 2;
    {
        MsgFactory f(gpu ? 0 : -1);
        if (gpu) TestTwoLanesThroughTheDevice(f, ReadFile(argv[2]), ReadFile(argv[3]), (size_t)atoi(argv[4]), argv[5], argv[6]);
        else TestWithAStandIn(f, ReadFile(argv[2]), ReadTruth(argv[3]), (size_t)atoi(argv[4]), argc > 5 ? (size_t)atoi(argv[5]) : 0);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
