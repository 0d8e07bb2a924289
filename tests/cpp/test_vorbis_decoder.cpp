// test_vorbis_decoder.cpp -- Ogg Vorbis in the host adapter (ohpipeline_amd/host/VorbisDecoder.h: VorbisRecognise, OggVorbisBatchDecoder;
// DESIGN.md 5.23).
// `test_vorbis_decoder cpu <stream.ogg> <truth> <pcm>` runs what needs no device: the recognition rule, the head arriving over ragged
// pushes, the refusals, and the element's whole tick with the device stood in for between Collect and Apply -- the truth file lists, per
// audio packet, where it begins (page offset, segment, page number), at which byte of the file it is complete, and what the model says
// it delivers; <pcm> is the model's samples, interleaved big-endian.  What the stand-in answers is what the fused call answers for the
// bytes at hand: the packets that are whole, the first of them priming.  Checked: the bytes that reach the sink are the model's, up to
// the last page's granule position (given one short of the decoded length: the trim), in pieces of whole samples within
// DecodedAudio::kMaxBytes, one decoded-stream message in front, every packet delivering once (a tick's last packet is the next tick's first,
// which primes).
// `test_vorbis_decoder gpu ...` adds the same lane through Tick(), the device doing the work: every sample within 1 LSB of the model's.
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
#define TEST_THROWS(expr, Exc) do { bool thrown_ = false; try { expr; } catch (Exc&) { thrown_ = true; } gChecks++; \
    if (!thrown_) { gFailures++; printf("FAILED %s:%d  %s did not throw\n", __FILE__, __LINE__, #expr); } } while (0)

static std::vector<TByte> ReadFile(const std::string& aPath)
{
    std::ifstream in(aPath, std::ios::binary);
    return std::vector<TByte>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

class Sink : public IPipelineElementDownstream {
public:
    void Push(Msg* aMsg) override
    {
        if (KindOf(aMsg) == MsgKind::AudioPcm) { iAudio.push_back(static_cast<MsgAudioPcm*>(aMsg)); return; }
        if (KindOf(aMsg) == MsgKind::DecodedStream) { iStreams++; iStreamBeforeAudio = iStreamBeforeAudio && iAudio.empty() && iAudioSeen == 0; }
        aMsg->RemoveRef();
    }
    std::deque<MsgAudioPcm*> iAudio;
    TUint iStreams = 0, iAudioSeen = 0;
    TBool iStreamBeforeAudio = true;
};

struct Truth {
    struct Packet { uint64_t page_offset; uint32_t segment, seq; uint64_t whole_at; uint32_t samples; uint64_t position; };
    uint32_t channels = 0;
    int64_t granule = 0;                // the last page's
    uint64_t audio_page = 0;
    std::vector<Packet> packets;
};

static Truth ReadTruth(const std::string& aPath)
{
    Truth t;
    std::ifstream in(aPath);
    size_t n = 0;
    in >> n >> t.channels >> t.granule >> t.audio_page;
    t.packets.resize(n);
    for (auto& p : t.packets) in >> p.page_offset >> p.segment >> p.seq >> p.whole_at >> p.samples >> p.position;
    return t;
}

static void TestRecogniseAndHead(const std::vector<TByte>& aOgg, const Truth& aTruth)
{
    TEST(VorbisRecognise(Brn(aOgg.data(), 64)));
    TEST(!VorbisRecognise(Brn(aOgg.data(), 27)) && !VorbisRecognise(Brn(aOgg.data(), 0)));
    std::vector<TByte> other(aOgg.begin(), aOgg.begin() + 64);
    other[27 + other[26] + 1] = 'f';                                                  // an Ogg stream of another codec
    TEST(!VorbisRecognise(Brn(other.data(), 64)));
    const TByte riff[64] = {'R', 'I', 'F', 'F'};
    TEST(!VorbisRecognise(Brn(riff, 64)));
    // the head over ragged pushes: known exactly when its last byte is in, and the queue starts at the first audio page from then on
    OggVorbisBatchDecoder d;
    const TUint steps[] = {3, 1, 2, 5, 7, 11, 13, 1, 1, 40, 17, 60, 300, 1000, 5000, 20000, 100000};
    size_t at = 0;
    for (TUint n : steps) {
        if (at >= aOgg.size()) break;
        n = (TUint)std::min<size_t>(n, aOgg.size() - at);
        TEST(d.HeadKnown() == (at >= aTruth.audio_page));
        TEST(d.PendingBytes() == (at >= aTruth.audio_page ? at - aTruth.audio_page : 0));
        d.Push(Brn(aOgg.data() + at, n));
        at += n;
    }
    TEST(d.HeadKnown() && d.ConsumedBytes() == aTruth.audio_page && d.Info().channels == aTruth.channels && d.SamplesOutput() == 0 && !d.Corrupt());
    TEST(d.ResumeSegment() == 0 && d.NextPageNumber() == aTruth.packets[0].seq && d.Serial() == 0x5642);
    TEST_THROWS(OggVorbisBatchDecoder().Info(), AssertionFailed);
    { OggVorbisBatchDecoder x; TEST_THROWS(x.Push(Brn(riff, 1)), CodecStreamCorrupt); TEST(x.Corrupt()); }
    { OggVorbisBatchDecoder x; TEST_THROWS(x.Push(Brn(other.data(), 64)), CodecStreamCorrupt); }
}

// The device's answer for what a decoder has at hand, from the truth.  Returns how many packets it recorded.
static size_t StandIn(const OggVorbisBatchDecoder& d, const Truth& t, const ohgpu_ogg_stream_desc& aOgg, ohgpu_ogg_stream_result& aDemuxed, std::vector<ohgpu_ogg_packet>& aRecords,
                      ohgpu_vorbis_stream_result& aDecoded, uint64_t& aPcmFrom, std::vector<TUint>& aSent)
{
    memset(&aDemuxed, 0, sizeof(aDemuxed));
    memset(&aDecoded, 0, sizeof(aDecoded));
    aRecords.clear();
    const uint64_t from = d.ConsumedBytes(), have = from + d.PendingBytes();
    size_t k0 = 0;
    while (k0 < t.packets.size() && !(t.packets[k0].page_offset == from && t.packets[k0].segment == aOgg.first_page_segment)) k0++;
    TEST(k0 < t.packets.size() && t.packets[k0].seq == aOgg.expect_seq);
    aPcmFrom = k0 + 1 < t.packets.size() ? t.packets[k0 + 1].position : 0;
    for (size_t k = k0; k < t.packets.size() && t.packets[k].whole_at <= have; k++) {
        aDemuxed.packets++;
        if (aRecords.size() < aOgg.packet_capacity) {
            ohgpu_ogg_packet r;
            memset(&r, 0, sizeof(r));
            r.page_offset = t.packets[k].page_offset - from; r.segment = t.packets[k].segment; r.page_seq = t.packets[k].seq;
            aRecords.push_back(r);
            if (k > k0) { aSent[k]++; aDecoded.samples += t.packets[k].samples; }
            if (k + 1 == t.packets.size()) { aDemuxed.eos_seen = 1; aDemuxed.last_granule = t.granule; }
        }
    }
    aDemuxed.last_granule = aDemuxed.eos_seen ? t.granule : -1;
    return aRecords.size();
}

static void Drain(Sink& aSink, PlayableBatch* aBatch, std::vector<TByte>& aGot, std::vector<TUint>& aSizes, TUint64& aJiffies)
{
    std::vector<std::unique_ptr<ProcessorPcmBufTest>> procs;
    while (!aSink.iAudio.empty()) {
        MsgAudioPcm* m = aSink.iAudio.front();
        aSink.iAudio.pop_front();
        aSink.iAudioSeen++;
        TEST(m->TrackOffset() == aJiffies);
        aJiffies += m->Jiffies();
        MsgPlayable* p = m->CreatePlayable();
        aSizes.push_back(p->Bytes());
        if (aBatch) {
            procs.emplace_back(new ProcessorPcmBufTest());
            aBatch->Add(p, *procs.back());
        } else {
            p->RemoveRef();
        }
    }
    if (aBatch && !procs.empty()) {
        aBatch->Run();
        for (auto& pr : procs) { const Brn b = pr->Buf(); aGot.insert(aGot.end(), b.Ptr(), b.Ptr() + b.Bytes()); }
    }
}

static void TestTicksWithAStandIn(MsgFactory& f, const std::vector<TByte>& aOgg, const Truth& t, const std::vector<TByte>& aPcm)
{
    OggVorbisBatchDecoder d;
    Sink sink;
    CodecController controller(f, sink, Jiffies::kPerSecond);
    TUint64 trackOffset = 0, jiffies = 0;
    std::vector<TUint> sizes, sent(t.packets.size(), 0);
    std::vector<TByte> unused;
    const TUint frame = 2u * t.channels;
    uint64_t bytesOut = 0;
    for (size_t at = 0; at < aOgg.size(); at += 1500) {
        d.Push(Brn(aOgg.data() + at, (TUint)std::min<size_t>(1500, aOgg.size() - at)));
        ohgpu_ogg_stream_desc og;
        ohgpu_vorbis_stream_desc vo;
        if (!d.Collect(0, 0, 0, 0, 0, og, vo)) continue;
        TEST(og.src_bytes == d.PendingBytes() && og.serial == 0x5642 && vo.image_bytes == d.Image().size() && vo.max_samples >= OggVorbisBatchDecoder::kMaxPacketsPerTick);
        ohgpu_ogg_stream_result dem;
        ohgpu_vorbis_stream_result dec;
        std::vector<ohgpu_ogg_packet> recs;
        uint64_t pcmFrom = 0;
        if (StandIn(d, t, og, dem, recs, dec, pcmFrom, sent) == 0) continue;
        const uint64_t before = d.SamplesOutput();
        TEST(pcmFrom == before || dec.samples == 0);                                 // what a tick delivers follows what the last one did
        TEST(d.Apply(og, dem, recs.data(), dec, aPcm.data() + pcmFrom * frame, controller, trackOffset));
        bytesOut += (d.SamplesOutput() - before) * frame;
        Drain(sink, nullptr, unused, sizes, jiffies);
    }
    TEST(d.Finished() && d.PendingBytes() == 0 && !d.Corrupt());
    TEST(d.SamplesOutput() == (uint64_t)t.granule && bytesOut == (uint64_t)t.granule * frame);     // trimmed to the last page's granule position
    TEST(sink.iStreams == 1 && sink.iStreamBeforeAudio && trackOffset == jiffies);
    uint64_t total = 0;
    for (TUint s : sizes) { TEST(s <= DecodedAudio::kMaxBytes && s % frame == 0 && s > 0); total += s; }
    TEST(total == bytesOut);
    for (size_t k = 0; k < sent.size(); k++) TEST(sent[k] == (k ? 1u : 0u));           // behind a tick's first packet, which primes: every packet once
    ohgpu_ogg_stream_desc og;
    ohgpu_vorbis_stream_desc vo;
    TEST(!d.Collect(0, 0, 0, 0, 0, og, vo));                                          // a finished lane asks for nothing
    printf("stand-in: %zu packets, %llu samples a channel in %zu pieces\n", t.packets.size(), (unsigned long long)d.SamplesOutput(), sizes.size());
}

static void TestTicksThroughTheDevice(MsgFactory& f, const std::vector<TByte>& aOgg, const Truth& t, const std::vector<TByte>& aPcm)
{
    OggVorbisBatchDecoder d;
    Sink sink;
    CodecController controller(f, sink, Jiffies::kPerSecond);
    OggVorbisBatchDecoder::Lane lane = {&d, &controller, 0};
    PlayableBatch batch(f);
    std::vector<TByte> got;
    std::vector<TUint> sizes;
    TUint64 jiffies = 0;
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    for (size_t at = 0; at < aOgg.size(); at += 4000) {
        d.Push(Brn(aOgg.data() + at, (TUint)std::min<size_t>(4000, aOgg.size() - at)));
        const bool anything = d.PendingBytes() != 0 && !d.Finished();
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        OggVorbisBatchDecoder::Tick(f, &lane, 1);
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + (anything ? 1 : 0));                                 // one fused call a tick
        Drain(sink, &batch, got, sizes, jiffies);
    }
    const TUint frame = 2u * t.channels;
    TEST(d.Finished() && got.size() == (size_t)t.granule * frame && got.size() <= aPcm.size());
    int worst = 0;
    for (size_t i = 0; i + 1 < got.size() && i + 1 < aPcm.size(); i += 2) {
        const int a = (int16_t)((got[i] << 8) | got[i + 1]), b = (int16_t)((aPcm[i] << 8) | aPcm[i + 1]);
        worst = std::max(worst, a > b ? a - b : b - a);
    }
    TEST(worst <= 1);
    TEST(sink.iStreams == 1 && sink.iStreamBeforeAudio && lane.trackOffset == jiffies);
    printf("device: %zu bytes, largest difference from the model %d LSB\n", got.size(), worst);
}

int main(int argc, char** argv)
{
    if (argc < 5) { printf("usage: test_vorbis_decoder cpu|gpu stream.ogg truth pcm\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    const std::vector<TByte> ogg = ReadFile(argv[2]), pcm = ReadFile(argv[4]);
    const Truth truth = ReadTruth(argv[3]);
    TestRecogniseAndHead(ogg, truth);
    {
        MsgFactory f(gpu ? 0 : -1);
        TestTicksWithAStandIn(f, ogg, truth, pcm);
        if (gpu) TestTicksThroughTheDevice(f, ogg, truth, pcm);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
