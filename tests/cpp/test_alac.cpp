// test_alac.cpp -- Apple Lossless in the host adapter (ohpipeline_amd/host/AlacDecoder.h: AlacBatchDecoder).
// `test_alac cpu` runs what needs no device: the configuration with and without its atoms, the packet queue's bookkeeping, the
// refusals (more than two channels, a frame length above 4096), the rule Decode cuts a packet into messages by, the seek.
// `test_alac gpu <manifest>` adds the whole path: per line of the manifest one lane -- its cookie, its packets and their sizes, the
// bytes that must reach the processor, the sizes its messages must have, whether the lane must throw -- two packets pushed per tick,
// ONE Flush per tick for all lanes, every message read through a playable into ProcessorPcmBufTest.  The expectations are made by
// tests/test_alac_host_cpp.py from the PCM the packets were encoded from and the plain-Python model.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/AlacDecoder.h"
#include "../../ohpipeline_amd/host/Msg.h"

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

static std::vector<TByte> Cookie(TUint aFrameLength, TUint aDepth, TUint aChannels, TUint aRate, TUint aVersion = 0)
{
    std::vector<TByte> c(24, 0);
    for (int k = 0; k < 4; k++) { c[k] = (TByte)(aFrameLength >> (24 - 8 * k)); c[20 + k] = (TByte)(aRate >> (24 - 8 * k)); }
    c[4] = (TByte)aVersion; c[5] = (TByte)aDepth; c[6] = 40; c[7] = 10; c[8] = 14; c[9] = (TByte)aChannels; c[11] = 255;
    return c;
}

class Sink : public IPipelineElementDownstream {
public:
    void Push(Msg* aMsg) override
    {
        if (KindOf(aMsg) == MsgKind::AudioPcm) { iAudio.push_back(static_cast<MsgAudioPcm*>(aMsg)); return; }
        if (KindOf(aMsg) == MsgKind::DecodedStream) { iStreams++; iStreamBeforeAudio = iStreamBeforeAudio && iAudioSeen == 0; }
        aMsg->RemoveRef();
    }
    std::deque<MsgAudioPcm*> iAudio;
    TUint iStreams = 0, iAudioSeen = 0;
    TBool iStreamBeforeAudio = true;
};

static void TestBookkeeping()
{
    const std::vector<TByte> plain = Cookie(4096, 24, 2, 96000);
    std::vector<TByte> front = {0, 0, 0, 12, 'f', 'r', 'm', 'a', 'a', 'l', 'a', 'c', 0, 0, 0, 36, 'a', 'l', 'a', 'c', 0, 0, 0, 0};
    front.insert(front.end(), plain.begin(), plain.end());
    const std::vector<TByte> wrapped = front;
    for (const std::vector<TByte>* c : {&plain, &wrapped}) {
        AlacBatchDecoder d;
        TEST(!d.Configured());
        d.SetConfig(Brn(c->data(), (TUint)c->size()), 48000, 480000);
        TEST(d.Configured() && d.Config().frame_length == 4096 && d.Config().bit_depth == 24 && d.Config().channels == 2 && d.Config().sample_rate == 96000);
        TEST(d.Config().pb == 40 && d.Config().mb == 10 && d.Config().kb == 14 && d.Config().max_run == 255);
    }
    // the queue: packets wait for the next Flush, a seek drops them and renumbers the next one
    AlacBatchDecoder d;
    TEST_THROWS(d.Config(), AssertionFailed);
    TEST_THROWS(d.PushPacket(Brn(plain.data(), 3)), AssertionFailed);
    d.SetConfig(Brn(plain.data(), 24), 44100, 441000);
    TEST(d.PendingPackets() == 0 && d.PendingBytes() == 0 && d.NextPacket() == 0 && d.SamplesDecoded() == 0 && !d.Corrupt());
    const TByte bytes[16] = {0};
    d.PushPacket(Brn(bytes, 5));
    d.PushPacket(Brn(bytes, 0));
    d.PushPacket(Brn(bytes, 16));
    TEST(d.PendingPackets() == 3 && d.PendingBytes() == 21);
    d.SeekToPacket(77);
    TEST(d.PendingPackets() == 0 && d.PendingBytes() == 0 && d.NextPacket() == 77 && !d.Corrupt());
    d.PushPacket(Brn(bytes, 9));
    TEST(d.PendingPackets() == 1 && d.PendingBytes() == 9);
    // the refusals (AlacApple.cpp:147-157): what the decoded buffer has no room for, and what is no configuration
    { AlacBatchDecoder x; const auto c = Cookie(4096, 16, 3, 44100); TEST_THROWS(x.SetConfig(Brn(c.data(), 24), 44100, 1), CodecStreamCorrupt); TEST(x.Corrupt() && !x.Configured()); }
    { AlacBatchDecoder x; const auto c = Cookie(4096, 16, 6, 44100); TEST_THROWS(x.SetConfig(Brn(c.data(), 24), 44100, 1), CodecStreamCorrupt); }
    { AlacBatchDecoder x; const auto c = Cookie(4097, 16, 2, 44100); TEST_THROWS(x.SetConfig(Brn(c.data(), 24), 44100, 1), CodecStreamCorrupt); }
    { AlacBatchDecoder x; const auto c = Cookie(0, 16, 2, 44100); TEST_THROWS(x.SetConfig(Brn(c.data(), 24), 44100, 1), CodecStreamCorrupt); }
    { AlacBatchDecoder x; const auto c = Cookie(4096, 16, 2, 44100); TEST_THROWS(x.SetConfig(Brn(c.data(), 23), 44100, 1), CodecStreamCorrupt); }
    { AlacBatchDecoder x; const auto c = Cookie(4096, 16, 2, 44100, 1); TEST_THROWS(x.SetConfig(Brn(c.data(), 24), 44100, 1), CodecStreamCorrupt); }
    { AlacBatchDecoder x; const auto c = Cookie(4096, 16, 2, 44100); TEST_THROWS(x.SetConfig(Brn(c.data(), 24), 0, 1), CodecStreamCorrupt); }
    { AlacBatchDecoder x; const auto c = Cookie(4096, 12, 2, 44100); TEST_THROWS(x.SetConfig(Brn(c.data(), 24), 44100, 1), CodecStreamFeatureUnsupported); }
    { AlacBatchDecoder x; const auto c = Cookie(4096, 32, 1, 44100); x.SetConfig(Brn(c.data(), 24), 44100, 1); TEST(x.Configured()); }
    // AlacAppleBase.cpp:94-111: pieces of 9216 bytes and the rest
    TEST(AlacBatchDecoder::kMaxPieceBytes == 9216);
    TEST(AlacBatchDecoder::Pieces(0) == 0 && AlacBatchDecoder::Pieces(1) == 1 && AlacBatchDecoder::Pieces(9216) == 1 && AlacBatchDecoder::Pieces(9217) == 2);
    TEST(AlacBatchDecoder::Pieces(4096 * 2 * 2) == 2 && AlacBatchDecoder::Pieces(4096 * 2 * 3) == 3 && AlacBatchDecoder::Pieces(4096 * 2 * 4) == 4);
}

struct LaneSpec {
    std::vector<TByte> cookie, packets, want;
    std::vector<TUint> sizes, pieces;
    TUint rate;
    bool throws;
};

static std::vector<TUint> ReadNumbers(const std::string& aPath)
{
    std::vector<TUint> out;
    std::ifstream in(aPath);
    for (TUint v; in >> v; ) out.push_back(v);
    return out;
}

static void TestPipeline(MsgFactory& f, const std::string& aManifest)
{
    std::vector<LaneSpec> specs;
    std::ifstream in(aManifest);
    for (std::string line; std::getline(in, line); ) {
        std::istringstream ls(line);
        std::string stem;
        int throws = 0;
        LaneSpec s;
        ls >> stem >> s.rate >> throws;
        s.cookie = ReadFile(stem + ".cookie");
        s.packets = ReadFile(stem + ".packets");
        s.want = ReadFile(stem + ".want");
        s.sizes = ReadNumbers(stem + ".sizes");
        s.pieces = ReadNumbers(stem + ".pieces");
        s.throws = throws != 0;
        specs.push_back(s);
    }
    TEST(specs.size() == 5);
    const size_t kPerTick = 2;
    std::vector<std::unique_ptr<AlacBatchDecoder>> decoders;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<AlacBatchDecoder::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    std::vector<std::vector<TUint>> sizes(specs.size());
    std::vector<TUint64> jiffies(specs.size(), 0);
    std::vector<size_t> offsets(specs.size(), 0);
    size_t ticks = 0, throwsSeen = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        decoders.emplace_back(new AlacBatchDecoder());
        decoders[k]->SetConfig(Brn(specs[k].cookie.data(), (TUint)specs[k].cookie.size()), specs[k].rate, 10 * specs[k].rate);
        sinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerSecond));
        lanes.push_back({decoders[k].get(), controllers[k].get(), 0});
        ticks = std::max(ticks, (specs[k].sizes.size() + kPerTick - 1) / kPerTick);
    }
    PlayableBatch batch(f);
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    for (size_t t = 0; t < ticks; t++) {
        bool anything = false;
        for (size_t k = 0; k < specs.size(); k++) {
            for (size_t p = t * kPerTick; p < std::min(specs[k].sizes.size(), (t + 1) * kPerTick) && !decoders[k]->Corrupt(); p++) {
                decoders[k]->PushPacket(Brn(specs[k].packets.data() + offsets[k], specs[k].sizes[p]));
                offsets[k] += specs[k].sizes[p];
            }
            anything = anything || (decoders[k]->PendingPackets() != 0 && !decoders[k]->Corrupt());
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        try {
            AlacBatchDecoder::Flush(f, lanes.data(), lanes.size());
        } catch (CodecStreamCorrupt&) {
            throwsSeen++;
            for (size_t k = 0; k < specs.size(); k++) TEST(decoders[k]->Corrupt() == specs[k].throws);
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + (anything ? 1 : 0));                                 // every lane's decode in one device call
        for (size_t k = 0; k < specs.size(); k++) TEST(decoders[k]->PendingPackets() == 0);
        std::vector<std::unique_ptr<ProcessorPcmBufTest>> procs;
        std::vector<size_t> laneOf;
        for (size_t k = 0; k < specs.size(); k++) {
            while (!sinks[k]->iAudio.empty()) {
                MsgAudioPcm* m = sinks[k]->iAudio.front();
                sinks[k]->iAudio.pop_front();
                sinks[k]->iAudioSeen++;
                TEST(m->TrackOffset() == jiffies[k]);
                jiffies[k] += m->Jiffies();
                MsgPlayable* p = m->CreatePlayable();
                sizes[k].push_back(p->Bytes());
                procs.emplace_back(new ProcessorPcmBufTest());
                laneOf.push_back(k);
                batch.Add(p, *procs.back());
            }
        }
        if (!procs.empty()) batch.Run();
        for (size_t i = 0; i < procs.size(); i++) {
            const Brn b = procs[i]->Buf();
            got[laneOf[i]].insert(got[laneOf[i]].end(), b.Ptr(), b.Ptr() + b.Bytes());
        }
    }
    size_t bytesChecked = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        const ohgpu_alac_config& c = decoders[k]->Config();
        TEST(got[k].size() == specs[k].want.size());
        TEST(got[k] == specs[k].want);
        TEST(sizes[k] == specs[k].pieces);
        TEST(sinks[k]->iStreams == 1 && sinks[k]->iStreamBeforeAudio);
        TEST(lanes[k].trackOffset == jiffies[k]);
        TEST(decoders[k]->SamplesDecoded() * c.channels * (c.bit_depth / 8) == got[k].size());
        if (!specs[k].throws) TEST(decoders[k]->NextPacket() == specs[k].sizes.size());
        if (specs[k].throws) TEST(!got[k].empty() && decoders[k]->NextPacket() < specs[k].sizes.size());      // its good packets came first
        bytesChecked += got[k].size();
    }
    TEST(throwsSeen == 1);
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", specs.size(), ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: test_alac cpu | gpu manifest\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    TestBookkeeping();
    printf("cpu: %d checks\n", gChecks);
    if (gpu && argc > 2) {
        MsgFactory f(0);
        TestPipeline(f, argv[2]);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
