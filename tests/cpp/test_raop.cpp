// test_raop.cpp -- RAOP audio in the host adapter (ohpipeline_amd/host/RaopDecoder.h: RaopBatchDecoder).
// `test_raop cpu` runs what needs no device: the fmtp string and its refusals, datagram parsing and every InvalidRaopPacket case, the
// 1472-byte limit, the queue's bookkeeping (every payload at a 16-byte boundary of the pending arena), the key-length asserts.
// `test_raop gpu <manifest>` adds the whole path: per line of the manifest one lane -- its fmtp string, key and IV, its datagrams and
// their sizes, the bytes that must reach the processor, the sizes its messages must have, whether the lane must throw -- two
// datagrams pushed per tick, ONE Flush per tick for all lanes, every message read through a playable into ProcessorPcmBufTest.  The
// expectations are made by tests/test_raop_host_cpp.py from the PCM the packets were encoded from and the plain-Python model chain.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/Msg.h"
#include "../../ohpipeline_amd/host/RaopDecoder.h"

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

static Brn Text(const char* aText) { return Brn((const TByte*)aText, (TUint)strlen(aText)); }

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

static const char* kFmtp = "96 352 0 16 40 10 14 2 255 0 0 44100";

static void TestBookkeeping()
{
    TByte key[17], iv[17];
    for (int k = 0; k < 17; k++) { key[k] = (TByte)k; iv[k] = (TByte)(0xf0 + k); }
    {
        RaopBatchDecoder d;
        TEST(!d.Configured());
        TEST_THROWS(d.Config(), AssertionFailed);
        d.SetSession(Text(kFmtp), Brn(key, 16), Brn(iv, 16));
        const ohgpu_alac_config& c = d.Config();
        TEST(d.Configured() && c.frame_length == 352 && c.compatible_version == 0 && c.bit_depth == 16 && c.pb == 40 && c.mb == 10 && c.kb == 14);
        TEST(c.channels == 2 && c.max_run == 255 && c.max_frame_bytes == 0 && c.avg_bit_rate == 0 && c.sample_rate == 44100);
        d.SetSession(Text("0 4096 0 24 40 10 14 1 65535 4294967295 7 48000 and more"), Brn(key, 16), Brn(iv, 16));
        TEST(d.Config().frame_length == 4096 && d.Config().bit_depth == 24 && d.Config().channels == 1 && d.Config().max_run == 65535);
        TEST(d.Config().max_frame_bytes == 4294967295u && d.Config().avg_bit_rate == 7 && d.Config().sample_rate == 48000);
    }
    // the refusals: what is no fmtp string (CodecRaopApple.cpp:80-83), what would be truncated, what the decoded buffer has no room for (:85-94)
    for (const char* bad : {"", "96", "96 352 0 16 40 10 14 2 255 0 0", "96 352 0 16 40 10 14 2 255 0 0 x", "96 352 0 16 40 10 14 2 255 0 0 -1", "96 352 1 16 40 10 14 2 255 0 0 44100",
                            "96 352 0 256 40 10 14 2 255 0 0 44100", "96 352 0 16 40 10 14 2 65536 0 0 44100", "96 4294967296 0 16 40 10 14 2 255 0 0 44100",
                            "96 4097 0 16 40 10 14 2 255 0 0 44100", "96 0 0 16 40 10 14 2 255 0 0 44100", "96 352 0 16 40 10 14 3 255 0 0 44100", "96 352 0 16 40 10 14 0 255 0 0 44100"}) {
        RaopBatchDecoder x;
        TEST_THROWS(x.SetSession(Text(bad), Brn(key, 16), Brn(iv, 16)), CodecStreamCorrupt);
        TEST(x.Corrupt() && !x.Configured());
    }
    { RaopBatchDecoder x; TEST_THROWS(x.SetSession(Text("96 352 0 12 40 10 14 2 255 0 0 44100"), Brn(key, 16), Brn(iv, 16)), CodecStreamFeatureUnsupported); }
    { RaopBatchDecoder x; x.SetSession(Text("96 4096 0 32 40 10 14 1 255 0 0 44100"), Brn(key, 16), Brn(iv, 16)); TEST(x.Configured()); }
    // RaopAudioDecryptor wants a key and an IV: 16 bytes each
    for (TUint n : {0u, 15u, 17u}) {
        RaopBatchDecoder x;
        TEST_THROWS(x.SetSession(Text(kFmtp), Brn(key, n), Brn(iv, 16)), AssertionFailed);
        TEST_THROWS(x.SetSession(Text(kFmtp), Brn(key, 16), Brn(iv, n)), AssertionFailed);
        TEST(!x.Configured());
    }
    // datagrams: 4 bytes of RTP header, 8 of timestamp and ssrc, the payload
    RaopBatchDecoder d;
    std::vector<TByte> g(RaopBatchDecoder::kMaxDatagramBytes + 1, 0x5a);
    TEST_THROWS(d.PushDatagram(Brn(g.data(), 12)), AssertionFailed);              // no session yet
    d.SetSession(Text(kFmtp), Brn(key, 16), Brn(iv, 16));
    TEST(d.PendingPackets() == 0 && d.PendingBytes() == 0 && d.SamplesDecoded() == 0 && d.PacketsDecoded() == 0 && !d.Corrupt());
    for (TUint n : {0u, 1u, 3u}) TEST_THROWS(d.PushDatagram(Brn(g.data(), n)), InvalidRaopPacket);        // RtpPacketRaop::Set
    for (TUint n : {4u, 5u, 11u}) TEST_THROWS(d.PushDatagram(Brn(g.data(), n)), InvalidRaopPacket);       // RaopPacketAudio::Set
    TEST_THROWS(d.PushDatagram(Brn(g.data(), RaopBatchDecoder::kMaxDatagramBytes + 1)), InvalidRaopPacket);
    TEST(d.PendingPackets() == 0);
    const TByte head[12] = {0x80, 0xe0, 0xfe, 0xdc, 0x01, 0x02, 0x03, 0x04, 0xa1, 0xb2, 0xc3, 0xd4};
    memcpy(g.data(), head, 12);
    d.PushDatagram(Brn(g.data(), 12 + 5));
    TEST(d.LastSeq() == 0xfedc && d.LastTimestamp() == 0x01020304 && d.LastSsrc() == 0xa1b2c3d4u);
    TEST(d.PendingPackets() == 1 && d.PendingBytes() == 5 && d.PendingOffset(0) == 0);
    g[0] = 0x00; g[1] = 0x00; g[3] = 0xdd;                                        // version 0, type 0: a resent packet of some senders
    d.PushDatagram(Brn(g.data(), 12));                                            // an empty payload is a packet
    d.PushDatagram(Brn(g.data(), 12 + 33));
    d.PushDatagram(Brn(g.data(), RaopBatchDecoder::kMaxDatagramBytes));
    TEST(d.LastSeq() == 0xfedd);
    TEST(d.PendingPackets() == 4 && d.PendingBytes() == 5 + 0 + 33 + 1460);
    TEST(d.PendingOffset(1) == 16 && d.PendingOffset(2) == 16 && d.PendingOffset(3) == 64);      // every payload at a 16-byte boundary
    TEST_THROWS(d.PendingOffset(4), AssertionFailed);
    d.SetSession(Text(kFmtp), Brn(key, 16), Brn(iv, 16));                         // a new session drops what is queued
    TEST(d.PendingPackets() == 0 && d.PendingBytes() == 0);
    TEST(RaopBatchDecoder::kMaxPieceBytes == 9216 && RaopBatchDecoder::kMaxDatagramBytes == 1472);
    TEST(RaopBatchDecoder::Pieces(0) == 0 && RaopBatchDecoder::Pieces(9216) == 1 && RaopBatchDecoder::Pieces(9217) == 2 && RaopBatchDecoder::Pieces(4096 * 2 * 4) == 4);
}

struct LaneSpec {
    std::string fmtp;
    std::vector<TByte> secret, datagrams, want;
    std::vector<TUint> sizes, pieces;
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
        ls >> stem >> throws;
        const std::vector<TByte> text = ReadFile(stem + ".fmtp");
        s.fmtp.assign(text.begin(), text.end());
        s.secret = ReadFile(stem + ".secret");                       // key, then IV
        s.datagrams = ReadFile(stem + ".datagrams");
        s.want = ReadFile(stem + ".want");
        s.sizes = ReadNumbers(stem + ".sizes");
        s.pieces = ReadNumbers(stem + ".pieces");
        s.throws = throws != 0;
        specs.push_back(s);
    }
    TEST(specs.size() == 4);
    const size_t kPerTick = 2;
    std::vector<std::unique_ptr<RaopBatchDecoder>> decoders;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<RaopBatchDecoder::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    std::vector<std::vector<TUint>> sizes(specs.size());
    std::vector<TUint64> jiffies(specs.size(), 0);
    std::vector<size_t> offsets(specs.size(), 0);
    size_t ticks = 0, throwsSeen = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        TEST(specs[k].secret.size() == 32);
        decoders.emplace_back(new RaopBatchDecoder());
        decoders[k]->SetSession(Brn((const TByte*)specs[k].fmtp.data(), (TUint)specs[k].fmtp.size()), Brn(specs[k].secret.data(), 16), Brn(specs[k].secret.data() + 16, 16));
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
                decoders[k]->PushDatagram(Brn(specs[k].datagrams.data() + offsets[k], specs[k].sizes[p]));
                offsets[k] += specs[k].sizes[p];
            }
            anything = anything || (decoders[k]->PendingPackets() != 0 && !decoders[k]->Corrupt());
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        try {
            RaopBatchDecoder::Flush(f, lanes.data(), lanes.size());
        } catch (CodecStreamCorrupt&) {
            throwsSeen++;
            for (size_t k = 0; k < specs.size(); k++) TEST(decoders[k]->Corrupt() == specs[k].throws);
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + (anything ? 1 : 0));                                 // every lane's decrypt and decode in one device call
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
        if (!specs[k].throws) TEST(decoders[k]->PacketsDecoded() == specs[k].sizes.size());
        if (specs[k].throws) TEST(!got[k].empty() && decoders[k]->PacketsDecoded() < specs[k].sizes.size());      // its good packets came first
        bytesChecked += got[k].size();
    }
    TEST(throwsSeen == 1);
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", specs.size(), ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: test_raop cpu | gpu manifest\n"); return 2; }
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
