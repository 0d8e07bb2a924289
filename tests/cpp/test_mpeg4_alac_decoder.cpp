// test_mpeg4_alac_decoder.cpp -- Apple Lossless in an MPEG-4 file in the host adapter (ohpipeline_amd/host/Mpeg4AlacDecoder.h:
// Mpeg4Recognise, Mpeg4AlacBatchDecoder).
// `test_mpeg4_alac_decoder cpu <moov-first.m4a> <whole-at> <moov-last.m4a> <whole-at>` runs what needs no device: the recognition
// rule, the top-level peek over ragged pushes (the head is whole exactly when the stated byte has arrived), the refusals.
// `test_mpeg4_alac_decoder gpu ... <manifest>` adds the whole path: per line of the manifest one lane -- a file, the bytes that must
// reach the processor, the sizes its messages must have, what it must throw (0 nothing, 2 CodecStreamFeatureUnsupported), a frame to
// seek to once its head has been read (-1: none) and the first frame that seek must report -- pushed in 1000-byte pieces over as many
// ticks as it takes, ONE Flush per tick for all lanes, every message read through a playable into ProcessorPcmBufTest.  The
// expectations are made by tests/test_mp4_host_cpp.py from the PCM the fixtures were encoded from.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/Mpeg4AlacDecoder.h"
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

static void TestRecognise(const std::vector<TByte>& aFile)
{
    TEST(Mpeg4Recognise(Brn(aFile.data(), 8)) && Mpeg4Recognise(Brn(aFile.data(), (TUint)aFile.size())));
    TEST(!Mpeg4Recognise(Brn(aFile.data(), 7)) && !Mpeg4Recognise(Brn(aFile.data(), 0)));
    std::vector<TByte> other(aFile.begin(), aFile.begin() + 16);
    other[7] = 'q';
    TEST(!Mpeg4Recognise(Brn(other.data(), 16)));
    const TByte riff[12] = {'R', 'I', 'F', 'F', 0, 0, 0, 0, 'W', 'A', 'V', 'E'};
    TEST(!Mpeg4Recognise(Brn(riff, 12)));
}

static void TestPeek(const std::vector<TByte>& aFile, size_t aWholeAt)
{
    // ragged pushes: the head is whole exactly when byte aWholeAt - 1 has arrived, and nothing is read before a Flush
    const TUint steps[] = {3, 1, 2, 5, 7, 11, 13, 1, 1, 40, 17, 60, 200, 1, 333};
    Mpeg4AlacBatchDecoder d;
    size_t at = 0, k = 0;
    while (at < aFile.size()) {
        TEST(d.HeadWhole() == (at >= aWholeAt));
        const size_t n = std::min<size_t>(steps[k++ % (sizeof(steps) / sizeof(steps[0]))], aFile.size() - at);
        d.Push(Brn(aFile.data() + at, (TUint)n));
        at += n;
        TEST(d.BytesPushed() == at && !d.HeadRead() && !d.Corrupt());
    }
    TEST(d.HeadWhole() && d.Extent() == aFile.size() && d.TopLevelBoxes() == 3 && d.NextPacket() == 0);
    TUint64 first = 0;
    TEST(!d.TrySeek(0, first));                                                      // (no table before the head has been read)
    TEST_THROWS(d.Result(), AssertionFailed);
}

static void TestRefusals(const std::vector<TByte>& aFile)
{
    const TByte riff[12] = {'R', 'I', 'F', 'F', 0, 0, 0, 0, 'W', 'A', 'V', 'E'};
    { Mpeg4AlacBatchDecoder x; x.Push(Brn(riff, 7)); TEST(!x.Corrupt()); TEST_THROWS(x.Push(Brn(riff + 7, 1)), CodecStreamCorrupt); TEST(x.Corrupt()); }
    { Mpeg4AlacBatchDecoder x; TEST_THROWS(x.Push(Brn(riff, 12)), CodecStreamCorrupt); }
    {   // a top-level size no walk accepts ends the peek; the head counts as whole once `moov` has been seen
        std::vector<TByte> bad(aFile.begin(), aFile.begin() + 64);
        bad[24] = 0; bad[25] = 0; bad[26] = 0; bad[27] = 3;                          // the box behind ftyp: a size of 3
        Mpeg4AlacBatchDecoder x;
        x.Push(Brn(bad.data(), 64));
        TEST(!x.Corrupt() && x.TopLevelBoxes() == 2);
    }
}

struct LaneSpec {
    std::vector<TByte> file, want;
    std::vector<TUint> pieces;
    int throws;
    long long seekFrame, seekFirst;
};

static void TestPipeline(MsgFactory& f, const std::string& aManifest)
{
    std::vector<LaneSpec> specs;
    std::ifstream in(aManifest);
    for (std::string line; std::getline(in, line); ) {
        std::istringstream ls(line);
        std::string file, want, pieces;
        LaneSpec s;
        ls >> file >> want >> pieces >> s.throws >> s.seekFrame >> s.seekFirst;
        s.file = ReadFile(file);
        s.want = ReadFile(want);
        std::ifstream pf(pieces);
        for (TUint v; pf >> v; ) s.pieces.push_back(v);
        specs.push_back(s);
    }
    TEST(specs.size() == 5);
    std::vector<std::unique_ptr<Mpeg4AlacBatchDecoder>> decoders;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<Mpeg4AlacBatchDecoder::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    std::vector<std::vector<TUint>> sizes(specs.size());
    std::vector<TUint64> jiffies(specs.size(), 0);
    std::vector<bool> sought(specs.size(), false);
    size_t ticks = 0, throwsSeen = 0, seeks = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        decoders.emplace_back(new Mpeg4AlacBatchDecoder());
        sinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerSecond));
        lanes.push_back({decoders[k].get(), controllers[k].get(), 0});
        ticks = std::max(ticks, (specs[k].file.size() + 999) / 1000);
    }
    PlayableBatch batch(f);
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    for (size_t t = 0; t < ticks; t++) {
        bool heads = false;
        for (size_t k = 0; k < specs.size(); k++) {
            const size_t lo = t * 1000, hi = std::min(specs[k].file.size(), lo + 1000);
            if (lo < hi && !decoders[k]->Corrupt()) decoders[k]->Push(Brn(specs[k].file.data() + lo, (TUint)(hi - lo)));
            heads = heads || (decoders[k]->HeadWhole() && !decoders[k]->HeadRead() && !decoders[k]->Corrupt());
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        try {
            Mpeg4AlacBatchDecoder::Flush(f, lanes.data(), lanes.size());
        } catch (CodecStreamFeatureUnsupported&) {
            throwsSeen++;
            for (size_t k = 0; k < specs.size(); k++) TEST(decoders[k]->Corrupt() == (specs[k].throws != 0));
            for (size_t k = 0; k < specs.size(); k++) TEST(decoders[k]->HeadRead() == decoders[k]->HeadWhole());      // every lane was served first
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        bool audio = false;
        for (size_t k = 0; k < specs.size(); k++) audio = audio || !sinks[k]->iAudio.empty();
        TEST(calls1 == calls0 + (heads ? 1 : 0) + (audio ? 1 : 0));                  // one call for the heads of the tick, one decode for all lanes
        for (size_t k = 0; k < specs.size(); k++) {
            if (specs[k].seekFrame < 0 || sought[k] || !decoders[k]->HeadRead()) continue;
            TUint64 first = 0;
            TEST(sinks[k]->iAudio.empty());                                          // (the seek comes before the lane's first packet is whole)
            TEST(decoders[k]->TrySeek((TUint64)specs[k].seekFrame, first) && first == (TUint64)specs[k].seekFirst);
            TEST(decoders[k]->NextPacket() == 2 && decoders[k]->Alac().NextPacket() == 2);
            TEST(!decoders[k]->TrySeek(1ull << 40, first));
            sought[k] = true;
            seeks++;
        }
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
        if (got[k] != specs[k].want || sizes[k] != specs[k].pieces)
            printf("lane %zu: %zu bytes in %zu messages where %zu in %zu are due; next packet %llu\n", k, got[k].size(), sizes[k].size(), specs[k].want.size(), specs[k].pieces.size(),
                   (unsigned long long)decoders[k]->NextPacket());
        TEST(got[k].size() == specs[k].want.size());
        TEST(got[k] == specs[k].want);
        TEST(sizes[k] == specs[k].pieces);
        if (!specs[k].throws) TEST(sinks[k]->iStreams == 1 && sinks[k]->iStreamBeforeAudio && decoders[k]->NextPacket() == decoders[k]->Result().samples);
        if (specs[k].throws) TEST(got[k].empty() && decoders[k]->Result().status == OHGPU_MP4_NOT_ALAC && decoders[k]->Result().codec == 0x6d703461u);
        TEST(lanes[k].trackOffset == jiffies[k]);
        bytesChecked += got[k].size();
    }
    TEST(throwsSeen == 1 && seeks == 1);
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", specs.size(), ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    if (argc < 6) { printf("usage: test_mpeg4_alac_decoder cpu|gpu first.m4a whole-at last.m4a whole-at [manifest]\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    const std::vector<TByte> first = ReadFile(argv[2]), last = ReadFile(argv[4]);
    TestRecognise(first);
    TestPeek(first, (size_t)atol(argv[3]));
    TestPeek(last, (size_t)atol(argv[5]));
    TestRefusals(first);
    printf("cpu: %d checks\n", gChecks);
    if (gpu && argc > 6) {
        MsgFactory f(0);
        TestPipeline(f, argv[6]);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
