// test_pcm_file_decoder.cpp -- PCM files in the host adapter (ohpipeline_amd/host/PcmFileDecoder.h: WavRecognise, AiffRecognise,
// AifcRecognise, PcmFileBatchDecoder).
// `test_pcm_file_decoder cpu` runs what needs no device: the three recognition rules and a decoder's state before any tick.
// `test_pcm_file_decoder gpu <manifest>` adds the whole path: per line of the manifest one lane -- a file, the bytes that must reach
// the processor, the sizes its messages must have, what it must throw (0 nothing, 1 CodecStreamCorrupt), its bit-depth limit, a
// sample to seek to once its stream has been announced (-1: none), and the fields its MsgDecodedStream must carry -- pushed in
// 20000-byte pieces over as many ticks as it takes, ONE Flush per tick for all lanes, every message read through a playable into
// ProcessorPcmBufTest.  The expectations are made by tests/test_iff_host_cpp.py from the record of the tests' own writer.
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
#include "../../ohpipeline_amd/host/PcmFileDecoder.h"
#include "../../ohpipeline_amd/host/Ramp.h"

using namespace OpenHome;
using namespace OpenHome::Media;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)
#define TEST_THROWS(expr, Exc) do { bool thrown_ = false; try { expr; } catch (Exc&) { thrown_ = true; } gChecks++; \
    if (!thrown_) { gFailures++; printf("FAILED %s:%d  %s did not throw\n", __FILE__, __LINE__, #expr); } } while (0)

static const TUint kPush = 20000;

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
        if (KindOf(aMsg) == MsgKind::DecodedStream) {
            const DecodedStreamInfo& s = static_cast<MsgDecodedStream*>(aMsg)->StreamInfo();
            iStreams++;
            iBitRate = s.BitRate(); iBitDepth = s.BitDepth(); iRate = s.SampleRate(); iChannels = s.NumChannels();
            iLength = s.TrackLength(); iStart = s.SampleStart(); iLossless = s.Lossless();
            iName.assign((const char*)s.CodecName().Ptr(), s.CodecName().Bytes());
            if (iStreams == 1) iStreamBeforeAudio = iAudioSeen == 0 && iAudio.empty();
        }
        aMsg->RemoveRef();
    }
    std::deque<MsgAudioPcm*> iAudio;
    TUint iStreams = 0, iAudioSeen = 0, iBitRate = 0, iBitDepth = 0, iRate = 0, iChannels = 0;
    TUint64 iLength = 0, iStart = 0;
    TBool iStreamBeforeAudio = false, iLossless = false;
    std::string iName;
};

static void TestRecognise()
{
    const TByte wav[13] = {'R', 'I', 'F', 'F', 1, 2, 3, 4, 'W', 'A', 'V', 'E', 'f'};
    const TByte aiff[12] = {'F', 'O', 'R', 'M', 0, 0, 0, 0, 'A', 'I', 'F', 'F'};
    const TByte aifc[12] = {'F', 'O', 'R', 'M', 9, 9, 9, 9, 'A', 'I', 'F', 'C'};
    const TByte avi[12] = {'R', 'I', 'F', 'F', 0, 0, 0, 0, 'A', 'V', 'I', ' '};
    const TByte mixed[12] = {'F', 'O', 'R', 'M', 0, 0, 0, 0, 'W', 'A', 'V', 'E'};
    TEST(WavRecognise(Brn(wav, 12)) && WavRecognise(Brn(wav, 13)) && !WavRecognise(Brn(wav, 11)) && !WavRecognise(Brn(wav, 0)));
    TEST(!AiffRecognise(Brn(wav, 12)) && !AifcRecognise(Brn(wav, 12)));
    TEST(AiffRecognise(Brn(aiff, 12)) && !AifcRecognise(Brn(aiff, 12)) && !WavRecognise(Brn(aiff, 12)) && !AiffRecognise(Brn(aiff, 11)));
    TEST(AifcRecognise(Brn(aifc, 12)) && !AiffRecognise(Brn(aifc, 12)) && !WavRecognise(Brn(aifc, 12)) && !AifcRecognise(Brn(aifc, 11)));
    TEST(!WavRecognise(Brn(avi, 12)) && !WavRecognise(Brn(mixed, 12)) && !AiffRecognise(Brn(mixed, 12)) && !AifcRecognise(Brn(mixed, 12)));
}

static void TestBeforeAnyTick()
{
    const TByte wav[12] = {'R', 'I', 'F', 'F', 0, 0, 0, 0, 'W', 'A', 'V', 'E'};
    PcmFileBatchDecoder d(32);
    d.Push(Brn(wav, 5));
    d.Push(Brn(wav + 5, 7));
    TEST(d.BytesPushed() == 12 && !d.Announced() && !d.Dropped() && d.NextFrame() == 0);
    PcmFileBatchDecoder::Lane lane = {&d, nullptr, 0};
    TEST(!PcmFileBatchDecoder::TrySeek(lane, 0) && lane.trackOffset == 0);            // (no stream before the first tick)
    TEST_THROWS(d.Result(), AssertionFailed);
    TEST_THROWS(PcmFileBatchDecoder(16), AssertionFailed);
}

struct LaneSpec {
    std::vector<TByte> file, want;
    std::vector<TUint> pieces;
    int throws, maxDepth;
    long long seek;
    TUint bitRate, depth, rate, channels;
    std::string name;
    unsigned long long length;
};

static void TestPipeline(MsgFactory& f, const std::string& aManifest)
{
    std::vector<LaneSpec> specs;
    std::ifstream in(aManifest);
    for (std::string line; std::getline(in, line); ) {
        std::istringstream ls(line);
        std::string file, want, pieces;
        LaneSpec s;
        ls >> file >> want >> pieces >> s.throws >> s.maxDepth >> s.seek >> s.bitRate >> s.depth >> s.rate >> s.channels >> s.name >> s.length;
        s.file = ReadFile(file);
        s.want = ReadFile(want);
        std::ifstream pf(pieces);
        for (TUint v; pf >> v; ) s.pieces.push_back(v);
        specs.push_back(s);
    }
    TEST(specs.size() == 5);
    std::vector<std::unique_ptr<PcmFileBatchDecoder>> decoders;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<PcmFileBatchDecoder::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    std::vector<std::vector<TUint>> sizes(specs.size());
    std::vector<TUint64> jiffies(specs.size(), 0);
    std::vector<bool> sought(specs.size(), false);
    size_t ticks = 0, throwsSeen = 0, seeks = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        decoders.emplace_back(new PcmFileBatchDecoder((TUint)specs[k].maxDepth));
        sinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerSecond));
        lanes.push_back({decoders[k].get(), controllers[k].get(), 0});
        ticks = std::max(ticks, (specs[k].file.size() + kPush - 1) / kPush);
    }
    PlayableBatch batch(f);
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    for (size_t t = 0; t < ticks; t++) {
        bool served = false;
        for (size_t k = 0; k < specs.size(); k++) {
            const size_t lo = t * kPush, hi = std::min(specs[k].file.size(), lo + kPush);
            if (lo < hi && !decoders[k]->Dropped()) decoders[k]->Push(Brn(specs[k].file.data() + lo, (TUint)(hi - lo)));
            if (hi == specs[k].file.size()) decoders[k]->End();
            served = served || !decoders[k]->Dropped();
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        try {
            PcmFileBatchDecoder::Flush(f, lanes.data(), lanes.size());
        } catch (CodecStreamCorrupt&) {
            throwsSeen++;
            for (size_t k = 0; k < specs.size(); k++) TEST(decoders[k]->Dropped() == (specs[k].throws != 0));
            for (size_t k = 0; k < specs.size(); k++) TEST(specs[k].throws != 0 || decoders[k]->Announced());      // every lane was served first
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + (served ? 1 : 0));                                  // one call a tick for all lanes
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
            TEST(lanes[k].trackOffset == jiffies[k]);
        }
        if (!procs.empty()) batch.Run();
        for (size_t i = 0; i < procs.size(); i++) {
            const Brn b = procs[i]->Buf();
            got[laneOf[i]].insert(got[laneOf[i]].end(), b.Ptr(), b.Ptr() + b.Bytes());
        }
        for (size_t k = 0; k < specs.size(); k++) {
            if (specs[k].seek < 0 || sought[k] || !decoders[k]->Announced()) continue;
            const TUint64 total = decoders[k]->Result().frames_total;
            TEST(total > (TUint64)specs[k].seek && sinks[k]->iStreams == 1 && sinks[k]->iStart == 0);
            TEST(!PcmFileBatchDecoder::TrySeek(lanes[k], total) && !PcmFileBatchDecoder::TrySeek(lanes[k], 1ull << 40));     // beyond the track: refused,
            TEST(lanes[k].trackOffset == jiffies[k] && sinks[k]->iStreams == 1);                                              // and nothing changes
            TEST(PcmFileBatchDecoder::TrySeek(lanes[k], (TUint64)specs[k].seek));
            TEST(decoders[k]->NextFrame() == (TUint64)specs[k].seek && sinks[k]->iStreams == 2 && sinks[k]->iStart == (TUint64)specs[k].seek);
            TEST(lanes[k].trackOffset == (TUint64)specs[k].seek * Jiffies::kPerSecond / specs[k].rate);
            jiffies[k] = lanes[k].trackOffset;
            sought[k] = true;
            seeks++;
        }
    }
    size_t bytesChecked = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        if (got[k] != specs[k].want || sizes[k] != specs[k].pieces)
            printf("lane %zu: %zu bytes in %zu messages where %zu in %zu are due; next frame %llu\n", k, got[k].size(), sizes[k].size(), specs[k].want.size(), specs[k].pieces.size(),
                   (unsigned long long)decoders[k]->NextFrame());
        TEST(got[k].size() == specs[k].want.size());
        TEST(got[k] == specs[k].want);
        TEST(sizes[k] == specs[k].pieces);
        const Sink& s = *sinks[k];
        if (!specs[k].throws) {
            TEST(s.iStreams == (specs[k].seek < 0 ? 1u : 2u) && s.iStreamBeforeAudio && s.iLossless);
            TEST(s.iBitRate == specs[k].bitRate && s.iBitDepth == specs[k].depth && s.iRate == specs[k].rate && s.iChannels == specs[k].channels);
            TEST(s.iName == specs[k].name && s.iLength == specs[k].length);
        } else {
            TEST(got[k].empty() && s.iStreams == 0 && decoders[k]->Result().status == OHGPU_IFF_NOT_IFF);
        }
        bytesChecked += got[k].size();
    }
    TEST(throwsSeen == 1 && seeks == 1);
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", specs.size(), ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: test_pcm_file_decoder cpu | gpu <manifest>\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    TestRecognise();
    TestBeforeAnyTick();
    printf("cpu: %d checks\n", gChecks);
    if (gpu && argc > 2) {
        MsgFactory f(0);
        TestPipeline(f, argv[2]);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
