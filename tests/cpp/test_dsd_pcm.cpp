// test_dsd_pcm.cpp -- the DSD -> PCM element of the host adapter (ohpipeline_amd/host/DsdPcmConverter.{h,cpp}).
// `test_dsd_pcm cpu` runs what needs no device on a control-plane-only factory: the filter's design, a lane's bookkeeping (frames
// that are whole, the window the next Flush sends, the N - D bits of history kept and nothing older), the announced stream and the
// pieces of at most 9216 bytes.
// `test_dsd_pcm gpu` runs five lanes of mixed formats over several ticks -- ragged pushes, a tick without input, one lane joining
// mid-run -- ONE device call per tick, every message read through a playable into ProcessorPcmBufTest, and holds each lane's bytes
// to a single-shot conversion of its whole stream (a fresh converter, one Flush).
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <random>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/DsdPcmConverter.h"
#include "../../ohpipeline_amd/host/Msg.h"

using namespace OpenHome;
using namespace OpenHome::Media;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)
#define TEST_THROWS(expr, Exc) do { bool thrown_ = false; try { expr; } catch (Exc&) { thrown_ = true; } gChecks++; \
    if (!thrown_) { gFailures++; printf("FAILED %s:%d  %s did not throw\n", __FILE__, __LINE__, #expr); } } while (0)

static const TUint kDsdRate = 2822400, kPcmRate = 88200;

class Sink : public IPipelineElementDownstream {
public:
    void Push(Msg* aMsg) override
    {
        if (KindOf(aMsg) == MsgKind::AudioPcm) { iAudio.push_back(static_cast<MsgAudioPcm*>(aMsg)); return; }
        if (KindOf(aMsg) == MsgKind::DecodedStream) {
            iStreams++;
            iStreamBeforeAudio = iStreamBeforeAudio && iAudio.empty() && iAudioSeen == 0;
            iInfo = static_cast<MsgDecodedStream*>(aMsg)->StreamInfo();
        }
        aMsg->RemoveRef();
    }
    std::deque<MsgAudioPcm*> iAudio;
    DecodedStreamInfo iInfo;
    TUint iStreams = 0, iAudioSeen = 0;
    TBool iStreamBeforeAudio = true;
};

static void TestBookkeeping(MsgFactory& f)
{
    DsdPcmFilter filter(f, kDsdRate, kPcmRate);
    TEST(filter.Decimation() == 32 && filter.TapsPerOutput() == 16 && filter.Coefficients().size() == 512 && filter.Handle() == nullptr);
    int64_t sum = 0, sabs = 0;
    for (int32_t c : filter.Coefficients()) { sum += c; sabs += c < 0 ? -(int64_t)c : c; }
    TEST(sum > (1ll << 28) - 256 && sum < (1ll << 28) + 256 && sabs < (1ll << 30));
    TEST_THROWS(DsdPcmFilter(f, kDsdRate, 96000), AssertionFailed);                  // not a whole decimation
    TEST_THROWS(DsdPcmFilter(f, kDsdRate, kPcmRate, 12), AssertionFailed);
    TEST_THROWS(DsdPcmConverter(filter, 6, 4), AssertionFailed);                     // the format's own rule for (W, P)

    Sink sink;
    CodecController controller(f, sink, Jiffies::kPerSecond);
    DsdPcmConverter c(filter, 6, 2);
    DsdPcmConverter::Lane lane = {&c, &controller, 0};
    TUint64 lo = 0, hi = 0;
    TEST(c.ConvertibleFrames() == 0 && !c.Window(lo, hi));
    std::vector<TByte> chunks(6 * 8000, 0x69);
    TEST_THROWS(c.Push(Brn(chunks.data(), 7)), AssertionFailed);                     // whole chunks only
    c.Push(Brn(chunks.data(), 6 * 9));                                               // 144 bits: four frames and half of the fifth
    TEST(c.ConvertibleFrames() == 4 && c.Window(lo, hi) && lo == 0 && hi == 8);
    c.Push(Brn(chunks.data(), 6));
    TEST(c.ConvertibleFrames() == 5 && c.Window(lo, hi) && lo == 0 && hi == 10);     // a stream start holds no chunk before chunk 0

    std::vector<TByte> pcm(6 * 4000, 0);
    DsdPcmConverter::Deliver(lane, pcm.data(), 5);
    TEST(sink.iStreams == 1 && sink.iStreamBeforeAudio && sink.iAudio.size() == 1);
    TEST(sink.iInfo.SampleRate() == kPcmRate && sink.iInfo.BitDepth() == 24 && sink.iInfo.NumChannels() == 2);
    TEST(sink.iInfo.Multiroom() == Multiroom::Allowed && sink.iInfo.Format() == AudioFormat::Pcm && sink.iInfo.BitRate() == kPcmRate * 48);
    TEST(c.FramesOut() == 5 && c.FirstChunkHeld() == 0 && c.ChunksHeld() == 10);     // frame 5 still reads from before the start
    TEST(lane.trackOffset == 5ull * Jiffies::PerSample(kPcmRate));
    TEST(c.ConvertibleFrames() == 0);

    c.Push(Brn(chunks.data(), 6 * 8000));                                            // 8010 chunks: 4005 frames
    TEST(c.ConvertibleFrames() == 4000 && c.Window(lo, hi) && lo == 0 && hi == 8010);
    DsdPcmConverter::Deliver(lane, pcm.data(), 4000);
    TEST(sink.iStreams == 1);                                                        // announced once
    std::vector<TUint> sizes;
    TUint64 jiffies = 0;
    while (!sink.iAudio.empty()) {
        MsgAudioPcm* m = sink.iAudio.front();
        sink.iAudio.pop_front();
        TEST(m->TrackOffset() == jiffies);
        jiffies += m->Jiffies();
        MsgPlayable* p = m->CreatePlayable();
        sizes.push_back(p->Bytes());
        p->RemoveRef();
    }
    TEST(sizes == (std::vector<TUint>{30, 9216, 9216, 4000 * 6 - 2 * 9216}));         // pieces of at most 9216 bytes
    TEST(jiffies == lane.trackOffset && jiffies == 4005ull * Jiffies::PerSample(kPcmRate));
    // frame 4005 reads bits 4006 * 32 - 512 ..: chunk 7980 on; 30 chunks = 480 bits = N - D of history stay
    TEST(c.FramesOut() == 4005 && c.FirstChunkHeld() == 7980 && c.ChunksHeld() == 30);
    c.Push(Brn(chunks.data(), 6 * 2));
    TEST(c.ConvertibleFrames() == 1 && c.Window(lo, hi) && lo == 7980 && hi == 8012);
}

struct Stream {
    TUint W, P;
    size_t firstTick;
    std::vector<TUint> pushes;                                                       // chunks per tick from firstTick on
};

static void Collect(MsgFactory& f, std::vector<std::unique_ptr<Sink>>& aSinks, std::vector<TUint64>& aJiffies, std::vector<std::vector<TByte>>& aGot)
{
    PlayableBatch batch(f);
    std::vector<std::unique_ptr<ProcessorPcmBufTest>> procs;
    std::vector<size_t> laneOf;
    for (size_t k = 0; k < aSinks.size(); k++) {
        while (!aSinks[k]->iAudio.empty()) {
            MsgAudioPcm* m = aSinks[k]->iAudio.front();
            aSinks[k]->iAudio.pop_front();
            aSinks[k]->iAudioSeen++;
            TEST(m->TrackOffset() == aJiffies[k]);
            aJiffies[k] += m->Jiffies();
            MsgPlayable* p = m->CreatePlayable();
            TEST(p->Bytes() <= DecodedAudio::kMaxBytes && p->Bytes() % 6 == 0);
            procs.emplace_back(new ProcessorPcmBufTest());
            laneOf.push_back(k);
            batch.Add(p, *procs.back());
        }
    }
    if (!procs.empty()) batch.Run();
    for (size_t i = 0; i < procs.size(); i++) {
        const Brn b = procs[i]->Buf();
        aGot[laneOf[i]].insert(aGot[laneOf[i]].end(), b.Ptr(), b.Ptr() + b.Bytes());
    }
}

static void TestPipeline(MsgFactory& f)
{
    const std::vector<Stream> streams = {
        {2, 0, 0, {1, 1, 1, 61, 0, 3000, 7}},                                        // a frame is two chunks: some ticks bring half of one
        {6, 2, 0, {4000, 0, 0, 1, 2999, 64, 1}},
        {8, 4, 0, {15, 16, 17, 3073, 0, 2, 900}},                                    // 3073 chunks: a piece and a bit
        {6, 2, 3, {0, 0, 0, 1200, 31, 33, 5}},                                       // joins at tick 3
        {2, 0, 0, {30, 2, 2, 2, 2, 2, 8000}},                                        // the filter fills over several ticks
    };
    DsdPcmFilter filter(f, kDsdRate, kPcmRate);
    TEST(filter.Handle() != nullptr);
    std::mt19937 rng(20261);
    const size_t n = streams.size(), ticks = 7;
    std::vector<std::unique_ptr<DsdPcmConverter>> converters, whole;
    std::vector<std::unique_ptr<Sink>> sinks, wholeSinks;
    std::vector<std::unique_ptr<CodecController>> controllers, wholeControllers;
    std::vector<DsdPcmConverter::Lane> lanes, wholeLanes;
    std::vector<std::vector<TByte>> data(n), got(n), want(n);
    std::vector<TUint64> jiffies(n, 0), wholeJiffies(n, 0);
    for (size_t k = 0; k < n; k++) {
        converters.emplace_back(new DsdPcmConverter(filter, streams[k].W, streams[k].P));
        whole.emplace_back(new DsdPcmConverter(filter, streams[k].W, streams[k].P));
        sinks.emplace_back(new Sink());
        wholeSinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerSecond));
        wholeControllers.emplace_back(new CodecController(f, *wholeSinks[k], Jiffies::kPerSecond));
        wholeLanes.push_back({whole[k].get(), wholeControllers[k].get(), 0});
    }
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d0 = 0, h2d1 = 0, d2h = 0;
    for (size_t t = 0; t < ticks; t++) {
        uint64_t windowBytes = 0;
        bool anything = false;
        for (size_t k = 0; k < n; k++) {
            if (t == streams[k].firstTick) lanes.push_back({converters[k].get(), controllers[k].get(), 0});
            if (t < streams[k].firstTick) continue;
            std::vector<TByte> bytes((size_t)streams[k].pushes[t] * (4 + streams[k].P));
            for (TByte& b : bytes) b = (TByte)rng();                                 // (pad bytes too: nobody may look at them)
            data[k].insert(data[k].end(), bytes.begin(), bytes.end());
            converters[k]->Push(Brn(bytes.data(), (TUint)bytes.size()));
            TUint64 lo = 0, hi = 0;
            if (converters[k]->Window(lo, hi)) { anything = true; windowBytes += ((hi - lo) * (4 + streams[k].P) + 15) & ~15ull; }
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d0, &d2h) == OHGPU_OK);
        DsdPcmConverter::Flush(f, lanes.data(), lanes.size());
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d1, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + (anything ? 1 : 0));                                 // every lane's conversion in one device call
        TEST(h2d1 - h2d0 == windowBytes);                                            // only the windows cross the link
        Collect(f, sinks, jiffies, got);
    }
    for (size_t k = 0; k < n; k++) whole[k]->Push(Brn(data[k].data(), (TUint)data[k].size()));
    DsdPcmConverter::Flush(f, wholeLanes.data(), wholeLanes.size());
    Collect(f, wholeSinks, wholeJiffies, want);
    size_t bytesChecked = 0;
    for (size_t k = 0; k < n; k++) {
        const size_t chunks = data[k].size() / (4 + streams[k].P);
        TEST(want[k].size() == chunks / 2 * 6 && !want[k].empty());
        TEST(got[k].size() == want[k].size());
        TEST(got[k] == want[k]);
        if (got[k] != want[k]) {
            for (size_t i = 0; i < std::min(got[k].size(), want[k].size()); i++)
                if (got[k][i] != want[k][i]) { printf("lane %zu: first difference at byte %zu: %02x != %02x\n", k, i, got[k][i], want[k][i]); break; }
        }
        TEST(sinks[k]->iStreams == 1 && sinks[k]->iStreamBeforeAudio && sinks[k]->iInfo.SampleRate() == kPcmRate);
        TEST(jiffies[k] == wholeJiffies[k] && converters[k]->FramesOut() == chunks / 2 && converters[k]->ChunksHeld() <= 31);
        bytesChecked += want[k].size();
    }
    for (size_t k = 0; k < lanes.size(); k++) TEST(lanes[k].trackOffset == (TUint64)lanes[k].converter->FramesOut() * Jiffies::PerSample(kPcmRate));
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", n, ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
    {
        MsgFactory control(-1);
        TestBookkeeping(control);
    }
    printf("cpu: %d checks\n", gChecks);
    if (gpu) {
        MsgFactory f(0);
        TestPipeline(f);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
