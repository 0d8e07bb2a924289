// test_pull.cpp -- tests of PullableSampleRateConverter (ohpipeline_amd/host), the pulled resampler's element.
// `test_pull cpu` runs the control-plane checks on a factory without a device: how many outputs a message makes under changing
// pulls, MaxPull clamping, positions carried through Split / SetRamp / MsgPlayable::Split, streams already at the output rate.
// `test_pull gpu` also runs 64 lanes for 200 ticks through PlayableBatch and checks every byte against a restatement of the
// specification in this file, the device allocations and the number of device calls per tick.
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <random>
#include <thread>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/Msg.h"
#include "../../ohpipeline_amd/host/PullableSampleRateConverter.h"

using namespace OpenHome;
using namespace OpenHome::Media;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)

// ---- a lane: this suite is the upstream element; its input is random S24LE audio kept as S24 values for the restatement ----
class Lane : public IPipelineElementUpstream {
public:
    Lane(MsgFactory& aFactory, TUint aRate, TUint aChannels, uint32_t aSeed)
        : iFactory(aFactory), iRate(aRate), iChannels(aChannels), iRng(aSeed), iSrc(aFactory, *this, 48000) {}
    Msg* Pull() override { Msg* m = iQueue.front(); iQueue.pop_front(); return m; }
    void Start()
    {
        DecodedStreamInfo info;
        info.iSampleRate = iRate;
        info.iBitDepth = 24;
        info.iNumChannels = iChannels;
        info.iBitRate = iRate * 24 * iChannels;
        iQueue.push_back(iFactory.CreateMsgDecodedStream(info));
        Msg* m = iSrc.Pull();
        TEST(KindOf(m) == MsgKind::DecodedStream);
        TEST(static_cast<MsgDecodedStream*>(m)->StreamInfo().SampleRate() == 48000);
        TEST(static_cast<MsgDecodedStream*>(m)->StreamInfo().BitDepth() == 24);
        m->RemoveRef();
    }
    /** Feeds aFrames of input and pulls the element once: the message it emits. */
    MsgAudioPcm* Feed(TUint aFrames)
    {
        std::vector<TByte> bytes(aFrames * iChannels * 3);
        std::uniform_int_distribution<int32_t> d(-(1 << 23), (1 << 23) - 1);
        for (TUint i = 0; i < aFrames * iChannels; i++) {
            const int32_t v = d(iRng);
            iHistory.push_back(v);
            bytes[3 * i] = (TByte)v; bytes[3 * i + 1] = (TByte)(v >> 8); bytes[3 * i + 2] = (TByte)(v >> 16);
        }
        iQueue.push_back(iFactory.CreateMsgAudioPcm(Brn(bytes.data(), (TUint)bytes.size()), iChannels, iRate, 24, AudioDataEndian::Little,
                                                    iFed * Jiffies::PerSample(iRate)));
        iFed += aFrames;
        Msg* m = iSrc.Pull();
        TEST(KindOf(m) == MsgKind::AudioPcm);
        return static_cast<MsgAudioPcm*>(m);
    }
    PullableSampleRateConverter& Src() { return iSrc; }
    const std::vector<int32_t>& History() const { return iHistory; }
    TUint Channels() const { return iChannels; }
    TUint Rate() const { return iRate; }
    TUint64 Fed() const { return iFed; }
private:
    MsgFactory& iFactory;
    const TUint iRate, iChannels;
    std::mt19937 iRng;
    PullableSampleRateConverter iSrc;
    std::deque<Msg*> iQueue;
    std::vector<int32_t> iHistory;
    TUint64 iFed = 0;
};

// ---- the specification, restated: one output message's S24 big-endian bytes ----
static std::vector<TByte> Restate(const PullFilter& aFilter, const std::vector<int32_t>& aX, TUint aCh, TUint64 aPos, TUint aFrac,
                                  TUint64 aStep, TUint aFrames)
{
    const TUint T = aFilter.T, s = aFilter.phasesLog2;
    const int32_t* C = aFilter.table.data();
    std::vector<TByte> out;
    for (TUint j = 0; j < aFrames; j++) {
        const TUint64 u = aFrac + (TUint64)j * aStep;
        const int64_t n = (int64_t)(aPos + (u >> 32));
        const uint32_t f = (uint32_t)u;
        const uint32_t p = f >> (32 - s), w = (f >> (16 - s)) & 0xffffu;
        for (TUint c = 0; c < aCh; c++) {
            int64_t acc = 0;
            for (TUint k = 0; k < T; k++) {
                const int64_t c0 = C[p * T + k], c1 = C[(p + 1) * T + k];
                const int64_t ck = c0 + (((c1 - c0) * (int64_t)w) >> 16);
                const int64_t idx = n - (int64_t)k;
                acc += ck * (idx >= 0 ? (int64_t)aX[(size_t)idx * aCh + c] : 0);
            }
            int64_t y = (acc + (1 << 27)) >> 28;
            y = y > 8388607 ? 8388607 : (y < -8388608 ? -8388608 : y);
            out.push_back((TByte)(y >> 16)); out.push_back((TByte)(y >> 8)); out.push_back((TByte)y);
        }
    }
    return out;
}

static TUint64 Outputs(TUint64 aHave, TUint64 aPos, TUint aFrac, TUint64 aStep)
{
    if (aHave <= aPos) return 0;
    return ((((aHave - 1 - aPos) << 32) + (0xffffffffull - aFrac)) / aStep) + 1;
}

// ------------------------------------------------------------------------------------------- control plane
static void SuiteEmissionAndClamping(MsgFactory& f)
{
    for (TUint rate : {44100u, 48000u}) {                                  // 48 -> 48 kHz is converted too: the common drift case
        Lane lane(f, rate, 2, rate);
        PullableSampleRateConverter& src = lane.Src();
        TEST(src.MaxPull() == (TUint)(0.001 * 2147483648.0 + 0.5));
        src.PullClock(IPullableClock::kNominalFreq + 10 * src.MaxPull());
        TEST(src.Multiplier() == IPullableClock::kNominalFreq + src.MaxPull());
        src.PullClock(0);
        TEST(src.Multiplier() == IPullableClock::kNominalFreq - src.MaxPull());
        src.PullClock(IPullableClock::kNominalFreq + 1234);
        TEST(src.Multiplier() == IPullableClock::kNominalFreq + 1234);
        lane.Start();
        std::mt19937 rng(5);
        TUint64 pos = 0, outTotal = 0;
        TUint frac = 0;
        for (int m = 0; m < 300; m++) {
            if (m % 7 == 0) {                                             // a pull change takes effect at the next message
                std::thread t([&] { src.PullClock(IPullableClock::kNominalFreq - src.MaxPull() + (TUint)(rng() % (2 * src.MaxPull() + 1))); });
                t.join();
            }
            const TUint mult = src.Multiplier();
            uint64_t step = 0;
            TEST(ohgpu_src_pull_step(rate, 48000, mult, &step) == OHGPU_OK);
            const TUint frames = 3 + rng() % 500;                        // (three frames always complete an output at these ratios)
            const TUint64 want = Outputs(lane.Fed() + frames, pos, frac, step);
            TEST(want > 0);
            MsgAudioPcm* msg = lane.Feed(frames);
            TEST(msg->Jiffies() == want * Jiffies::PerSample(48000));
            TEST(msg->TrackOffset() == outTotal * Jiffies::PerSample(48000));
            MsgPlayable* p = msg->CreatePlayable();
            const PlayableWork& w = p->Work();
            TEST(w.pulled && !w.resampled && w.frames == want && w.pullStep == step && w.pullPosFrame == pos && w.pullPosFrac == frac);
            p->RemoveRef();
            PullAdvance(pos, frac, step, want);
            outTotal += want;
        }
        // the outputs follow the input at the ratio the pulls asked for: within the pulls' range of it
        const double ratio = (double)outTotal / (double)lane.Fed() * rate / 48000.0;
        TEST(ratio > 1.0 - 0.0011 && ratio < 1.0 + 0.0011);
    }
}

static void SuitePositionsThroughSplitAndRamp(MsgFactory& f)
{
    Lane lane(f, 44100, 2, 3);
    lane.Src().PullClock(IPullableClock::kNominalFreq + 777);
    lane.Start();
    lane.Feed(1500)->CreatePlayable()->RemoveRef();                   // (a DecodedAudio holds up to 9216 bytes)
    MsgAudioPcm* msg = lane.Feed(441);
    MsgPlayable* whole = static_cast<MsgAudioPcm*>(msg->Clone())->CreatePlayable();
    const PlayableWork w0 = whole->Work();
    const TUint jps = Jiffies::PerSample(48000);
    // Split: the remainder's first output is at pos + k * step
    MsgAudio* tail = msg->Split(100 * jps);
    MsgPlayable* head = msg->CreatePlayable();
    MsgPlayable* rest = static_cast<MsgAudioPcm*>(tail)->CreatePlayable();
    TUint64 pos = w0.pullPosFrame;
    TUint frac = w0.pullPosFrac;
    TEST(head->Work().pullPosFrame == pos && head->Work().pullPosFrac == frac && head->Work().frames == 100);
    PullAdvance(pos, frac, w0.pullStep, 100);
    TEST(rest->Work().pullPosFrame == pos && rest->Work().pullPosFrac == frac && rest->Work().frames == w0.frames - 100);
    TEST(rest->Work().pullStep == w0.pullStep);
    // MsgPlayable::Split: the same identity on the driver's side
    MsgPlayable* rest2 = rest->Split(37 * 6);
    PullAdvance(pos, frac, w0.pullStep, 37);
    TEST(rest2 != nullptr && rest2->Work().pullPosFrame == pos && rest2->Work().pullPosFrac == frac);
    // SetRamp that splits where two ramps cross: both parts keep their positions
    MsgAudioPcm* m2 = lane.Feed(441);
    MsgPlayable* p2 = static_cast<MsgAudioPcm*>(m2->Clone())->CreatePlayable();
    const PlayableWork w2 = p2->Work();
    MsgAudio* tail2 = m2->Split(200 * jps);                           // (a ramp never runs past its message: split, then ramp)
    TUint remaining = 200 * jps;
    MsgAudio* split = nullptr;
    m2->SetRamp(Ramp::kMax, remaining, Ramp::EDown, split);
    TUint remaining2 = m2->Jiffies() * 4;
    MsgAudio* split2 = nullptr;
    m2->SetRamp(Ramp::kMin, remaining2, Ramp::EUp, split2);            // the rising line crosses the falling one: m2 splits there
    TEST(split2 != nullptr);
    MsgAudio* parts[] = {m2, split2, split, tail2};                    // (in stream order)
    TUint64 frames = 0;
    for (MsgAudio* part : parts) {
        if (part == nullptr) continue;
        MsgPlayable* pp = static_cast<MsgAudioPcm*>(part)->CreatePlayable();
        TUint64 ppos = w2.pullPosFrame;
        TUint pfrac = w2.pullPosFrac;
        PullAdvance(ppos, pfrac, w2.pullStep, frames);
        TEST(pp->Work().pullPosFrame == ppos && pp->Work().pullPosFrac == pfrac);
        frames += pp->Work().frames;
        pp->RemoveRef();
    }
    TEST(frames == w2.frames);
    for (MsgPlayable* p : {whole, head, rest, rest2, p2}) p->RemoveRef();
}

class Sink : public IPcmProcessor {
public:
    void BeginBlock() override { iBuf.clear(); }
    void ProcessFragment(const Brx& aData, TUint, TUint) override { iBuf.insert(iBuf.end(), aData.Ptr(), aData.Ptr() + aData.Bytes()); }
    void ProcessSilence(const Brx& aData, TUint, TUint) override { iBuf.insert(iBuf.end(), aData.Ptr(), aData.Ptr() + aData.Bytes()); }
    void EndBlock() override {}
    void Flush() override {}
    std::vector<TByte> iBuf;
};

// Every rate the pipeline accepts is converted: below 24 kHz the default 20 kHz pass band would meet the stop band, so the design is
// chosen per stream (PullableSampleRateConverter::StreamDesign).  With a device, each lane's output is read and restated too.
static void SuiteEveryRateConverts(MsgFactory& f, TBool aRead)
{
    TUint taps = 0;
    double pass = 0.0;
    PullableSampleRateConverter::StreamDesign(44100, 48000, 0, 20000.0, 0.001, taps, pass);
    TEST(taps == 32 && pass == 20000.0);                               // the common cases keep T = 32 and the whole 20 kHz
    PullableSampleRateConverter::StreamDesign(48000, 48000, 0, 20000.0, 0.001, taps, pass);
    TEST(taps == 32 && pass == 20000.0);
    PullableSampleRateConverter::StreamDesign(22050, 48000, 0, 20000.0, 0.001, taps, pass);
    TEST(taps == 64 && pass == 10000.0);                               // 20 kHz of 44.1 kHz, scaled to the narrower rate
    PullableSampleRateConverter::StreamDesign(96000, 48000, 0, 20000.0, 0.001, taps, pass);
    TEST(taps == 64 && pass < 20000.0 && pass > 19000.0);              // downsampling: T = 64, the pass edge a shade lower
    for (TUint rate : {8000u, 11025u, 16000u, 22050u, 24000u, 32000u, 88200u, 96000u, 176400u, 192000u}) {
        Lane lane(f, rate, 2, rate + 1);
        lane.Src().PullClock(IPullableClock::kNominalFreq + 777);
        lane.Start();
        TUint64 pos = 0;
        TUint frac = 0;
        PlayableBatch batch(f);
        std::vector<Sink> sinks(3);
        std::vector<PlayableWork> works;
        for (TUint m = 0; m < 3; m++) {
            uint64_t step = 0;
            TEST(ohgpu_src_pull_step(rate, 48000, IPullableClock::kNominalFreq + 777, &step) == OHGPU_OK);
            const TUint64 want = Outputs(lane.Fed() + 1000, pos, frac, step);
            MsgAudioPcm* msg = lane.Feed(1000);                           // (does not throw: a design exists for the rate)
            MsgPlayable* p = msg->CreatePlayable();
            const PlayableWork& w = p->Work();
            TEST(w.pulled && w.frames == want && w.pullPosFrame == pos && w.pullPosFrac == frac);
            works.push_back(w);
            PullAdvance(pos, frac, step, want);
            if (aRead) batch.Add(p, sinks[m]);
            else p->RemoveRef();
        }
        if (aRead) {
            batch.Run();
            for (TUint m = 0; m < 3; m++) {
                const PlayableWork& w = works[m];
                TEST(sinks[m].iBuf == Restate(w.pullStream->Filter(), lane.History(), 2, w.pullPosFrame, w.pullPosFrac, w.pullStep, w.frames));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------- through the device
static void SuiteManyPulledLanesGpu(MsgFactory& f)
{
    const TUint kLanes = 64, kTicks = 200;
    std::vector<std::unique_ptr<Lane>> lanes;
    for (TUint l = 0; l < kLanes; l++) {
        lanes.emplace_back(new Lane(f, l % 2 ? 48000 : 44100, 1 + l % 3, 100 + l));     // two filters, 1-3 channels
        lanes.back()->Start();
    }
    std::vector<Sink> sinks(kLanes);
    std::mt19937 rng(17);
    PlayableBatch batch(f);
    uint64_t allocs2 = 0, calls0 = 0, src0 = 0, h2d = 0, d2h = 0;
    TUint64 checked = 0;
    for (TUint t = 0; t < kTicks; t++) {
        if (t % 3 == 0)
            for (auto& lane : lanes) lane->Src().PullClock(IPullableClock::kNominalFreq - 3 * lane->Src().MaxPull() / 2 + rng() % (3 * lane->Src().MaxPull()));
        std::vector<PlayableWork> works(kLanes);
        for (TUint l = 0; l < kLanes; l++) {
            Lane& lane = *lanes[l];
            const TUint frames = lane.Rate() == 48000 ? 240 : 220 + (t % 2);        // a 5 ms period of input
            MsgPlayable* p = lane.Feed(frames)->CreatePlayable();
            works[l] = p->Work();
            batch.Add(p, sinks[l]);
        }
        ohgpu_host_transfer_stats(f.Gpu(), &calls0, &src0, &h2d, &d2h);
        batch.Run();
        uint64_t calls1 = 0, src1 = 0;
        ohgpu_host_transfer_stats(f.Gpu(), &calls1, &src1, &h2d, &d2h);
        TEST(src1 - src0 == 2 && calls1 - calls0 == 2);                   // one pulled device call per filter per tick
        if (t == 1) ohgpu_device_allocations(f.Gpu(), &allocs2);
        for (TUint l = 0; l < kLanes; l++) {
            const PlayableWork& w = works[l];
            const std::vector<TByte> want = Restate(w.pullStream->Filter(), lanes[l]->History(), lanes[l]->Channels(), w.pullPosFrame,
                                                    w.pullPosFrac, w.pullStep, w.frames);
            TEST(sinks[l].iBuf == want);
            checked += w.frames;
        }
    }
    uint64_t allocs = 0;
    ohgpu_device_allocations(f.Gpu(), &allocs);
    TEST(allocs == allocs2);                                               // flat after the second tick
    TEST(checked > (TUint64)kLanes * kTicks * 200);
    printf("gpu: %u lanes x %u ticks, %llu pulled output frames bit-exact\n", kLanes, kTicks, (unsigned long long)checked);
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
    try {
        MsgFactory control(-1);
        SuiteEmissionAndClamping(control);
        SuitePositionsThroughSplitAndRamp(control);
        SuiteEveryRateConverts(control, false);
        if (gpu) {
            MsgFactory f(0);
            SuiteEmissionAndClamping(f);
            SuiteEveryRateConverts(f, true);
            SuiteManyPulledLanesGpu(f);
        }
    }
    catch (const std::exception& e) {
        printf("UNEXPECTED EXCEPTION %s\n", e.what());
        gFailures++;
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
