// test_dsd.cpp -- DSD in the host adapter (ohpipeline_amd/host: MsgAudioDsd, DSD silence, the DSD playables, IDsdProcessor,
// CodecController::OutputAudioDsd, DsdPacker).
// `test_dsd cpu` runs what needs no device on a control-plane-only factory: the reference's own suite for DSD messages
// (SuiteMsgAudioDsd, OpenHome/Media/Tests/TestMsg.cpp:1767-1960) restated in this repository's words -- rates and jiffies, split,
// clone, the asserts, the split off a block boundary that leaves 0 and 24 bytes, the members of both halves of a split at (1, 0)
// and at (6, 2), Jiffies::ToBytesSampleBlock, playable to total jiffies -- and the packer's bookkeeping.
// `test_dsd gpu` adds the parts of that suite that read audio (0xde through a playable, silence and muted audio as 0x69) and the
// whole path, byte for byte against expectations computed here: packer -> OutputAudioDsd -> CreatePlayable -> PlayableBatch ->
// ProcessorDsdBufTest, five lanes over several ticks, one lane ending inside a sample block and one muted.
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <random>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/DsdPacker.h"
#include "../../ohpipeline_amd/host/Msg.h"

using namespace OpenHome;
using namespace OpenHome::Media;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)
#define TEST_THROWS(expr, Exc) do { bool thrown_ = false; try { expr; } catch (Exc&) { thrown_ = true; } gChecks++; \
    if (!thrown_) { gFailures++; printf("FAILED %s:%d  %s did not throw\n", __FILE__, __LINE__, #expr); } } while (0)

static const TUint kRate = 2822400;
static const TByte kDsdSilence = 0x69;

// ---------------------------------------------------------------- the message algebra (no device)
static void TestMessages(MsgFactory& f)
{
    std::vector<TByte> data(1200, 0xde);
    const Brn buf(data.data(), (TUint)data.size());
    const TUint jps = Jiffies::PerSample(kRate);

    // the same bytes last longer at a lower rate
    TUint prev = 0xffffffff;
    for (TUint rate : {2822400u, 5644800u, 11289600u}) {
        MsgAudioDsd* m = f.CreateMsgAudioDsd(buf, 2, rate, 2, 0, 0);
        TEST(m->Jiffies() < prev);
        TEST(m->Jiffies() == 1200u * 8 / 2 * Jiffies::PerSample(rate));
        prev = m->Jiffies();
        m->RemoveRef();
    }

    // split: the parts add up, the track offset runs on
    MsgAudioDsd* msg = f.CreateMsgAudioDsd(buf, 2, kRate, 2, Jiffies::kPerSecond, 0);
    const TUint whole = msg->Jiffies();
    MsgAudio* rest = msg->Split(800);
    TEST(rest != nullptr);
    TEST(msg->Jiffies() == 800 && rest->Jiffies() == whole - 800);
    TEST(msg->Jiffies() > 0 && rest->Jiffies() > 0 && msg->Jiffies() < whole && rest->Jiffies() < whole);
    TEST(msg->TrackOffset() == Jiffies::kPerSecond);
    TEST(static_cast<MsgAudioDsd*>(rest)->TrackOffset() == msg->TrackOffset() + msg->Jiffies());
    rest->RemoveRef();
    TEST_THROWS(rest = msg->Split(0), AssertionFailed);
    TEST_THROWS(rest = msg->Split(msg->Jiffies()), AssertionFailed);
    TEST_THROWS(rest = msg->Split(msg->Jiffies() + 1), AssertionFailed);

    // clone: same length, same offset, outlives its parent
    MsgAudio* clone = msg->Clone();
    TEST(clone->Jiffies() == msg->Jiffies());
    TEST(static_cast<MsgAudioDsd*>(clone)->TrackOffset() == msg->TrackOffset());
    TEST(static_cast<MsgAudioDsd*>(clone)->SizeTotalJiffies() == msg->SizeTotalJiffies());
    const TUint cloneJiffies = clone->Jiffies();
    msg->RemoveRef();
    TEST(clone->Jiffies() == cloneJiffies);
    clone->RemoveRef();

    TEST_THROWS(f.CreateMsgAudioDsd(Brn(), 2, kRate, 2, 0, 0), AssertionFailed);     // no audio, no message

    // a split that is not on a block boundary: the head holds no whole block, the tail all of them
    TByte data2[24] = {0};
    TUint W = 1;
    TUint blockJiffies = W * 32 / 2 * jps;
    msg = f.CreateMsgAudioDsd(Brn(data2, sizeof data2), 2, kRate, W, 0, 0);
    MsgAudio* tail = msg->Split(blockJiffies - 1);
    MsgPlayable* playable = msg->CreatePlayable();
    TEST(playable->Bytes() == 0);
    playable->RemoveRef();
    playable = static_cast<MsgAudioDsd*>(tail)->CreatePlayable();
    TEST(playable->Bytes() == sizeof data2);
    playable->RemoveRef();

    // both halves of a split know their own sizes: (1, 0) ...
    std::vector<TByte> data3(320, 0);
    const Brn buf3(data3.data(), (TUint)data3.size());
    msg = f.CreateMsgAudioDsd(buf3, 2, kRate, W, Jiffies::kPerSecond, 0);
    MsgAudioDsd* second = static_cast<MsgAudioDsd*>(msg->Split(blockJiffies));
    const TUint allJiffies = 320 * 8 / 2 * jps;
    TEST(second->SampleBlockWords() == W && second->BlockWordsNoPad() == W);
    TEST(msg->Jiffies() == msg->SizeTotalJiffies() && msg->SizeTotalJiffies() == blockJiffies && msg->JiffiesNonPlayable() == 0);
    TEST(second->Jiffies() == second->SizeTotalJiffies() && second->SizeTotalJiffies() == allJiffies - blockJiffies);
    TEST(second->JiffiesNonPlayable() == 0);
    second->RemoveRef();
    msg->RemoveRef();

    // ... and (6, 2): four of six words are audio
    W = 6;
    const TUint P = 2, noPad = 4;
    blockJiffies = W * 32 / 2 * jps;
    const TUint playableBlockJiffies = noPad * 32 / 2 * jps;
    msg = f.CreateMsgAudioDsd(buf3, 2, kRate, W, Jiffies::kPerSecond, P);
    const TUint before = msg->Jiffies();
    TEST(before == 320u * 8 * noPad / W / 2 * jps);
    second = static_cast<MsgAudioDsd*>(msg->Split(blockJiffies));
    TEST(second->SampleBlockWords() == W && second->BlockWordsNoPad() == W - P);
    TUint wholeBlocks = msg->Jiffies() - msg->Jiffies() % playableBlockJiffies;
    TUint total = wholeBlocks * W / noPad;
    TEST(msg->Jiffies() == blockJiffies && msg->SizeTotalJiffies() == total && msg->JiffiesNonPlayable() == total - msg->Jiffies());
    wholeBlocks = second->Jiffies() - second->Jiffies() % playableBlockJiffies;
    total = wholeBlocks * W / noPad;
    TEST(second->Jiffies() == before - blockJiffies);
    TEST(second->SizeTotalJiffies() == total + blockJiffies);
    TEST(second->JiffiesNonPlayable() == total - second->Jiffies() + blockJiffies);
    second->RemoveRef();
    msg->RemoveRef();

    // jiffies to bytes, on and off a block boundary
    const TUint samplesPerBlock = 6 * 32 / 2;
    TUint jiffies = 192000;
    const TUint target = 192000 / jps * 2 / 8;
    TEST(Jiffies::ToBytesSampleBlock(jiffies, jps, 2, 1, samplesPerBlock) == target);
    jiffies = 192000 + jps;
    TEST(Jiffies::ToBytesSampleBlock(jiffies, jps, 2, 1, samplesPerBlock) == target);
    TEST(jiffies == 192000);

    // playable to total jiffies, on and off a block boundary
    const TUint playableBlock = noPad * 32 * jps;
    msg = f.CreateMsgAudioDsd(buf3, 2, kRate, 6, 0, 2);
    TEST(msg->JiffiesPlayableToJiffiesTotal(128000, playableBlock) == 128000u * W / noPad);
    TEST(msg->JiffiesPlayableToJiffiesTotal(128000 + jps, playableBlock) == 128000u * W / noPad);
    msg->RemoveRef();

    // DSD silence: whole blocks, split keeps both parts whole
    jiffies = Jiffies::kPerMs * 3;
    MsgSilence* silence = f.CreateMsgSilenceDsd(jiffies, kRate, 1, 2, 0);
    TEST(silence->Jiffies() == jiffies && jiffies % (2 * 32 * jps) == 0 && silence->SampleBlockWords() == 2);
    MsgAudio* silenceRest = silence->Split(2 * 32 * jps + 7);
    TEST(silence->Jiffies() == 2 * 32 * jps && silenceRest->Jiffies() == jiffies - 2 * 32 * jps);
    playable = silence->CreatePlayable();
    TEST(playable->Bytes() == 8 && playable->Work().silence && playable->Work().Dsd());
    playable->RemoveRef();
    silenceRest->RemoveRef();

    MsgAudioDsd* plain = new MsgAudioDsd();                                         // still default-constructible, still a message
    TEST(KindOf(plain) == MsgKind::AudioDsd && plain->Jiffies() == 0);
    plain->RemoveRef();
}

// ---------------------------------------------------------------- a sink for what the codec side outputs
class Sink : public IPipelineElementDownstream {
public:
    void Push(Msg* aMsg) override
    {
        if (KindOf(aMsg) == MsgKind::AudioDsd) iAudio.push_back(static_cast<MsgAudioDsd*>(aMsg));
        else aMsg->RemoveRef();
    }
    std::deque<MsgAudioDsd*> iAudio;
};

static void TestPackerBookkeeping(MsgFactory& f)
{
    (void)f;
    std::vector<TByte> bytes(20000, 0x55);
    DsdPacker dsf(DsdPacker::EKind::Dsf, 6, 2);
    dsf.Push(Brn(bytes.data(), 8191));
    TEST(dsf.ConvertibleChunks() == 0);                                             // not yet a pair
    dsf.Push(Brn(bytes.data(), 1 + 8192 + 100));
    TEST(dsf.ConvertibleChunks() == 4096);
    dsf.SetStreamChunks(2048 + 1001);                                               // the stream ends inside the second pair
    TEST(dsf.ConvertibleChunks() == 2048);
    dsf.Drain();
    TEST(dsf.ConvertibleChunks() == 2048 + 1001);
    DsdPacker dff(DsdPacker::EKind::Dff, 6, 2);
    dff.Push(Brn(bytes.data(), 4 * 9 + 3));
    TEST(dff.ConvertibleChunks() == 8);                                             // whole blocks of four while the stream runs
    dff.Drain();
    TEST(dff.ConvertibleChunks() == 9);
    DsdPacker raw(DsdPacker::EKind::Raw, 8, 4);
    raw.Push(Brn(bytes.data(), 16 * 3 + 5));
    TEST(raw.ConvertibleChunks() == 12);
    raw.Drain();                                                                    // the last input block is completed on the host
    TEST(raw.ConvertibleChunks() == 16);
    TEST_THROWS(DsdPacker(DsdPacker::EKind::Dff, 6, 4), AssertionFailed);
    TEST_THROWS(DsdPacker(DsdPacker::EKind::Raw, 7, 3), AssertionFailed);
}

// ---------------------------------------------------------------- reading audio (device)
static TByte Reverse(TByte v)
{
    TByte r = 0;
    for (int k = 0; k < 8; k++) if (v & (1 << k)) r |= (TByte)(0x80 >> k);
    return r;
}

/** What a stream's file bytes become, computed here: the chunks, then 0x69 to the end of the last sample block. */
static std::vector<TByte> Expect(DsdPacker::EKind aKind, TUint aW, TUint aP, std::vector<TByte> aFile, TUint64 aStreamChunks)
{
    const TUint perBlock = aW - aP;
    if (aKind == DsdPacker::EKind::Raw) {
        while (aFile.size() % (perBlock * 4) != 0) aFile.push_back(kDsdSilence);
    }
    TUint64 chunks = aKind == DsdPacker::EKind::Dsf ? std::min<TUint64>(aStreamChunks, aFile.size() / 8192 * 2048) : aFile.size() / 4;
    std::vector<TByte> out;
    for (TUint64 j = 0; j < chunks; j++) {
        TByte l0, l1, r0, r1;
        if (aKind == DsdPacker::EKind::Dsf) {
            const TByte* pair = aFile.data() + j / 2048 * 8192;
            const size_t at = (size_t)(j % 2048) * 2;
            l0 = Reverse(pair[at]); l1 = Reverse(pair[at + 1]); r0 = Reverse(pair[4096 + at]); r1 = Reverse(pair[4096 + at + 1]);
        }
        else if (aKind == DsdPacker::EKind::Dff) {
            l0 = aFile[4 * j]; r0 = aFile[4 * j + 1]; l1 = aFile[4 * j + 2]; r1 = aFile[4 * j + 3];
        }
        else {
            l0 = aFile[4 * j]; l1 = aFile[4 * j + 1]; r0 = aFile[4 * j + 2]; r1 = aFile[4 * j + 3];
        }
        out.insert(out.end(), aP / 2, 0); out.push_back(l0); out.push_back(l1);
        out.insert(out.end(), aP / 2, 0); out.push_back(r0); out.push_back(r1);
    }
    while (out.size() % (aW * 4) != 0) out.push_back(kDsdSilence);
    return out;
}

static void TestReads(MsgFactory& f)
{
    std::vector<TByte> data(1200, 0xde);
    const Brn buf(data.data(), (TUint)data.size());
    ProcessorDsdBufTest processor;
    MsgAudioDsd* msg = f.CreateMsgAudioDsd(buf, 2, kRate, 2, 0, 0);
    MsgPlayable* playable = msg->CreatePlayable();
    playable->Read(processor);
    TEST(processor.Buf().Bytes() == 1200 && processor.Fragments().size() == 1);
    for (TUint i = 0; i < processor.Buf().Bytes(); i++) if (processor.Buf()[i] != 0xde) { TEST(processor.Buf()[i] == 0xde); break; }
    playable->RemoveRef();

    TUint jiffies = Jiffies::kPerMs * 3;
    MsgSilence* silence = f.CreateMsgSilenceDsd(jiffies, kRate, 1, 2, 0);
    playable = silence->CreatePlayable();
    playable->Read(processor);
    TEST(processor.Buf().Bytes() == jiffies / Jiffies::PerSample(kRate) / 8 && processor.Buf().Bytes() > 0);
    for (TUint i = 0; i < processor.Buf().Bytes(); i++) if (processor.Buf()[i] != kDsdSilence) { TEST(processor.Buf()[i] == kDsdSilence); break; }
    playable->RemoveRef();

    msg = f.CreateMsgAudioDsd(buf, 2, kRate, 2, 0, 0);                               // muted audio plays silence
    msg->SetMuted();
    playable = msg->CreatePlayable();
    playable->Read(processor);
    TEST(processor.Buf().Bytes() == 1200);
    for (TUint i = 0; i < processor.Buf().Bytes(); i++) if (processor.Buf()[i] != kDsdSilence) { TEST(processor.Buf()[i] == kDsdSilence); break; }
    playable->RemoveRef();

    jiffies = 64 * Jiffies::PerSample(kRate) * 3000;                                 // 24000 bytes of silence: pieces of kMaxBytes
    silence = f.CreateMsgSilenceDsd(jiffies, kRate, 2, 6, 2);
    playable = silence->CreatePlayable();
    TEST(playable->Bytes() == 3000 * 24);
    MsgPlayable* behind = playable->Split(24 * 1000);
    TEST(playable->Bytes() == 24000 && behind->Bytes() == 48000);
    TEST_THROWS(behind->Split(25), AssertionFailed);
    behind->RemoveRef();
    playable->Read(processor);
    TEST(processor.Fragments() == (std::vector<TUint>{9216, 9216, 24000 - 2 * 9216}));
    playable->RemoveRef();

    msg = f.CreateMsgAudioDsd(buf, 2, kRate, 2, 0, 0);                               // a playable of no bytes still reports a block
    MsgAudio* rest = msg->Split(1);
    playable = msg->CreatePlayable();
    playable->Read(processor);
    TEST(processor.Buf().Bytes() == 0 && processor.Fragments().size() == 1);
    playable->RemoveRef();
    rest->RemoveRef();
}

struct Stream {
    DsdPacker::EKind kind;
    TUint W, P;
    TUint64 streamChunks;                                                            // DSF: the header's length
    std::vector<TUint> pushes;                                                       // file bytes per tick
    TBool muted;
};

static void TestPipeline(MsgFactory& f)
{
    const std::vector<Stream> streams = {
        {DsdPacker::EKind::Dsf, 6, 2, 3 * 2048 + 1001, {10000, 10000, 12768}, false},   // ends inside a sample block (7145 = 4 * 1786 + 1)
        {DsdPacker::EKind::Dsf, 2, 0, 2 * 2048, {8192, 0, 8192}, false},
        {DsdPacker::EKind::Dff, 6, 2, 0, {4 * 1000 + 2, 4 * 3001 + 2, 4 * 77 + 1}, false},   // 4078 chunks and a stray byte: ends mid-block
        {DsdPacker::EKind::Raw, 8, 4, 0, {4 * 400, 4 * 401 + 3, 4 * 2500}, false},          // the last input block completed on the host
        {DsdPacker::EKind::Dff, 8, 4, 0, {4 * 640, 4 * 640, 4 * 640}, true},                // muted: plays 0x69 of the same length
    };
    std::mt19937 rng(20260);
    std::vector<std::unique_ptr<DsdPacker>> packers;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<DsdPacker::Lane> lanes;
    std::vector<std::vector<TByte>> files(streams.size()), got(streams.size());
    std::vector<TUint64> jiffiesPlayed(streams.size(), 0);
    for (size_t k = 0; k < streams.size(); k++) {
        packers.emplace_back(new DsdPacker(streams[k].kind, streams[k].W, streams[k].P));
        if (streams[k].kind == DsdPacker::EKind::Dsf) packers[k]->SetStreamChunks(streams[k].streamChunks);
        sinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerMs * 5));
        controllers[k]->OutputDecodedStream(kRate * 2, 1, kRate, 2, Brn((const TByte*)"DSD", 3), 0, 0, true);
        lanes.push_back({packers[k].get(), controllers[k].get(), 2, kRate, 0});
    }
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    PlayableBatch batch(f);
    const size_t ticks = 3;
    for (size_t t = 0; t <= ticks; t++) {                                            // (the tick after the last push drains)
        for (size_t k = 0; k < streams.size(); k++) {
            if (t == ticks) { packers[k]->Drain(); continue; }
            std::vector<TByte> bytes(streams[k].pushes[t]);
            for (TByte& b : bytes) b = (TByte)rng();
            files[k].insert(files[k].end(), bytes.begin(), bytes.end());
            packers[k]->Push(Brn(bytes.data(), (TUint)bytes.size()));
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        DsdPacker::Flush(f, lanes.data(), lanes.size());
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + 1);                                                  // every lane's conversion in one device call
        // the driver's side of the tick: every message a playable, every playable in one batch
        std::vector<std::unique_ptr<ProcessorDsdBufTest>> procs;
        std::vector<size_t> laneOf;
        for (size_t k = 0; k < streams.size(); k++) {
            while (!sinks[k]->iAudio.empty()) {
                MsgAudioDsd* m = sinks[k]->iAudio.front();
                sinks[k]->iAudio.pop_front();
                TEST(m->TrackOffset() == jiffiesPlayed[k]);
                TEST(m->SampleBlockWords() == streams[k].W && m->SizeTotalJiffies() == m->Jiffies() / (streams[k].W - streams[k].P) * streams[k].W);
                jiffiesPlayed[k] += m->Jiffies();
                if (streams[k].muted) m->SetMuted();
                MsgPlayable* p = m->CreatePlayable();
                TEST(p->Bytes() <= DecodedAudio::kMaxBytes && p->Bytes() % (streams[k].W * 4) == 0);
                procs.emplace_back(new ProcessorDsdBufTest());
                laneOf.push_back(k);
                batch.Add(p, *procs.back());
            }
        }
        TEST(!procs.empty());
        batch.Run();
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls0 == calls1 + 1);                                                  // ... and every playable's read in one more
        for (size_t i = 0; i < procs.size(); i++) {
            const Brn b = procs[i]->Buf();
            got[laneOf[i]].insert(got[laneOf[i]].end(), b.Ptr(), b.Ptr() + b.Bytes());
        }
        TEST(lanes[0].trackOffset == jiffiesPlayed[0]);
    }
    size_t bytesChecked = 0;
    for (size_t k = 0; k < streams.size(); k++) {
        std::vector<TByte> want = Expect(streams[k].kind, streams[k].W, streams[k].P, files[k], streams[k].streamChunks);
        if (streams[k].muted) std::fill(want.begin(), want.end(), kDsdSilence);
        TEST(got[k].size() == want.size());
        TEST(got[k] == want);
        if (got[k] != want) {
            for (size_t i = 0; i < std::min(got[k].size(), want.size()); i++)
                if (got[k][i] != want[i]) { printf("lane %zu: first difference at byte %zu: %02x != %02x\n", k, i, got[k][i], want[i]); break; }
        }
        TEST(packers[k]->ConvertibleChunks() == 0);
        TEST(jiffiesPlayed[k] == (TUint64)want.size() / (streams[k].W * 4) * (streams[k].W - streams[k].P) * 32 / 2 * Jiffies::PerSample(kRate));
        bytesChecked += want.size();
    }
    // lane 0 ends inside a block: 7145 chunks of 6 bytes, then 0x69 to the end of block 1787
    TEST(got[0].size() == 1787 * 24 && got[0][7145 * 6] == kDsdSilence && got[0].back() == kDsdSilence);
    printf("pipeline: %zu lanes, %zu bytes byte-exact\n", streams.size(), bytesChecked);
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
    {
        MsgFactory control(-1);
        TestMessages(control);
        TestPackerBookkeeping(control);
    }
    printf("cpu: %d checks\n", gChecks);
    if (gpu) {
        MsgFactory f(0);
        TestMessages(f);
        TestReads(f);
        TestPipeline(f);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
