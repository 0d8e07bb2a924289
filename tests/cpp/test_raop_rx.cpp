// test_raop_rx.cpp -- RaopReceiver (host/RaopReceiver.h) for tests/test_raop_rx_host_cpp.py.
//   test_raop_rx cpu          the element's own logic with a mock clock, sink and observer; csrc/raop_rx_core.h, built for the CPU, stands
//                             in for the device between Collect and Apply: the wire packet, the 10 / 30 ms schedule, the requeue,
//                             DropAudio, SendFlush
//   test_raop_rx gpu STEM     one lane through RaopReceiver::Tick: STEM.fmtp, .secret (key, IV), .datagrams, .sizes, .ports, .ticks
//                             (datagrams a tick), .want (the PCM, packed big-endian) -- one fused device call a tick
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/csrc/raop_rx_core.h"
#include "../../ohpipeline_amd/host/Msg.h"
#include "../../ohpipeline_amd/host/RaopReceiver.h"

using namespace OpenHome;
using namespace OpenHome::Media;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)

static Brn Text(const char* aText) { return Brn((const TByte*)aText, (TUint)strlen(aText)); }
static const char* kFmtp = "96 352 0 16 40 10 14 2 255 0 0 44100";
static const uint32_t kSsrc = 0x1234abcd;

struct MockSink : IRaopResendSink {
    std::vector<std::pair<TUint, TUint>> asked;
    void RequestResend(TUint aSeqStart, TUint aCount) override { asked.push_back({aSeqStart, aCount}); }
};
struct MockObserver : IRaopReceiverObserver {
    TUint streams = 0, delays = 0, lastDelay = 0, stops = 0, lastStop = 0;
    void NotifyNewStream() override { streams++; }
    void NotifyDelay(TUint aLatency) override { delays++; lastDelay = aLatency; }
    void NotifyDiscontinuity(TUint aReason) override { stops++; lastStop = aReason; }
};

static std::vector<TByte> Audio(TUint aSeq, bool aResend = false)
{
    std::vector<TByte> g;
    if (aResend) { const TByte outer[4] = {0x80, 0xd6, 0, 1}; g.insert(g.end(), outer, outer + 4); }
    const TUint ts = aSeq * 352;
    const TByte head[12] = {0x80, 0x60, (TByte)(aSeq >> 8), (TByte)aSeq, (TByte)(ts >> 24), (TByte)(ts >> 16), (TByte)(ts >> 8), (TByte)ts,
                            (TByte)(kSsrc >> 24), (TByte)(kSsrc >> 16), (TByte)(kSsrc >> 8), (TByte)kSsrc};
    g.insert(g.end(), head, head + 12);
    g.push_back((TByte)aSeq);
    return g;
}
static std::vector<TByte> Sync(TUint aLatency)
{
    const TUint now = 100000, before = now - aLatency;
    const TByte g[20] = {0x80, 0xd4, 0, 7, (TByte)(before >> 24), (TByte)(before >> 16), (TByte)(before >> 8), (TByte)before, 0, 0, 0, 0, 0, 0, 0, 0,
                         (TByte)(now >> 24), (TByte)(now >> 16), (TByte)(now >> 8), (TByte)now};
    return std::vector<TByte>(g, g + 20);
}

// What the device does between Collect and Apply, on the CPU: the core's parse and serial sequencer over the receiver's queue
static raoprx::StreamResult StandIn(RaopReceiver& r, TUint64 aNowMs)
{
    ohgpu_raop_rx_stream s;
    std::vector<ohgpu_raop_rx_datagram> grams;
    r.Collect(0, s, grams);
    std::vector<raoprx::Record> recs(grams.size() + 1);
    std::vector<raoprx::Key> keys(grams.size() + 1);
    for (size_t k = 0; k < grams.size(); k++) raoprx::parse(r.PendingArena().data() + grams[k].src_offset, grams[k].bytes, grams[k].port, &recs[k], &keys[k]);
    uint64_t slots[raoprx::kSlots];
    raoprx::StreamResult out;
    raoprx::Stream cs;
    memcpy(&cs, &s, sizeof(cs));
    raoprx::sequence(cs, keys.data(), recs.data(), slots, &out);
    ohgpu_raop_rx_stream_result res;
    memcpy(&res, &out, sizeof(res));
    r.Apply(aNowMs, res, (const ohgpu_raop_rx_record*)recs.data());
    return out;
}

static void TestElement()
{
    TByte key[16], iv[16];
    for (int k = 0; k < 16; k++) { key[k] = (TByte)k; iv[k] = (TByte)(0xf0 + k); }
    TByte wire[RaopReceiver::kResendRequestBytes];
    RaopReceiver::WriteResendRequest(0xfffe, 3, wire);
    const TByte want[8] = {0x80, 0xd5, 0x00, 0x01, 0xff, 0xfe, 0x00, 0x03};
    TEST(memcmp(wire, want, 8) == 0);

    MockSink sink;
    MockObserver obs;
    RaopReceiver r(&sink, &obs, 5);
    r.SetSession(Text(kFmtp), Brn(key, 16), Brn(iv, 16));
    auto audio = [&](TUint seq, bool resend = false) { const std::vector<TByte> g = Audio(seq, resend); if (resend) r.PushControl(Brn(g.data(), (TUint)g.size())); else r.PushAudio(Brn(g.data(), (TUint)g.size())); };
    { const std::vector<TByte> g = Sync(11025); r.PushControl(Brn(g.data(), (TUint)g.size())); }
    audio(10); audio(11); audio(13); audio(14);                       // 12 is missing
    TEST(r.PendingDatagrams() == 5);
    raoprx::StreamResult res = StandIn(r, 1000);
    TEST(res.n_output == 2 && res.n_pending == 2 && r.PendingDatagrams() == 2 && r.WaitingFrames() == 2 && r.Repairing());
    TEST(obs.streams == 1 && obs.delays == 1 && obs.lastDelay == 11025 && obs.stops == 0);
    TEST(sink.asked.empty());                                         // the repair is 0 ms old
    audio(15);
    res = StandIn(r, 1009);                                           // the two that waited are replayed in front of 15
    TEST(res.n_pending == 3 && r.WaitingFrames() == 3 && sink.asked.empty());
    res = StandIn(r, 1010);                                           // kInitialRepairTimeoutMs
    TEST(sink.asked.size() == 1 && sink.asked[0].first == 12 && sink.asked[0].second == 1);
    res = StandIn(r, 1039);
    TEST(sink.asked.size() == 1);
    audio(17);
    res = StandIn(r, 1040);                                           // kSubsequentRepairTimeoutMs later: both gaps
    TEST(sink.asked.size() == 3 && sink.asked[1].first == 12 && sink.asked[1].second == 1 && sink.asked[2].first == 16 && sink.asked[2].second == 1);
    audio(12, true);
    res = StandIn(r, 1041);
    TEST(res.n_output == 4 && res.n_pending == 1 && res.state_out.frame == 15 && r.PacketsOutput() == 6 && r.Repairing());
    audio(16, true);
    res = StandIn(r, 1042);
    TEST(res.n_output == 2 && res.n_pending == 0 && !r.Repairing() && r.PendingDatagrams() == 0 && r.State().frame == 17);
    // a new repair starts its own 10 ms
    audio(20);
    res = StandIn(r, 2000);
    TEST(r.Repairing() && sink.asked.size() == 3);
    res = StandIn(r, 2010);
    TEST(sink.asked.size() == 4 && sink.asked[3].first == 18 && sink.asked[3].second == 2);
    // DropAudio: what waits is forgotten, what came since stays, the next frame starts the count
    audio(30);
    TEST(r.PendingDatagrams() == 2 && r.WaitingFrames() == 1);
    r.DropAudio();
    TEST(r.PendingDatagrams() == 1 && r.WaitingFrames() == 0 && !r.Repairing() && r.State().running == 0);
    res = StandIn(r, 2020);
    TEST(res.n_output == 1 && res.state_out.frame == 30 && res.state_out.running == 1);
    // a restart stops the stream; SendFlush then drops what lies inside the window until the stream resumes
    audio(30);
    audio(31);
    res = StandIn(r, 2030);
    TEST(res.stop_reason == OHGPU_RAOP_RX_STOP_RESTARTED && obs.stops == 1 && obs.lastStop == OHGPU_RAOP_RX_STOP_RESTARTED && r.PendingDatagrams() == 0);
    TEST(r.State().resume_pending == 1 && r.State().running == 0);
    r.SendFlush(41, 41 * 352);
    TEST(r.State().flush_seq == 41 && r.State().flush_time == 41 * 352);
    audio(40); audio(41); audio(42); audio(43);
    res = StandIn(r, 2040);
    TEST(res.n_output == 2 && res.state_out.frame == 43 && res.state_out.resume_pending == 0 && res.state_out.flush_seq == 0 && obs.streams == 2 && obs.delays == 1);
    // a new session starts from nothing
    r.SetSession(Text(kFmtp), Brn(key, 16), Brn(iv, 16));
    TEST(r.State().started == 0 && r.State().session_id == 0 && r.PendingDatagrams() == 0);
}

class Sink : public IPipelineElementDownstream {
public:
    void Push(Msg* aMsg) override
    {
        if (KindOf(aMsg) == MsgKind::AudioPcm) { iAudio.push_back(static_cast<MsgAudioPcm*>(aMsg)); return; }
        aMsg->RemoveRef();
    }
    std::deque<MsgAudioPcm*> iAudio;
};

static std::vector<TByte> ReadFile(const std::string& aPath)
{
    std::ifstream in(aPath, std::ios::binary);
    return std::vector<TByte>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
static std::vector<TUint> ReadNumbers(const std::string& aPath)
{
    std::vector<TUint> out;
    std::ifstream in(aPath);
    for (TUint v; in >> v; ) out.push_back(v);
    return out;
}

static void TestTick(MsgFactory& f, const std::string& aStem)
{
    const std::vector<TByte> fmtp = ReadFile(aStem + ".fmtp"), secret = ReadFile(aStem + ".secret"), grams = ReadFile(aStem + ".datagrams"), want = ReadFile(aStem + ".want");
    const std::vector<TUint> sizes = ReadNumbers(aStem + ".sizes"), ports = ReadNumbers(aStem + ".ports"), ticks = ReadNumbers(aStem + ".ticks");
    TEST(secret.size() == 32 && sizes.size() == ports.size());
    MockSink sink;
    MockObserver obs;
    RaopReceiver r(&sink, &obs, 5);
    r.SetSession(Brn(fmtp.data(), (TUint)fmtp.size()), Brn(secret.data(), 16), Brn(secret.data() + 16, 16));
    Sink down;
    CodecController controller(f, down, Jiffies::kPerSecond);
    RaopReceiver::Lane lane = {&r, &controller, 0};
    PlayableBatch batch(f);
    std::vector<TByte> got;
    size_t next = 0, at = 0;
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    for (size_t t = 0; t < ticks.size(); t++) {
        for (TUint k = 0; k < ticks[t]; k++, next++) {
            const Brn g(grams.data() + at, sizes[next]);
            if (ports[next]) r.PushControl(g); else r.PushAudio(g);
            at += sizes[next];
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        RaopReceiver::Tick(1000 + 10 * t, f, &lane, 1);
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 - calls0 <= 1);                                   // the receiver, the cipher and the decoder in one fused call
        std::vector<std::unique_ptr<ProcessorPcmBufTest>> procs;
        while (!down.iAudio.empty()) {
            MsgAudioPcm* m = down.iAudio.front();
            down.iAudio.pop_front();
            procs.emplace_back(new ProcessorPcmBufTest());
            batch.Add(m->CreatePlayable(), *procs.back());
        }
        if (!procs.empty()) batch.Run();
        for (auto& p : procs) { const Brn b = p->Buf(); got.insert(got.end(), b.Ptr(), b.Ptr() + b.Bytes()); }
    }
    TEST(next == sizes.size() && r.PendingDatagrams() == 0 && !r.Repairing());
    TEST(got.size() == want.size());
    TEST(got == want);
    TEST(obs.streams == 1 && obs.stops == 0 && sink.asked.size() >= 1);
    printf("tick: %zu ticks, %zu bytes byte-exact, %zu resend requests\n", ticks.size(), got.size(), sink.asked.size());
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: test_raop_rx cpu | gpu stem\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    TestElement();
    printf("cpu: %d checks\n", gChecks);
    if (gpu && argc > 2) {
        MsgFactory f(0);
        TestTick(f, argv[2]);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
