// test_receiver.cpp -- the Songcast receiver in the host adapter (ohpipeline_amd/host/Receiver.h: OhmReceiver).
//   test_receiver cpu JOB REPORT        the element alone: the device call of a tick is stood in for by csrc/ohm_rx_core.h run on the
//                                       CPU over the tick's tables (OhmReceiver::Collect / FillSource / Deliver around it)
//   test_receiver gpu JOB REPORT BYTES  the same ticks through OhmReceiver::Flush, and every message read through a playable into
//                                       ProcessorPcmBufTest: BYTES gets what reached the processors, lane after lane
// JOB: per lane a line "<stem> <datagrams per tick>"; <stem>.datagrams holds the lane's datagrams back to back, <stem>.sizes their
// sizes; a size of 0 stands for Restart().  REPORT gets one line per thing that happened, in order -- stream, audio, delay, halt,
// stopped, resend, tick -- which tests/test_ohm_rx_host_cpp.py compares with what the model says must happen.
// Both modes first run the queue's bookkeeping checks, which need no device.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/csrc/ohm_rx_core.h"
#include "../../ohpipeline_amd/host/Msg.h"
#include "../../ohpipeline_amd/host/Receiver.h"

using namespace OpenHome;
using namespace OpenHome::Media;
using namespace OpenHome::Av;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)
#define TEST_THROWS(expr, Exc) do { bool thrown_ = false; try { expr; } catch (Exc&) { thrown_ = true; } gChecks++; \
    if (!thrown_) { gFailures++; printf("FAILED %s:%d  %s did not throw\n", __FILE__, __LINE__, #expr); } } while (0)

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

struct Report {
    std::vector<std::string> lines;
    void Add(size_t aLane, const std::string& aText) { std::ostringstream s; s << aLane << " " << aText; lines.push_back(s.str()); }
};

class Sink : public IPipelineElementDownstream, public IOhmReceiverObserver, public IOhmResendSink {
public:
    Sink(Report& aReport, size_t aLane) : iReport(aReport), iLane(aLane) {}
    void Push(Msg* aMsg) override
    {
        std::ostringstream s;
        if (KindOf(aMsg) == MsgKind::AudioPcm) {
            MsgAudioPcm* m = static_cast<MsgAudioPcm*>(aMsg);
            s << "audio " << m->TrackOffset() << " " << m->Jiffies();
            iReport.Add(iLane, s.str());
            iAudio.push_back(m);
            return;
        }
        if (KindOf(aMsg) == MsgKind::DecodedStream) {
            const DecodedStreamInfo& i = static_cast<MsgDecodedStream*>(aMsg)->StreamInfo();
            const Brn codec = i.CodecName();
            s << "stream " << i.BitRate() << " " << i.BitDepth() << " " << i.SampleRate() << " " << i.NumChannels() << " [" << std::string((const char*)codec.Ptr(), codec.Bytes())
              << "] " << i.TrackLength() << " " << i.SampleStart() << " " << (i.Lossless() ? 1 : 0);
            iReport.Add(iLane, s.str());
        }
        aMsg->RemoveRef();
    }
    void NotifyDelay(TUint aJiffies) override { std::ostringstream s; s << "delay " << aJiffies; iReport.Add(iLane, s.str()); }
    void NotifyHalt() override { iReport.Add(iLane, "halt"); }
    void NotifyStopped(TUint aReason) override { std::ostringstream s; s << "stopped " << aReason; iReport.Add(iLane, s.str()); }
    void RequestResend(const Brx& aDatagram) override
    {
        std::string hex = "resend ";
        char two[3];
        for (TUint k = 0; k < aDatagram.Bytes(); k++) { snprintf(two, sizeof(two), "%02x", aDatagram[k]); hex += two; }
        iReport.Add(iLane, hex);
    }
    std::deque<MsgAudioPcm*> iAudio;
private:
    Report& iReport;
    size_t iLane;
};

static void TestBookkeeping()
{
    OhmReceiver r;
    TEST(r.PendingDatagrams() == 0 && !r.Stopped() && r.WaitingFrames() == 0 && r.FramesOutput() == 0);
    TEST(r.State().running == 0 && r.State().stream_msg_due == 1 && r.State().last_sample_start == 0xffffffffu && r.State().frame == 0);
    TEST(r.State().bit_depth == 0 && r.State().sample_rate == 0 && r.State().channels == 0 && r.State().latency == 0);
    std::vector<TByte> g(70000, 0x5a);
    r.PushDatagram(Brn(g.data(), 5));                                  // nothing is looked at: any bytes queue
    r.PushDatagram(Brn(g.data(), 0));
    r.PushDatagram(Brn(g.data(), 33));
    r.PushDatagram(Brn(g.data(), 5847));
    r.PushDatagram(Brn(g.data(), 1));
    TEST(r.PendingDatagrams() == 5);
    TEST(r.PendingOffset(0) == 0 && r.PendingOffset(1) == 16 && r.PendingOffset(2) == 16 && r.PendingOffset(3) == 64 && r.PendingOffset(4) == 5920);   // every datagram at a 16-byte boundary
    TEST(r.PendingBytes(3) == 5847 && r.PendingBytes(1) == 0);
    TEST_THROWS(r.PendingOffset(5), AssertionFailed);
    TEST_THROWS(r.PushDatagram(Brn(g.data(), 65536)), AssertionFailed);
    r.PushDatagram(Brn(g.data(), 65535));
    TEST(r.PendingDatagrams() == 6);
    // the tables of a tick: one stream, its datagrams where the arena puts them, room for what the table alone says it may carry
    OhmReceiver idle;
    OhmReceiver::Lane lanes[2] = {{&idle, nullptr, 0}, {&r, nullptr, 0}};
    OhmReceiver::Tick tick;
    OhmReceiver::Collect(lanes, 2, tick);
    TEST(tick.streams.size() == 1 && tick.laneOf.size() == 1 && tick.laneOf[0] == 1 && tick.datagrams.size() == 6);
    TEST(tick.streams[0].first_datagram == 0 && tick.streams[0].n_datagrams == 6 && tick.streams[0].dst_offset == 0);
    TEST(tick.streams[0].dst_capacity == (5847 - 58) + (65535 - 58) && tick.dstBytes % 16 == 0 && tick.dstBytes >= tick.streams[0].dst_capacity);
    TEST(tick.datagrams[3].src_offset == 64 && tick.datagrams[3].bytes == 5847 && tick.srcBytes % 16 == 0);
    TEST(ohgpu_ohm_rx_batch_check(tick.streams.data(), 1, tick.datagrams.data(), 6, tick.srcBytes, tick.dstBytes) == OHGPU_OK);
}

struct LaneSpec {
    std::vector<TByte> datagrams;
    std::vector<TUint> sizes;
    size_t perTick = 1, next = 0, offset = 0;
};

// a tick's device call, by csrc/ohm_rx_core.h on the CPU
static void FakeDevice(const OhmReceiver::Tick& aTick, const TByte* aSrc, TByte* aDst, std::vector<ohgpu_ohm_rx_stream_result>& aResults, std::vector<ohgpu_ohm_rx_record>& aRecords)
{
    static_assert(sizeof(ohmrx::Record) == sizeof(ohgpu_ohm_rx_record) && sizeof(ohmrx::Stream) == sizeof(ohgpu_ohm_rx_stream), "layouts");
    ohmrx::Record* recs = (ohmrx::Record*)aRecords.data();
    for (size_t k = 0; k < aTick.datagrams.size(); k++) ohmrx::parse(aSrc + aTick.datagrams[k].src_offset, aTick.datagrams[k].bytes, &recs[k]);
    for (size_t i = 0; i < aTick.streams.size(); i++) {
        uint32_t ring[ohmrx::kRing];
        const ohmrx::Stream& s = *(const ohmrx::Stream*)&aTick.streams[i];
        ohmrx::sequence(s, recs + s.first_datagram, ring, (ohmrx::StreamResult*)&aResults[i]);
    }
    for (size_t k = 0; k < aTick.datagrams.size(); k++) {
        if (recs[k].disposition != ohmrx::kOutput || recs[k].audio_bytes == 0) continue;
        for (uint32_t lane = 0; lane < 64; lane++)
            ohmrx::gather_lane(aSrc + aTick.datagrams[k].src_offset + recs[k].audio_offset, aDst + recs[k].dst_offset, recs[k].audio_bytes, lane, 64);
    }
}

static void TestTicks(MsgFactory& f, bool aGpu, const std::string& aJob, const std::string& aReportPath, const std::string& aBytesPath)
{
    std::vector<LaneSpec> specs;
    std::ifstream in(aJob);
    for (std::string line; std::getline(in, line); ) {
        std::istringstream ls(line);
        std::string stem;
        LaneSpec s;
        ls >> stem >> s.perTick;
        s.datagrams = ReadFile(stem + ".datagrams");
        s.sizes = ReadNumbers(stem + ".sizes");
        specs.push_back(s);
    }
    TEST(!specs.empty());
    Report report;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<OhmReceiver>> receivers;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<OhmReceiver::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    for (size_t k = 0; k < specs.size(); k++) {
        sinks.emplace_back(new Sink(report, k));
        receivers.emplace_back(new OhmReceiver(sinks[k].get(), sinks[k].get()));
        controllers.emplace_back(new CodecController(f, *sinks[k], 5 * Jiffies::kPerMs));       // the 5 ms cuts of a Songcast receiver's pipeline
        lanes.push_back({receivers[k].get(), controllers[k].get(), 0});
    }
    std::unique_ptr<PlayableBatch> batch(aGpu ? new PlayableBatch(f) : nullptr);
    for (size_t tick = 0; ; tick++) {
        bool more = false;
        for (size_t k = 0; k < specs.size(); k++) {
            LaneSpec& s = specs[k];
            for (size_t n = 0; n < s.perTick && s.next < s.sizes.size(); n++, s.next++) {
                if (s.sizes[s.next] == 0) { receivers[k]->Restart(); continue; }
                receivers[k]->PushDatagram(Brn(s.datagrams.data() + s.offset, s.sizes[s.next]));
                s.offset += s.sizes[s.next];
            }
            more = more || s.next < s.sizes.size();
        }
        if (aGpu) {
            OhmReceiver::Flush(f, lanes.data(), lanes.size());
        } else {
            OhmReceiver::Tick t;
            OhmReceiver::Collect(lanes.data(), lanes.size(), t);
            if (!t.streams.empty()) {
                TEST(ohgpu_ohm_rx_batch_check(t.streams.data(), t.streams.size(), t.datagrams.data(), t.datagrams.size(), t.srcBytes, t.dstBytes) == OHGPU_OK);
                std::vector<TByte> src((size_t)t.srcBytes), dst((size_t)t.dstBytes + 16, 0xA5);
                OhmReceiver::FillSource(lanes.data(), t, src.data());
                std::vector<ohgpu_ohm_rx_stream_result> results(t.streams.size());
                std::vector<ohgpu_ohm_rx_record> records(t.datagrams.size());
                FakeDevice(t, src.data(), dst.data(), results, records);
                OhmReceiver::Deliver(lanes.data(), t, results.data(), records.data(), dst.data());
            }
        }
        std::vector<std::unique_ptr<ProcessorPcmBufTest>> procs;
        std::vector<size_t> laneOf;
        for (size_t k = 0; k < specs.size(); k++) {
            std::ostringstream s;
            s << "tick " << tick << " waiting " << receivers[k]->WaitingFrames() << " queued " << receivers[k]->PendingDatagrams() << " stopped " << (receivers[k]->Stopped() ? 1 : 0);
            report.Add(k, s.str());
            while (!sinks[k]->iAudio.empty()) {
                MsgAudioPcm* m = sinks[k]->iAudio.front();
                sinks[k]->iAudio.pop_front();
                if (!aGpu) { m->RemoveRef(); continue; }
                procs.emplace_back(new ProcessorPcmBufTest());
                laneOf.push_back(k);
                batch->Add(m->CreatePlayable(), *procs.back());
            }
        }
        if (!procs.empty()) batch->Run();
        for (size_t i = 0; i < procs.size(); i++) {
            const Brn b = procs[i]->Buf();
            got[laneOf[i]].insert(got[laneOf[i]].end(), b.Ptr(), b.Ptr() + b.Bytes());
        }
        if (!more) break;
    }
    for (size_t k = 0; k < specs.size(); k++) {
        std::ostringstream s;
        s << "end frames " << receivers[k]->FramesOutput() << " bytes " << receivers[k]->BytesOutput() << " ignored " << receivers[k]->IgnoredWhileStopped();
        report.Add(k, s.str());
    }
    std::ofstream out(aReportPath);
    for (const std::string& line : report.lines) out << line << "\n";
    if (aGpu) {
        std::ofstream bytes(aBytesPath, std::ios::binary);
        for (const auto& lane : got) bytes.write((const char*)lane.data(), (std::streamsize)lane.size());
    }
    printf("ticks: %zu lanes, %zu report lines\n", specs.size(), report.lines.size());
}

int main(int argc, char** argv)
{
    if (argc < 4) { printf("usage: test_receiver cpu JOB REPORT | gpu JOB REPORT BYTES\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    TestBookkeeping();
    {
        MsgFactory f(gpu ? 0 : -1);
        TestTicks(f, gpu, argv[2], argv[3], argc > 4 ? argv[4] : "");
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
