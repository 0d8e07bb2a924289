// test_mpegts_demuxer.cpp -- MpegTsAdtsBatchDemuxer, MpegTsRecognise, AdtsRecognise, Id3v2Skip (host/MpegTsDemuxer.h) for
// tests/test_ts_host_cpp.py.
//   test_mpegts_demuxer cpu STEM...   the recognisers; then every STEM through the element with csrc/ts_packet_core.h, built for the CPU,
//                                     standing in for the device between Collect and Apply
//   test_mpegts_demuxer gpu STEM...   every STEM a lane of MpegTsAdtsBatchDemuxer::Tick: one fused device call a tick for all lanes
// STEM.ts: the transport bytes; STEM.pieces: the sizes they are pushed in, a tick after every third push; STEM.es: the elementary bytes;
// STEM.want: a line per frame, "offset bytes pts" (pts -1: none); STEM.state: "pmt_pid audio_pid pes_open_bytes kept_bytes corrupt" at the end.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/csrc/ts_packet_core.h"
#include "../../ohpipeline_amd/host/DecodedAudioAggregator.h"
#include "../../ohpipeline_amd/host/Msg.h"
#include "../../ohpipeline_amd/host/MpegTsDemuxer.h"

using namespace OpenHome;
using namespace OpenHome::Media;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)

static std::vector<TByte> ReadFile(const std::string& aName)
{
    std::ifstream f(aName, std::ios::binary);
    return std::vector<TByte>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static std::vector<long long> ReadNumbers(const std::string& aName)
{
    std::ifstream f(aName);
    std::vector<long long> out;
    long long v;
    while (f >> v) out.push_back(v);
    return out;
}

struct Got { TUint64 offset; TUint bytes; TUint64 pts; TUint headerBytes; };
struct Sink : IAdtsFrameSink {
    std::vector<Got> frames;
    std::vector<TByte> bytes;                                          // the frames, one after the other
    void OutputAdtsFrame(TUint64 aEsOffset, const Brx& aFrame, const ohgpu_adts_frame& aHeader, TUint64 aPts) override
    {
        frames.push_back(Got{aEsOffset, aFrame.Bytes(), aPts, aHeader.header_bytes});
        TEST(aFrame.Bytes() == aHeader.bytes && aFrame.Ptr()[0] == 0xff);
        bytes.insert(bytes.end(), aFrame.Ptr(), aFrame.Ptr() + aFrame.Bytes());
    }
};

// What the device does between Collect and Apply, on the CPU: the core's serial text over the lane's queue
static void StandIn(MpegTsAdtsBatchDemuxer& d)
{
    ohgpu_ts_stream_desc ts;
    ohgpu_adts_stream_desc ad;
    d.Collect(0, 0, 0, 0, ts, ad);
    std::vector<uint8_t> src(d.Pending().begin(), d.Pending().begin() + ts.src_bytes), dst(d.Kept());
    src.resize(src.size() + 4);
    dst.resize(dst.size() + ts.dst_capacity + 16);
    const uint32_t np = ts.src_bytes / 188u;
    std::vector<tspkt::Pes> pes(ts.pes_capacity + 1);
    std::vector<tspkt::Pkt> pk(np + 1);
    std::vector<uint32_t> run_end(np + 1), src_at(np + 1);
    tspkt::Stream s;
    memcpy(&s, &ts, sizeof(s));
    tspkt::Result r;
    tspkt::demux(s, src.data(), dst.data(), pes.data(), pk.data(), run_end.data(), src_at.data(), &r);
    adts::Stream as;
    memcpy(&as, &ad, sizeof(as));
    as.src_bytes = (uint32_t)d.Kept().size() + r.bytes_delivered;
    std::vector<adts::Frame> frames(as.frame_capacity + 1);
    adts::Result ar;
    adts::walk(as, dst.data(), frames.data(), &ar);
    ohgpu_ts_stream_result tr;
    ohgpu_adts_stream_result aar;
    memcpy(&tr, &r, sizeof(tr));
    memcpy(&aar, &ar, sizeof(aar));
    d.Apply(tr, (const ohgpu_ts_pes*)pes.data(), aar, (const ohgpu_adts_frame*)frames.data(), dst.data());
}

static void TestRecognisers()
{
    const TByte ts[4] = {0x47, 0x40, 0x00, 0x10}, no[4] = {0x48, 0x47, 0, 0};
    TEST(MpegTsRecognise(Brn(ts, 4)) && !MpegTsRecognise(Brn(no, 4)) && !MpegTsRecognise(Brn(ts, 0)));
    std::vector<TByte> aac;
    for (int k = 0; k < 7; k++) {
        const TUint n = 7 + 20 + k;
        const TByte head[7] = {0xff, 0xf1, 0x50, (TByte)(0x80 | (n >> 11)), (TByte)(n >> 3), (TByte)(((n & 7) << 5) | 0x1f), 0xfc};
        aac.insert(aac.end(), head, head + 7);
        aac.insert(aac.end(), 20 + k, (TByte)k);
    }
    TUint start = 99;
    TEST(AdtsRecognise(Brn(aac.data(), (TUint)aac.size()), &start) && start == 0);
    std::vector<TByte> led(1001, 0x11);
    led.insert(led.end(), aac.begin(), aac.end());
    TEST(AdtsRecognise(Brn(led.data(), (TUint)led.size()), &start) && start == 1001);
    led.insert(led.begin(), 0x11);
    TEST(!AdtsRecognise(Brn(led.data(), (TUint)led.size()), &start));
    TEST(!AdtsRecognise(Brn(aac.data(), 27 + 28 + 29 + 30 + 9), nullptr) && AdtsRecognise(Brn(aac.data(), 27 + 28 + 29 + 30 + 10), nullptr));
    std::vector<TByte> tagged = {'I', 'D', '3', 4, 0, 0, 0, 0, 1, 5};
    tagged.resize(10 + 133, 0);
    tagged.insert(tagged.end(), aac.begin(), aac.end());
    TEST(Id3v2Skip(Brn(tagged.data(), (TUint)tagged.size())) == 143 && Id3v2Skip(Brn(aac.data(), (TUint)aac.size())) == 0);
    Sink sink;
    MpegTsAdtsBatchDemuxer d(sink);
    TEST(!d.TrySeek(1, 0) && d.PendingBytes() == 0 && d.EsBytes() == 0 && !d.Recognised());
}

static void RunLanes(bool aGpu, int aCount, char** aStems)
{
    std::vector<Sink> sinks(aCount);
    std::vector<MpegTsAdtsBatchDemuxer*> lanes;
    std::vector<std::vector<TByte>> data;
    std::vector<std::vector<long long>> pieces;
    std::vector<size_t> at(aCount, 0), piece(aCount, 0);
    for (int i = 0; i < aCount; i++) {
        lanes.push_back(new MpegTsAdtsBatchDemuxer(sinks[i]));
        data.push_back(ReadFile(std::string(aStems[i]) + ".ts"));
        pieces.push_back(ReadNumbers(std::string(aStems[i]) + ".pieces"));
        TEST(!data[i].empty() && !pieces[i].empty() && MpegTsRecognise(Brn(data[i].data(), 1)));
    }
    MsgFactory* factory = aGpu ? new MsgFactory(0) : nullptr;
    bool threw = false;
    TUint ticks = 0;
    for (bool more = true; more;) {
        more = false;
        for (int i = 0; i < aCount; i++)
            for (int k = 0; k < 3 && piece[i] < pieces[i].size(); k++) {
                const size_t n = (size_t)pieces[i][piece[i]++];
                lanes[i]->Push(Brn(data[i].data() + at[i], (TUint)n));
                at[i] += n;
                more = true;
            }
        if (!more) break;
        ticks++;
        if (aGpu) {
            std::vector<MpegTsAdtsBatchDemuxer::Lane> l;
            for (int i = 0; i < aCount; i++) l.push_back(MpegTsAdtsBatchDemuxer::Lane{lanes[i]});
            try { MpegTsAdtsBatchDemuxer::Tick(*factory, l.data(), l.size()); } catch (CodecStreamCorrupt&) { threw = true; }
        } else {
            for (int i = 0; i < aCount; i++) StandIn(*lanes[i]);
        }
    }
    bool anyCorrupt = false;
    for (int i = 0; i < aCount; i++) {
        const std::vector<long long> want = ReadNumbers(std::string(aStems[i]) + ".want"), state = ReadNumbers(std::string(aStems[i]) + ".state");
        const std::vector<TByte> es = ReadFile(std::string(aStems[i]) + ".es");
        TEST(at[i] == data[i].size() && state.size() == 5);
        TEST(sinks[i].frames.size() * 3 == want.size());
        bool same = sinks[i].frames.size() * 3 == want.size();
        for (size_t k = 0; same && k < sinks[i].frames.size(); k++) {
            const Got& g = sinks[i].frames[k];
            same = (long long)g.offset == want[3 * k] && (long long)g.bytes == want[3 * k + 1] && (g.pts == OHGPU_TS_NO_PTS ? -1 : (long long)g.pts) == want[3 * k + 2];
            if (!same) printf("lane %d frame %zu: %llu %u %lld, wanted %lld %lld %lld\n", i, k, (unsigned long long)g.offset, g.bytes, (long long)g.pts, want[3 * k], want[3 * k + 1], want[3 * k + 2]);
        }
        TEST(same);
        size_t pos = 0;                                                // every frame's bytes are the elementary stream's at its offset
        bool bytesSame = true;
        for (const Got& g : sinks[i].frames) {
            bytesSame = bytesSame && g.offset + g.bytes <= es.size() && memcmp(sinks[i].bytes.data() + pos, es.data() + g.offset, g.bytes) == 0;
            pos += g.bytes;
        }
        TEST(bytesSame);
        if (state.size() == 5) {
            TEST((long long)lanes[i]->PmtPid() == state[0] && (long long)lanes[i]->AudioPid() == state[1] && (long long)lanes[i]->PesOpenBytes() == state[2]);
            TEST((long long)lanes[i]->KeptBytes() == state[3] && (long long)lanes[i]->Corrupt() == state[4]);
            anyCorrupt = anyCorrupt || state[4];
        }
        TEST(lanes[i]->PendingBytes() == (lanes[i]->Corrupt() ? 0u : data[i].size() % 188u) && lanes[i]->Frames() == sinks[i].frames.size());
        TEST(lanes[i]->EsBytes() == es.size());
        if (same && bytesSame) printf("lane %d: %zu frames byte-exact over %u ticks\n", i, sinks[i].frames.size(), ticks);
    }
    if (aGpu) TEST(threw == anyCorrupt);
    for (MpegTsAdtsBatchDemuxer* d : lanes) delete d;
    delete factory;
}

int main(int argc, char** argv)
{
    if (argc < 3 || (strcmp(argv[1], "cpu") != 0 && strcmp(argv[1], "gpu") != 0)) { fprintf(stderr, "usage: %s cpu|gpu STEM...\n", argv[0]); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    if (!gpu) TestRecognisers();
    RunLanes(gpu, argc - 2, argv + 2);
    printf("%s: %d checks, %d failures\n", argv[1], gChecks, gFailures);
    return gFailures ? 1 : 0;
}
