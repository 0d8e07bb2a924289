// test_ogg_flac_decoder.cpp -- Ogg FLAC in the host adapter (ohpipeline_amd/host/OggFlacDecoder.h: FlacRecognise, OggFlacBatchDecoder;
// DESIGN.md 5.15).
// `test_ogg_flac_decoder cpu <stream.ogg> <stream.flac>` runs what needs no device: CodecFlac::Recognise's rule, the byte queue's
// bookkeeping, the head arriving over ragged pushes (the same STREAMINFO as the native stream's, the queue cut at the first audio
// page), the refusals.
// `test_ogg_flac_decoder gpu <stream.ogg> <stream.flac> <manifest>` adds the whole path: per line of the manifest one lane -- a
// stream's file, the bytes that must reach the processor, the sizes its messages must have, whether the lane must throw -- pushed in
// 1000-byte pieces over as many ticks as it takes, ONE Flush per tick for all lanes, every message read through a playable into
// ProcessorPcmBufTest.  The expectations are made by tests/test_ogg_host_cpp.py from the plain-Python models.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/OggFlacDecoder.h"
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

static void TestRecognise(const std::vector<TByte>& aOgg, const std::vector<TByte>& aFlac)
{
    // Flac.cpp:155-178 over the 42 bytes it reads
    TEST(FlacRecognise(Brn(aFlac.data(), 42)) == FlacStreamKind::Native);
    TEST(FlacRecognise(Brn(aFlac.data(), 4)) == FlacStreamKind::Native && FlacRecognise(Brn(aFlac.data(), 3)) == FlacStreamKind::None);
    TEST(FlacRecognise(Brn(aOgg.data(), 42)) == FlacStreamKind::Ogg);
    TEST(FlacRecognise(Brn(aOgg.data(), 41)) == FlacStreamKind::None);               // "fLaC" is there, the 42nd byte is not
    std::vector<TByte> other(aOgg.begin(), aOgg.begin() + 42);
    other[37] = 'v';                                                                 // an Ogg stream of another codec
    TEST(FlacRecognise(Brn(other.data(), 42)) == FlacStreamKind::None);
    const TByte riff[42] = {'R', 'I', 'F', 'F'};
    TEST(FlacRecognise(Brn(riff, 42)) == FlacStreamKind::None && FlacRecognise(Brn(riff, 0)) == FlacStreamKind::None);
}

static void TestBookkeeping(const std::vector<TByte>& aOgg, const std::vector<TByte>& aFlac)
{
    // the head over ragged pushes: known exactly when its last byte is in, and the queue starts at the first audio page from then on
    ohgpu_flac_streaminfo_t want, viaOgg;
    uint64_t audio = 0, page = 0;
    uint32_t serial = 0, segment = 0, seq = 0;
    TEST(ohgpu_flac_streaminfo(aFlac.data(), aFlac.size(), &want, &audio) == OHGPU_OK);
    TEST(ohgpu_ogg_flac_head(aOgg.data(), aOgg.size(), &viaOgg, &serial, &page, &segment, &seq) == OHGPU_OK && page > 42 && segment == 0);
    TEST(memcmp(&want, &viaOgg, sizeof(want)) == 0);
    TEST(ohgpu_ogg_flac_head(aOgg.data(), (size_t)page - 1, &viaOgg, &serial, &page, &segment, &seq) == OHGPU_ERR_INVALID);
    TEST(ohgpu_ogg_flac_head(aFlac.data(), aFlac.size(), &viaOgg, &serial, &page, &segment, &seq) == OHGPU_ERR_INVALID);
    TEST(ohgpu_ogg_flac_head(aOgg.data(), aOgg.size(), &viaOgg, &serial, &page, &segment, &seq) == OHGPU_OK);
    OggFlacBatchDecoder d;
    const TUint steps[] = {3, 1, 2, 5, 7, 11, 13, 1, 1, 40, 17, 60};
    size_t at = 0;
    for (TUint n : steps) {
        TEST(d.StreamInfoKnown() == (at >= page));
        TEST(d.PendingBytes() == (at >= page ? at - page : 0));
        d.Push(Brn(aOgg.data() + at, n));
        at += n;
    }
    TEST(at >= page && d.StreamInfoKnown() && d.PendingBytes() == at - page && d.SamplesDecoded() == 0 && !d.Corrupt());
    TEST(d.StreamInfo().channels == want.channels && d.StreamInfo().bits == want.bits && d.StreamInfo().sample_rate == want.sample_rate);
    TEST(d.StreamInfo().max_blocksize == want.max_blocksize && d.StreamInfo().total_samples == want.total_samples);
    TEST(memcmp(d.StreamInfo().md5, want.md5, 16) == 0);
    TEST(d.Serial() == serial && d.NextPageNumber() == seq && d.ResumeSegment() == 0);
    d.Push(Brn(aOgg.data(), 0));
    TEST(d.PendingBytes() == at - page);
    TEST_THROWS(OggFlacBatchDecoder().StreamInfo(), AssertionFailed);
    // what is no Ogg FLAC stream is refused as soon as that can be told
    const TByte riff[] = {'R', 'I', 'F', 'F'}, near[] = {'O', 'g', 'g', 'X'};
    { OggFlacBatchDecoder x; TEST_THROWS(x.Push(Brn(riff, 1)), CodecStreamCorrupt); TEST(x.Corrupt()); }
    { OggFlacBatchDecoder x; x.Push(Brn(near, 3)); TEST_THROWS(x.Push(Brn(near + 3, 1)), CodecStreamCorrupt); }
    { OggFlacBatchDecoder x; TEST_THROWS(x.Push(Brn(aFlac.data(), 42)), CodecStreamCorrupt); }      // a native stream goes to FlacBatchDecoder
    {   // "OggS" and 41 bytes say nothing yet; the 42nd decides
        std::vector<TByte> other(aOgg.begin(), aOgg.begin() + 42);
        other[38] = 'l';
        OggFlacBatchDecoder x;
        x.Push(Brn(other.data(), 41));
        TEST(!x.Corrupt());
        TEST_THROWS(x.Push(Brn(other.data() + 41, 1)), CodecStreamCorrupt);
    }
}

struct LaneSpec {
    std::vector<TByte> file, want;
    std::vector<TUint> pieces;
    bool throws;
};

static void TestPipeline(MsgFactory& f, const std::string& aManifest)
{
    std::vector<LaneSpec> specs;
    std::ifstream in(aManifest);
    for (std::string line; std::getline(in, line); ) {
        std::istringstream ls(line);
        std::string flac, want, pieces;      // (flac: the lane's .ogg file)
        int throws = 0;
        ls >> flac >> want >> pieces >> throws;
        LaneSpec s;
        s.file = ReadFile(flac);
        s.want = ReadFile(want);
        std::ifstream pf(pieces);
        for (TUint v; pf >> v; ) s.pieces.push_back(v);
        s.throws = throws != 0;
        specs.push_back(s);
    }
    TEST(specs.size() == 5);
    std::vector<std::unique_ptr<OggFlacBatchDecoder>> decoders;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<OggFlacBatchDecoder::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    std::vector<std::vector<TUint>> sizes(specs.size());
    std::vector<TUint64> jiffies(specs.size(), 0);
    size_t ticks = 0, throwsSeen = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        decoders.emplace_back(new OggFlacBatchDecoder());
        sinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerSecond));
        lanes.push_back({decoders[k].get(), controllers[k].get(), 0});
        ticks = std::max(ticks, (specs[k].file.size() + 999) / 1000);
    }
    PlayableBatch batch(f);
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    for (size_t t = 0; t < ticks; t++) {
        bool anything = false;
        for (size_t k = 0; k < specs.size(); k++) {
            const size_t lo = t * 1000, hi = std::min(specs[k].file.size(), lo + 1000);
            if (lo < hi && !decoders[k]->Corrupt()) decoders[k]->Push(Brn(specs[k].file.data() + lo, (TUint)(hi - lo)));
            anything = anything || (decoders[k]->PendingBytes() != 0 && !decoders[k]->Corrupt());
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        try {
            OggFlacBatchDecoder::Flush(f, lanes.data(), lanes.size());
        } catch (CodecStreamCorrupt&) {
            throwsSeen++;
            for (size_t k = 0; k < specs.size(); k++) TEST(decoders[k]->Corrupt() == specs[k].throws);
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + (anything ? 1 : 0));                                 // every lane's decode in one device call
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
        TEST(got[k].size() == specs[k].want.size());
        TEST(got[k] == specs[k].want);
        TEST(sizes[k] == specs[k].pieces);
        TEST(sinks[k]->iStreams == 1 && sinks[k]->iStreamBeforeAudio);
        TEST(lanes[k].trackOffset == jiffies[k]);
        if (!specs[k].throws) TEST(decoders[k]->PendingBytes() == 0 && decoders[k]->SamplesDecoded() * decoders[k]->StreamInfo().channels * (decoders[k]->StreamInfo().bits / 8) == got[k].size());
        if (specs[k].throws) TEST(!got[k].empty());                                  // its good frames came first
        bytesChecked += got[k].size();
    }
    TEST(throwsSeen == 1);
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", specs.size(), ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    if (argc < 4) { printf("usage: test_ogg_flac_decoder cpu|gpu stream.ogg stream.flac [manifest]\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    TestRecognise(ReadFile(argv[2]), ReadFile(argv[3]));
    TestBookkeeping(ReadFile(argv[2]), ReadFile(argv[3]));
    printf("cpu: %d checks\n", gChecks);
    if (gpu && argc > 4) {
        MsgFactory f(0);
        TestPipeline(f, argv[4]);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
