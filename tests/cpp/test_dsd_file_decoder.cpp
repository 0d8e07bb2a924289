// test_dsd_file_decoder.cpp -- DSD files in the host adapter (ohpipeline_amd/host/DsdFileDecoder.h: DsfRecognise, DffRecognise,
// DsdFileBatchDecoder, CodecController::OutputDecodedStreamDsd).
// `test_dsd_file_decoder cpu <manifest>` runs what needs no device: the two recognition rules, a decoder's state before any tick, and
// per line of the manifest the host-side walk (Head) over the file pushed in pieces, against the fields the manifest states.
// `test_dsd_file_decoder gpu <manifest>` adds the whole path: per line one lane -- a file, the bytes that must reach the processor,
// the sizes its messages must have, what becomes of it (0 plays, 1 CodecStreamCorrupt, 2 CodecStreamFeatureUnsupported, 3 not
// recognised: dropped, nothing thrown), its format (W, P), a sample to seek to once its stream has been announced (-1: none), and the
// kind, rate and sample count its record must carry -- pushed in 20000-byte pieces over as many ticks as it takes, ONE Flush per
// tick for all lanes, every message read through a playable into ProcessorDsdBufTest.  The expectations are made by
// tests/test_dsd_file_host_cpp.py from the model and the record of the tests' own writer.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/DsdFileDecoder.h"
#include "../../ohpipeline_amd/host/Msg.h"
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
        if (KindOf(aMsg) == MsgKind::AudioDsd) { iAudio.push_back(static_cast<MsgAudioDsd*>(aMsg)); return; }
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
    std::deque<MsgAudioDsd*> iAudio;
    TUint iStreams = 0, iAudioSeen = 0, iBitRate = 0, iBitDepth = 0, iRate = 0, iChannels = 0;
    TUint64 iLength = 0, iStart = 0;
    TBool iStreamBeforeAudio = false, iLossless = false;
    std::string iName;
};

static void TestRecognise()
{
    const TByte dsf[17] = {'D', 'S', 'D', ' ', 28, 0, 0, 0, 0, 0, 0, 0, 9, 9, 9, 9, 9};
    const TByte dff[16] = {'F', 'R', 'M', '8', 0, 0, 0, 0, 0, 0, 1, 0, 'D', 'S', 'D', ' '};
    const TByte pcm[16] = {'F', 'R', 'M', '8', 0, 0, 0, 0, 0, 0, 1, 0, 'P', 'C', 'M', ' '};
    const TByte lower[4] = {'d', 's', 'd', ' '};
    TEST(DsfRecognise(Brn(dsf, 4)) && DsfRecognise(Brn(dsf, 17)) && !DsfRecognise(Brn(dsf, 3)) && !DsfRecognise(Brn(dsf, 0)));
    TEST(!DffRecognise(Brn(dsf, 17)) && !DsfRecognise(Brn(dff, 16)) && !DsfRecognise(Brn(lower, 4)));
    TEST(DffRecognise(Brn(dff, 16)) && !DffRecognise(Brn(dff, 15)) && !DffRecognise(Brn(dff, 4)) && !DffRecognise(Brn(pcm, 16)));
}

static void TestBeforeAnyTick()
{
    const TByte dff[16] = {'F', 'R', 'M', '8', 0, 0, 0, 0, 0, 0, 1, 0, 'D', 'S', 'D', ' '};
    DsdFileBatchDecoder d(6, 2);
    d.Push(Brn(dff, 5));
    d.Push(Brn(dff + 5, 11));
    TEST(d.BytesPushed() == 16 && !d.Announced() && !d.Dropped() && d.Recognised() && d.NextChunk() == 0);
    const ohgpu_dsd_file_stream_result head = d.Head();
    TEST(head.status == OHGPU_DSD_FILE_TRUNCATED && head.error_offset == 16 && head.kind == 0);   // a DFF file whose chunks have not arrived
    DsdFileBatchDecoder::Lane lane = {&d, nullptr, 0};
    TEST(!DsdFileBatchDecoder::TrySeek(lane, 0) && lane.trackOffset == 0);            // (no stream before the first tick)
    TEST_THROWS(d.Result(), AssertionFailed);
    TEST_THROWS(DsdFileBatchDecoder(6, 4), AssertionFailed);                          // the library's own rule for (W, P)
    TEST_THROWS(DsdFileBatchDecoder(0, 0), AssertionFailed);
    DsdFileBatchDecoder none(2, 0);
    TEST(none.Head().status == OHGPU_DSD_FILE_NOT_DSD);
    uint64_t first = 0, rounded = 0;                                                  // the two grids a seek lands on
    TEST(ohgpu_dsd_file_seek(OHGPU_DSD_FILE_KIND_DSF, 70000, &first, &rounded) == OHGPU_OK && rounded == 65536 && first == 4096);
    TEST(ohgpu_dsd_file_seek(OHGPU_DSD_FILE_KIND_DFF, 70000, &first, &rounded) == OHGPU_OK && rounded == 69632 && first == 4352);
}

struct LaneSpec {
    std::vector<TByte> file, want;
    std::vector<TUint> pieces;
    int fate;
    TUint W, P;
    long long seek;
    TUint kind, rate;
    unsigned long long samples, chunks, dataOffset;
};

static std::vector<LaneSpec> ReadManifest(const std::string& aManifest)
{
    std::vector<LaneSpec> specs;
    std::ifstream in(aManifest);
    for (std::string line; std::getline(in, line); ) {
        std::istringstream ls(line);
        std::string file, want, pieces;
        LaneSpec s;
        ls >> file >> want >> pieces >> s.fate >> s.W >> s.P >> s.seek >> s.kind >> s.rate >> s.samples >> s.chunks >> s.dataOffset;
        s.file = ReadFile(file);
        s.want = ReadFile(want);
        std::ifstream pf(pieces);
        for (TUint v; pf >> v; ) s.pieces.push_back(v);
        specs.push_back(s);
    }
    return specs;
}

// The host-side walk over a file as it arrives: TRUNCATED or NOT_DSD until its chunks are there, then the record the manifest states
static void TestHeads(const std::vector<LaneSpec>& aSpecs)
{
    for (const LaneSpec& s : aSpecs) {
        DsdFileBatchDecoder d(s.W, s.P);
        bool settled = false;
        for (size_t lo = 0; lo < s.file.size(); lo += 37) {
            const size_t hi = std::min(s.file.size(), lo + 37);
            d.Push(Brn(s.file.data() + lo, (TUint)(hi - lo)));
            const ohgpu_dsd_file_stream_result head = d.Head();
            if (settled) { TEST(head.status == OHGPU_DSD_FILE_OK); continue; }
            if (head.status == OHGPU_DSD_FILE_OK) settled = true;
            else if (s.fate == 0) TEST(head.status == OHGPU_DSD_FILE_TRUNCATED || (head.status == OHGPU_DSD_FILE_NOT_DSD && hi < 16));
        }
        const ohgpu_dsd_file_stream_result head = d.Head();
        if (s.fate == 0) {
            TEST(head.status == OHGPU_DSD_FILE_OK && head.kind == s.kind && head.channels == 2 && head.sample_rate == s.rate);
            TEST(head.sample_count == s.samples && head.chunks_total == s.chunks && head.data_offset == s.dataOffset);
            TEST(head.chunks_available == s.chunks && head.chunks_written == s.chunks);
        } else {
            TEST(head.status == (s.fate == 1 ? OHGPU_DSD_FILE_TRUNCATED : s.fate == 2 ? OHGPU_DSD_FILE_UNSUPPORTED : OHGPU_DSD_FILE_NOT_DSD));
        }
    }
}

static void TestPipeline(MsgFactory& f, const std::vector<LaneSpec>& specs)
{
    TEST(specs.size() == 5);
    std::vector<std::unique_ptr<DsdFileBatchDecoder>> decoders;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<DsdFileBatchDecoder::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    std::vector<std::vector<TUint>> sizes(specs.size());
    std::vector<TUint64> jiffies(specs.size(), 0);
    std::vector<bool> sought(specs.size(), false);
    size_t ticks = 0, corruptSeen = 0, unsupportedSeen = 0, seeks = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        decoders.emplace_back(new DsdFileBatchDecoder(specs[k].W, specs[k].P));
        sinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerMs * 5));
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
            served = served || (!decoders[k]->Dropped() && specs[k].fate != 3);
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        try {
            DsdFileBatchDecoder::Flush(f, lanes.data(), lanes.size());
        } catch (CodecStreamCorrupt&) {
            corruptSeen++;
            for (size_t k = 0; k < specs.size(); k++) TEST(specs[k].fate != 1 || (decoders[k]->Dropped() && decoders[k]->Recognised()));
            for (size_t k = 0; k < specs.size(); k++) TEST(specs[k].fate != 0 || decoders[k]->Announced());      // every lane was served first
        } catch (CodecStreamFeatureUnsupported&) {
            unsupportedSeen++;
            for (size_t k = 0; k < specs.size(); k++) TEST(specs[k].fate != 2 || (decoders[k]->Dropped() && decoders[k]->Result().status == OHGPU_DSD_FILE_UNSUPPORTED));
            for (size_t k = 0; k < specs.size(); k++) TEST(specs[k].fate != 0 || decoders[k]->Announced());
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        TEST(calls1 == calls0 + (served ? 1 : 0));                                  // one call a tick for all lanes
        std::vector<std::unique_ptr<ProcessorDsdBufTest>> procs;
        std::vector<size_t> laneOf;
        for (size_t k = 0; k < specs.size(); k++) {
            while (!sinks[k]->iAudio.empty()) {
                MsgAudioDsd* m = sinks[k]->iAudio.front();
                sinks[k]->iAudio.pop_front();
                sinks[k]->iAudioSeen++;
                TEST(m->TrackOffset() == jiffies[k]);
                TEST(m->SampleBlockWords() == specs[k].W);
                jiffies[k] += m->Jiffies();
                MsgPlayable* p = m->CreatePlayable();
                TEST(p->Bytes() % (specs[k].W * 4) == 0);                           // whole sample blocks
                sizes[k].push_back(p->Bytes());
                procs.emplace_back(new ProcessorDsdBufTest());
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
            const TUint64 total = decoders[k]->Result().sample_count;
            TEST(total > (TUint64)specs[k].seek && sinks[k]->iStreams == 1 && sinks[k]->iStart == 0);
            TEST(!DsdFileBatchDecoder::TrySeek(lanes[k], total) && !DsdFileBatchDecoder::TrySeek(lanes[k], 1ull << 40));     // beyond the track: refused,
            TEST(lanes[k].trackOffset == jiffies[k] && sinks[k]->iStreams == 1);                                              // and nothing changes
            TEST(DsdFileBatchDecoder::TrySeek(lanes[k], (TUint64)specs[k].seek));
            const TUint64 grid = specs[k].kind == OHGPU_DSD_FILE_KIND_DSF ? 32768u : 2048u, rounded = (TUint64)specs[k].seek / grid * grid;
            TEST(decoders[k]->NextChunk() == rounded / 16 && sinks[k]->iStreams == 2 && sinks[k]->iStart == rounded);
            TEST(lanes[k].trackOffset == (specs[k].kind == OHGPU_DSD_FILE_KIND_DSF ? rounded * Jiffies::PerSample(specs[k].rate) : rounded * Jiffies::kPerSecond / specs[k].rate));
            jiffies[k] = lanes[k].trackOffset;
            sought[k] = true;
            seeks++;
        }
    }
    size_t bytesChecked = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        if (got[k] != specs[k].want || sizes[k] != specs[k].pieces)
            printf("lane %zu: %zu bytes in %zu messages where %zu in %zu are due; next chunk %llu\n", k, got[k].size(), sizes[k].size(), specs[k].want.size(), specs[k].pieces.size(),
                   (unsigned long long)decoders[k]->NextChunk());
        TEST(got[k].size() == specs[k].want.size());
        TEST(got[k] == specs[k].want);
        TEST(sizes[k] == specs[k].pieces);
        const Sink& s = *sinks[k];
        if (specs[k].fate == 0) {
            TEST(s.iStreams == (specs[k].seek < 0 ? 1u : 2u) && s.iStreamBeforeAudio && s.iLossless);
            TEST(s.iBitDepth == 1 && s.iRate == specs[k].rate && s.iChannels == 2 && s.iBitRate == 2 * specs[k].rate && s.iName == "DSD");
            TEST(s.iLength == specs[k].samples * Jiffies::PerSample(specs[k].rate));
            TEST(decoders[k]->Result().kind == specs[k].kind && decoders[k]->Result().chunks_total == specs[k].chunks);
        } else {
            TEST(got[k].empty() && s.iStreams == 0 && decoders[k]->Dropped());
            TEST(decoders[k]->Recognised() == (specs[k].fate != 3));
        }
        bytesChecked += got[k].size();
    }
    TEST(corruptSeen == 1 && unsupportedSeen == 1 && seeks == 2);
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", specs.size(), ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    if (argc < 3) { printf("usage: test_dsd_file_decoder cpu|gpu <manifest>\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    const std::vector<LaneSpec> specs = ReadManifest(argv[2]);
    TestRecognise();
    TestBeforeAnyTick();
    TestHeads(specs);
    printf("cpu: %d checks\n", gChecks);
    if (gpu) {
        MsgFactory f(0);
        TestPipeline(f, specs);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
