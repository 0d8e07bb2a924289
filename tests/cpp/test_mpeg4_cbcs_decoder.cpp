// test_mpeg4_cbcs_decoder.cpp -- the host element's all-schemes option (ohpipeline_amd/host/Mpeg4CencDecoder.h: Mpeg4CencBatchDecoder made
// with aAllSchemes, which is served by ohgpu_cbcs_*), in the shape of tests/cpp/test_mpeg4_cenc_decoder.cpp, which stays
// as it is and holds the element without the option to what it did before.
// `test_mpeg4_cbcs_decoder cpu <cbcs.mp4> <init-bytes> <kid-hex> <key-hex> <crypt> <skip> <constant-iv-bytes>` runs what needs no device: a
// `cbcs` stream is Other to the recognition and to an element without the option and Flac with it; the head is read exactly when the
// stated byte has arrived and the provider is asked exactly then, ONCE, by the head's kid; the wide head has the pattern and the
// constant IV.
// `test_mpeg4_cbcs_decoder gpu ... <manifest>` adds the whole path: per line of the manifest one lane -- a stream, the bytes that must
// reach the processor, what it must throw (0 nothing, 2 CodecStreamFeatureUnsupported), whether the lane has the option, and the lane's
// kid and key in hex ("-": the provider has no key) -- pushed in PIECE-byte pieces over as many ticks as it takes, ONE Flush per tick for
// all lanes of both families, every message read through a playable into ProcessorPcmBufTest.
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ohgpu.h"
#include "../../ohpipeline_amd/host/Mpeg4CencDecoder.h"
#include "../../ohpipeline_amd/host/Msg.h"

using namespace OpenHome;
using namespace OpenHome::Media;

static int gFailures = 0, gChecks = 0;
#define TEST(x) do { gChecks++; if (!(x)) { gFailures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } } while (0)
static const size_t PIECE = 3000;

static std::vector<TByte> ReadFile(const std::string& aPath)
{
    std::ifstream in(aPath, std::ios::binary);
    return std::vector<TByte>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static std::vector<TByte> Hex(const std::string& aText)
{
    std::vector<TByte> out;
    for (size_t k = 0; k + 1 < aText.size(); k += 2) out.push_back((TByte)strtoul(aText.substr(k, 2).c_str(), nullptr, 16));
    return out;
}

class Keys : public ICencKeyProvider {
public:
    TBool Key(const Brx& aKid, Bwx& aKey16) override
    {
        iCalls++;
        const std::vector<TByte> kid(aKid.Ptr(), aKid.Ptr() + aKid.Bytes());
        const auto it = iKeys.find(kid);
        if (it == iKeys.end() || aKey16.MaxBytes() < 16) return false;
        aKey16.Replace(Brn(it->second.data(), 16));
        return true;
    }
    std::map<std::vector<TByte>, std::vector<TByte>> iKeys;
    TUint iCalls = 0;
};

class Sink : public IPipelineElementDownstream {
public:
    void Push(Msg* aMsg) override
    {
        if (KindOf(aMsg) == MsgKind::AudioPcm) { iAudio.push_back(static_cast<MsgAudioPcm*>(aMsg)); return; }
        if (KindOf(aMsg) == MsgKind::DecodedStream) iStreams++;
        aMsg->RemoveRef();
    }
    std::deque<MsgAudioPcm*> iAudio;
    TUint iStreams = 0;
};

static void TestHead(const std::vector<TByte>& aFile, size_t aInitBytes, const std::vector<TByte>& aKid, const std::vector<TByte>& aKey, TUint aCrypt, TUint aSkip, TUint aConstantIv)
{
    TEST(Mpeg4CencRecognise(Brn(aFile.data(), (TUint)aFile.size())) == Mpeg4CencKind::Other);                    // the element as it was: not its stream
    TEST(Mpeg4CencRecognise(Brn(aFile.data(), (TUint)aFile.size()), true) == Mpeg4CencKind::Flac);
    TEST(Mpeg4CencRecognise(Brn(aFile.data(), (TUint)aInitBytes - 1), true) == Mpeg4CencKind::NeedMore);
    Keys keys;
    keys.iKeys[aKid] = aKey;
    Mpeg4CencBatchDecoder narrow(keys);
    narrow.Push(Brn(aFile.data(), (TUint)aFile.size()));
    TEST(narrow.HeadRead() && narrow.Kind() == Mpeg4CencKind::Other && !narrow.AllSchemes() && keys.iCalls == 0);
    const TUint steps[] = {3, 1, 2, 5, 7, 11, 13, 1, 1, 40, 17, 60, 200, 1, 333};
    Mpeg4CencBatchDecoder d(keys, true);
    size_t at = 0, k = 0;
    while (at < aFile.size()) {
        TEST(d.HeadRead() == (at >= aInitBytes) && d.Kind() == (at >= aInitBytes ? Mpeg4CencKind::Flac : Mpeg4CencKind::NeedMore));
        TEST(keys.iCalls == (at >= aInitBytes ? 1u : 0u) && d.HaveKey() == (at >= aInitBytes));
        const size_t n = std::min<size_t>(steps[k++ % (sizeof(steps) / sizeof(steps[0]))], aFile.size() - at);
        d.Push(Brn(aFile.data() + at, (TUint)n));
        at += n;
    }
    TEST(d.AllSchemes() && d.Protected() && d.Head().scheme == OHGPU_CBCS_SCHEME_CBCS && memcmp(d.Head().kid, aKid.data(), 16) == 0 && keys.iCalls == 1);
    TEST(d.WideHead().crypt_blocks == aCrypt && d.WideHead().skip_blocks == aSkip && d.WideHead().constant_iv_size == aConstantIv);
    TEST(memcmp(&d.WideHead().cenc, &d.Head(), sizeof(ohgpu_cenc_stream_result)) == 0);
}

struct LaneSpec {
    std::vector<TByte> file, want, kid;
    int throws, wide;
};

static void TestPipeline(MsgFactory& f, const std::string& aManifest)
{
    std::vector<LaneSpec> specs;
    Keys keys;
    std::ifstream in(aManifest);
    for (std::string line; std::getline(in, line); ) {
        std::istringstream ls(line);
        std::string file, want, kid, key;
        LaneSpec s;
        ls >> file >> want >> s.throws >> s.wide >> kid >> key;
        s.kid = Hex(kid);
        if (key != "-") keys.iKeys[s.kid] = Hex(key);
        s.file = ReadFile(file);
        s.want = ReadFile(want);
        specs.push_back(s);
    }
    TEST(specs.size() >= 5);
    std::vector<std::unique_ptr<Mpeg4CencBatchDecoder>> decoders;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<Mpeg4CencBatchDecoder::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    std::vector<TUint64> jiffies(specs.size(), 0);
    size_t ticks = 0, throwsSeen = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        decoders.emplace_back(new Mpeg4CencBatchDecoder(keys, specs[k].wide != 0));
        sinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerSecond));
        lanes.push_back({decoders[k].get(), controllers[k].get(), 0});
        ticks = std::max(ticks, (specs[k].file.size() + PIECE - 1) / PIECE);
    }
    ticks += 1;
    PlayableBatch batch(f);
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    for (size_t t = 0; t < ticks; t++) {
        TUint fresh[2][2] = {{0, 0}, {0, 0}};                                          // [family][codec]
        bool alacDecodes = false;
        for (size_t k = 0; k < specs.size(); k++) {
            const size_t lo = t * PIECE, hi = std::min(specs[k].file.size(), lo + PIECE);
            const TUint64 before = decoders[k]->WholeExtent();
            if (lo < hi && !decoders[k]->Corrupt()) decoders[k]->Push(Brn(specs[k].file.data() + lo, (TUint)(hi - lo)));
            if (!decoders[k]->HeadRead() || decoders[k]->Corrupt() || decoders[k]->WholeExtent() <= before) continue;
            if (decoders[k]->Kind() == Mpeg4CencKind::Flac) fresh[specs[k].wide][0] = 1;
            if (decoders[k]->Kind() == Mpeg4CencKind::Alac) fresh[specs[k].wide][1] = 1;
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls0, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        try {
            Mpeg4CencBatchDecoder::Flush(f, lanes.data(), lanes.size());
        } catch (CodecStreamFeatureUnsupported&) {
            throwsSeen++;
            for (size_t k = 0; k < specs.size(); k++) TEST(decoders[k]->Corrupt() == (specs[k].throws != 0 && decoders[k]->HeadRead()));
        }
        TEST(ohgpu_host_transfer_stats(f.Gpu(), &calls1, &srcCalls, &h2d, &d2h) == OHGPU_OK);
        for (size_t k = 0; k < specs.size(); k++) alacDecodes = alacDecodes || (decoders[k]->Kind() == Mpeg4CencKind::Alac && !sinks[k]->iAudio.empty());
        TEST(calls1 <= calls0 + fresh[0][0] + fresh[0][1] + fresh[1][0] + fresh[1][1] + (alacDecodes ? 1 : 0));      // one call a codec and family, one decode for the alac lanes
        std::vector<std::unique_ptr<ProcessorPcmBufTest>> procs;
        std::vector<size_t> laneOf;
        for (size_t k = 0; k < specs.size(); k++) {
            while (!sinks[k]->iAudio.empty()) {
                MsgAudioPcm* m = sinks[k]->iAudio.front();
                sinks[k]->iAudio.pop_front();
                TEST(m->TrackOffset() == jiffies[k]);
                jiffies[k] += m->Jiffies();
                MsgPlayable* p = m->CreatePlayable();
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
        if (got[k] != specs[k].want)
            printf("lane %zu: %zu bytes where %zu are due; next row %llu of %llu\n", k, got[k].size(), specs[k].want.size(), (unsigned long long)decoders[k]->NextRow(),
                   (unsigned long long)decoders[k]->RowsKnown());
        TEST(got[k] == specs[k].want);
        if (!specs[k].throws) TEST(sinks[k]->iStreams == 1 && decoders[k]->NextRow() == decoders[k]->RowsKnown() && !decoders[k]->Corrupt());
        if (specs[k].throws) TEST(got[k].empty() && decoders[k]->Corrupt());
        bytesChecked += got[k].size();
    }
    TEST(throwsSeen >= 1);
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", specs.size(), ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    if (argc < 9) { printf("usage: test_mpeg4_cbcs_decoder cpu|gpu cbcs.mp4 init-bytes kid-hex key-hex crypt skip constant-iv-bytes [manifest]\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    TestHead(ReadFile(argv[2]), (size_t)atol(argv[3]), Hex(argv[4]), Hex(argv[5]), (TUint)atoi(argv[6]), (TUint)atoi(argv[7]), (TUint)atoi(argv[8]));
    printf("cpu: %d checks\n", gChecks);
    if (gpu && argc > 9) {
        MsgFactory f(0);
        TestPipeline(f, argv[9]);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
