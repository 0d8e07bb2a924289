// test_mpeg4_cenc_decoder.cpp -- protected fragmented MPEG-4 in the host adapter (ohpipeline_amd/host/Mpeg4CencDecoder.h:
// Mpeg4CencRecognise, Mpeg4CencBatchDecoder, ICencKeyProvider), in the shape of tests/cpp/test_mpeg4_fragment_decoder.cpp.
// `test_mpeg4_cenc_decoder cpu <flac.mp4> <init-bytes> <alac.mp4> <init-bytes> <plain.m4a> <kid-hex> <key-hex>` runs what needs no
// device: the recognition over every prefix round the end of `moov` of a protected fLaC and a protected alac stream, the peek over
// ragged pushes (the head is read exactly when the stated byte has arrived, and the provider is asked exactly then, ONCE, by the
// head's kid), a provider that lacks the key, the refusals.
// `test_mpeg4_cenc_decoder gpu ... <manifest>` adds the whole path: per line of the manifest one lane -- a stream, the bytes that must
// reach the processor, what it must throw (0 nothing, 2 CodecStreamFeatureUnsupported), a seek as in the sibling's manifest, and the
// lane's kid and key in hex ("-": the provider has no key for that kid) -- pushed in PIECE-byte pieces over as many ticks as it takes,
// ONE Flush per tick for all lanes, every message read through a playable into ProcessorPcmBufTest.  The expectations are made by
// tests/test_cenc_host_cpp.py from the PCM the fixtures were encoded from.
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
#define TEST_THROWS(expr, Exc) do { bool thrown_ = false; try { expr; } catch (Exc&) { thrown_ = true; } gChecks++; \
    if (!thrown_) { gFailures++; printf("FAILED %s:%d  %s did not throw\n", __FILE__, __LINE__, #expr); } } while (0)
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

// the provider: the keys it has, by kid; every question is counted
class Keys : public ICencKeyProvider {
public:
    TBool Key(const Brx& aKid, Bwx& aKey16) override
    {
        iCalls++;
        const std::vector<TByte> kid(aKid.Ptr(), aKid.Ptr() + aKid.Bytes());
        iAsked[kid]++;
        const auto it = iKeys.find(kid);
        if (it == iKeys.end() || aKey16.MaxBytes() < 16) return false;
        aKey16.Replace(Brn(it->second.data(), 16));
        return true;
    }
    std::map<std::vector<TByte>, std::vector<TByte>> iKeys;
    std::map<std::vector<TByte>, TUint> iAsked;
    TUint iCalls = 0;
};

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

static void TestRecognise(const std::vector<TByte>& aFile, size_t aInitBytes, Mpeg4CencKind aKind, const std::vector<TByte>& aPlain)
{
    TEST(Mpeg4CencRecognise(Brn(aFile.data(), 0)) == Mpeg4CencKind::NeedMore && Mpeg4CencRecognise(Brn(aFile.data(), 7)) == Mpeg4CencKind::NeedMore);
    for (size_t n = 8; n < aInitBytes; n += n + 40 < aInitBytes ? 37 : 1) TEST(Mpeg4CencRecognise(Brn(aFile.data(), (TUint)n)) == Mpeg4CencKind::NeedMore);
    TEST(Mpeg4CencRecognise(Brn(aFile.data(), (TUint)aInitBytes)) == aKind && Mpeg4CencRecognise(Brn(aFile.data(), (TUint)aFile.size())) == aKind);
    TEST(Mpeg4CencRecognise(Brn(aPlain.data(), (TUint)aPlain.size())) == Mpeg4CencKind::Plain);
    const TByte riff[12] = {'R', 'I', 'F', 'F', 0, 0, 0, 0, 'W', 'A', 'V', 'E'};
    TEST(Mpeg4CencRecognise(Brn(riff, 12)) == Mpeg4CencKind::None && Mpeg4CencRecognise(Brn(riff, 8)) == Mpeg4CencKind::None);
}

static void TestPeek(const std::vector<TByte>& aFile, size_t aInitBytes, Mpeg4CencKind aKind, uint32_t aCodec, const std::vector<TByte>& aKid, const std::vector<TByte>& aKey)
{
    Keys keys, none;
    keys.iKeys[aKid] = aKey;
    // ragged pushes: the head is read exactly when byte aInitBytes - 1 has arrived; the whole extent never names a byte that has not
    const TUint steps[] = {3, 1, 2, 5, 7, 11, 13, 1, 1, 40, 17, 60, 200, 1, 333};
    Mpeg4CencBatchDecoder d(keys);
    size_t at = 0, k = 0;
    TUint64 last = 0;
    while (at < aFile.size()) {
        TEST(d.HeadRead() == (at >= aInitBytes) && d.Kind() == (at >= aInitBytes ? aKind : Mpeg4CencKind::NeedMore));
        TEST(keys.iCalls == (at >= aInitBytes ? 1u : 0u) && d.HaveKey() == (at >= aInitBytes) && d.Protected() == (at >= aInitBytes));
        const size_t n = std::min<size_t>(steps[k++ % (sizeof(steps) / sizeof(steps[0]))], aFile.size() - at);
        d.Push(Brn(aFile.data() + at, (TUint)n));
        at += n;
        TEST(d.BytesPushed() == at && d.WholeExtent() <= at && d.WholeExtent() >= last && !d.Corrupt());
        last = d.WholeExtent();
    }
    TEST(d.HeadRead() && d.WholeExtent() == aFile.size() && d.Head().mp4f.status == OHGPU_MP4F_OK && d.Head().mp4f.codec == aCodec && d.Head().mp4f.moov_offset < aInitBytes);
    TEST(d.Head().is_protected == 1 && d.Head().scheme == OHGPU_CENC_SCHEME && memcmp(d.Head().kid, aKid.data(), 16) == 0 && keys.iCalls == 1 && keys.iAsked[aKid] == 1);
    Mpeg4CencBatchDecoder keyless(none);                                              // a provider that lacks the key: asked once, the lane knows it has none
    keyless.Push(Brn(aFile.data(), (TUint)aFile.size()));
    TEST(keyless.HeadRead() && keyless.Protected() && !keyless.HaveKey() && none.iCalls == 1 && keyless.Kind() == aKind && !keyless.Corrupt());
    TUint64 first = 0;
    TEST(!d.TrySeek(0, first) && d.NextRow() == 0 && d.RowsKnown() == 0);             // (no rows before a Flush has read a fragment)
    Mpeg4CencBatchDecoder unread(keys);
    TEST_THROWS(unread.Head(), AssertionFailed);
}

static void TestRefusals()
{
    const TByte riff[12] = {'R', 'I', 'F', 'F', 0, 0, 0, 0, 'W', 'A', 'V', 'E'};
    Keys keys;
    { Mpeg4CencBatchDecoder x(keys); x.Push(Brn(riff, 7)); TEST(!x.Corrupt()); TEST_THROWS(x.Push(Brn(riff + 7, 1)), CodecStreamCorrupt); TEST(x.Corrupt()); }
    { Mpeg4CencBatchDecoder x(keys); TEST_THROWS(x.Push(Brn(riff, 12)), CodecStreamCorrupt); }
}

struct LaneSpec {
    std::vector<TByte> file, want;
    int throws;
    long long seekFrame, seekFirst, seekRow, seekFrom;
    std::vector<TByte> kid;
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
        ls >> file >> want >> s.throws >> s.seekFrame >> s.seekFirst >> s.seekRow >> s.seekFrom >> kid >> key;
        s.kid = Hex(kid);
        if (key != "-") keys.iKeys[s.kid] = Hex(key);
        s.file = ReadFile(file);
        s.want = ReadFile(want);
        specs.push_back(s);
    }
    TEST(specs.size() == 7);
    std::vector<std::unique_ptr<Mpeg4CencBatchDecoder>> decoders;
    std::vector<std::unique_ptr<Sink>> sinks;
    std::vector<std::unique_ptr<CodecController>> controllers;
    std::vector<Mpeg4CencBatchDecoder::Lane> lanes;
    std::vector<std::vector<TByte>> got(specs.size());
    std::vector<TUint64> jiffies(specs.size(), 0);
    std::vector<bool> sought(specs.size(), false);
    size_t ticks = 0, throwsSeen = 0, seeks = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        decoders.emplace_back(new Mpeg4CencBatchDecoder(keys));
        sinks.emplace_back(new Sink());
        controllers.emplace_back(new CodecController(f, *sinks[k], Jiffies::kPerSecond));
        lanes.push_back({decoders[k].get(), controllers[k].get(), 0});
        ticks = std::max(ticks, (specs[k].file.size() + PIECE - 1) / PIECE);
    }
    ticks += 2;                                                                      // (a lane that seeks in its last tick is served in the next)
    PlayableBatch batch(f);
    uint64_t calls0 = 0, calls1 = 0, srcCalls = 0, h2d = 0, d2h = 0;
    for (size_t t = 0; t < ticks; t++) {
        bool flac = false, alac = false, alacDecodes = false;
        for (size_t k = 0; k < specs.size(); k++) {
            const size_t lo = t * PIECE, hi = std::min(specs[k].file.size(), lo + PIECE);
            const TUint64 before = decoders[k]->WholeExtent();
            if (lo < hi && !decoders[k]->Corrupt()) decoders[k]->Push(Brn(specs[k].file.data() + lo, (TUint)(hi - lo)));
            const bool fresh = decoders[k]->HeadRead() && !decoders[k]->Corrupt() && (decoders[k]->WholeExtent() > before || (sought[k] && t > 0));
            flac = flac || (fresh && decoders[k]->Kind() == Mpeg4CencKind::Flac);
            alac = alac || (fresh && decoders[k]->Kind() == Mpeg4CencKind::Alac);
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
        TEST(calls1 <= calls0 + (flac ? 1 : 0) + (alac ? 1 : 0) + (alacDecodes ? 1 : 0));      // at most one call a codec for the fragments, one decode for the alac lanes
        for (size_t k = 0; k < specs.size(); k++) {
            if (specs[k].seekFrame < 0 || sought[k] || decoders[k]->WholeExtent() < (TUint64)specs[k].seekFrom) continue;
            TUint64 first = 0;
            TEST(decoders[k]->TrySeek((TUint64)specs[k].seekFrame, first) && first == (TUint64)specs[k].seekFirst);
            TEST(decoders[k]->NextRow() == (TUint64)specs[k].seekRow);
            if (decoders[k]->Kind() == Mpeg4CencKind::Alac) TEST(decoders[k]->Alac().NextPacket() == (TUint64)specs[k].seekRow);
            const TUint64 row = decoders[k]->NextRow();
            TEST(!decoders[k]->TrySeek(1ull << 40, first) && decoders[k]->NextRow() == row);
            sought[k] = true;
            seeks++;
        }
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
        TEST(got[k].size() == specs[k].want.size());
        TEST(got[k] == specs[k].want);
        if (!specs[k].throws) TEST(sinks[k]->iStreams == 1 && sinks[k]->iStreamBeforeAudio && decoders[k]->NextRow() == decoders[k]->RowsKnown() && !decoders[k]->Corrupt());
        if (specs[k].throws) TEST(got[k].empty() && decoders[k]->Corrupt());
        TEST(lanes[k].trackOffset == jiffies[k]);
        bytesChecked += got[k].size();
    }
    TEST(throwsSeen == 1 && seeks == 2);
    TUint protectedLanes = 0;
    for (size_t k = 0; k < specs.size(); k++) {
        if (!decoders[k]->Protected()) continue;
        protectedLanes++;
        TEST(decoders[k]->HaveKey() == (specs[k].throws == 0));
    }
    TEST(protectedLanes == 6 && keys.iCalls == protectedLanes);                     // the key is asked for once a lane, by its kid
    for (const auto& asked : keys.iAsked) TEST(asked.second >= 1);
    printf("pipeline: %zu lanes, %zu ticks, %zu bytes byte-exact\n", specs.size(), ticks, bytesChecked);
}

int main(int argc, char** argv)
{
    if (argc < 9) { printf("usage: test_mpeg4_cenc_decoder cpu|gpu flac.mp4 init-bytes alac.mp4 init-bytes plain.m4a kid-hex key-hex [manifest]\n"); return 2; }
    const bool gpu = strcmp(argv[1], "gpu") == 0;
    const std::vector<TByte> flac = ReadFile(argv[2]), alac = ReadFile(argv[4]), plain = ReadFile(argv[6]);
    TestRecognise(flac, (size_t)atol(argv[3]), Mpeg4CencKind::Flac, plain);
    TestRecognise(alac, (size_t)atol(argv[5]), Mpeg4CencKind::Alac, plain);
    TestPeek(flac, (size_t)atol(argv[3]), Mpeg4CencKind::Flac, 0x664c6143u, Hex(argv[7]), Hex(argv[8]));
    TestPeek(alac, (size_t)atol(argv[5]), Mpeg4CencKind::Alac, 0x616c6163u, Hex(argv[7]), Hex(argv[8]));
    TestRefusals();
    printf("cpu: %d checks\n", gChecks);
    if (gpu && argc > 9) {
        MsgFactory f(0);
        TestPipeline(f, argv[9]);
    }
    printf("%s: %d checks, %d failures\n", gpu ? "gpu" : "cpu", gChecks, gFailures);
    return gFailures == 0 ? 0 : 1;
}
