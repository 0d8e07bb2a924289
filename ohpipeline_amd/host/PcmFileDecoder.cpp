// PcmFileDecoder.cpp -- see PcmFileDecoder.h.
#include "PcmFileDecoder.h"

#include <algorithm>
#include <cstring>

#include "Ramp.h"

namespace OpenHome {
namespace Media {

static TBool FormIs(const Brx& aBytes, const char* aForm, const char* aKind)
{
    return aBytes.Bytes() >= 12 && memcmp(aBytes.Ptr(), aForm, 4) == 0 && memcmp(aBytes.Ptr() + 8, aKind, 4) == 0;
}
TBool WavRecognise(const Brx& aBytes) { return FormIs(aBytes, "RIFF", "WAVE"); }
TBool AiffRecognise(const Brx& aBytes) { return FormIs(aBytes, "FORM", "AIFF"); }
TBool AifcRecognise(const Brx& aBytes) { return FormIs(aBytes, "FORM", "AIFC"); }

PcmFileBatchDecoder::PcmFileBatchDecoder(TUint aMaxBitDepth, TBool aWav8Unsigned)
    : iMaxBitDepth(aMaxBitDepth), iFlags(aWav8Unsigned ? OHGPU_IFF_FLAG_WAV8_UNSIGNED : 0u), iNextFrame(0), iEnded(false), iAnnounced(false), iDropped(false)
{
    ASSERT(aMaxBitDepth == 24 || aMaxBitDepth == 32);
    memset(&iResult, 0, sizeof(iResult));
}

void PcmFileBatchDecoder::Push(const Brx& aFileBytes)
{
    ASSERT(iFile.size() + aFileBytes.Bytes() < 0x80000000ull);
    iFile.insert(iFile.end(), aFileBytes.Ptr(), aFileBytes.Ptr() + aFileBytes.Bytes());
}

void PcmFileBatchDecoder::Announce(CodecController& aController)
{
    const ohgpu_iff_stream_result& r = iResult;
    const TUint64 length = r.frames_total * Jiffies::PerSample(r.sample_rate);
    const char* const name = r.kind == OHGPU_IFF_KIND_WAV ? "WAV" : "AIFF";          // (the reference names both AIFF kinds "AIFF")
    aController.OutputDecodedStream(r.bit_rate, r.out_bit_depth, r.sample_rate, r.channels, Brn((const TByte*)name, (TUint)strlen(name)), length, iNextFrame, true);
}

TBool PcmFileBatchDecoder::TrySeek(Lane& aLane, TUint64 aSample)
{
    PcmFileBatchDecoder& d = *aLane.decoder;
    if (!d.iAnnounced || d.iDropped) return false;
    if (d.iResult.frames_total != 0 && aSample >= d.iResult.frames_total) return false;      // (0: a continuous stream has no length to hold it to)
    d.iNextFrame = aSample;
    aLane.trackOffset = aSample * Jiffies::kPerSecond / d.iResult.sample_rate;
    d.Announce(*aLane.controller);
    return true;
}

void PcmFileBatchDecoder::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_iff_stream_desc> descs;
    std::vector<size_t> laneOf;
    std::vector<TByte> src;
    TUint64 room = 0;
    for (size_t k = 0; k < aCount; k++) {
        PcmFileBatchDecoder& d = *aLanes[k].decoder;
        if (d.iDropped || d.iFile.empty()) continue;
        ohgpu_iff_stream_desc s;
        memset(&s, 0, sizeof(s));
        s.src_offset = src.size();
        s.src_bytes = (uint32_t)d.iFile.size();
        s.flags = d.iFlags;
        s.dst_offset = room;
        s.dst_bytes_capacity = d.iFile.size();                                // (the audio is no larger than the file it lies in)
        s.dst_frame_capacity = s.src_bytes;
        s.frame_first = d.iNextFrame;
        s.max_bit_depth = d.iMaxBitDepth;
        src.insert(src.end(), d.iFile.begin(), d.iFile.end());
        src.resize((src.size() + 15u) & ~(size_t)15u, 0);
        room = (room + s.dst_bytes_capacity + 15u) & ~(TUint64)15u;
        descs.push_back(s);
        laneOf.push_back(k);
    }
    if (descs.empty()) return;
    std::vector<ohgpu_iff_stream_result> results(descs.size());
    std::vector<TByte> pcm((size_t)room);
    const int err = ohgpu_iff_process_host(aFactory.Gpu(), descs.data(), descs.size(), src.data(), src.size(), pcm.data(), pcm.size(), results.data());
    ASSERT(err == OHGPU_OK);
    int firstBad = 0;                                                         // 1: corrupt, 2: unsupported
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        PcmFileBatchDecoder& d = *lane.decoder;
        const ohgpu_iff_stream_result& r = results[i];
        if (r.status == OHGPU_IFF_TRUNCATED && !d.iEnded) continue;           // its chunks have not all arrived
        if (r.status != OHGPU_IFF_OK) {
            d.iResult = r;
            d.iDropped = true;
            if (!firstBad) firstBad = r.status == OHGPU_IFF_UNSUPPORTED ? 2 : 1;
            continue;
        }
        const ohgpu_iff_stream_result before = d.iResult;
        d.iResult = r;
        if (!d.iAnnounced) {
            d.iAnnounced = true;
            d.Announce(*lane.controller);
        } else {
            d.iResult.frames_total = before.frames_total;                     // (what was announced stands)
        }
        const TUint frame = r.channels * (r.out_bit_depth / 8u);
        const TUint64 bytes = r.frames_written * frame, piece = (TUint64)(DecodedAudio::kMaxBytes / frame) * frame;
        const TByte* p = pcm.data() + descs[i].dst_offset;
        for (TUint64 at = 0; at < bytes; at += piece) {
            const TUint n = (TUint)std::min<TUint64>(piece, bytes - at);
            lane.trackOffset += lane.controller->OutputAudioPcm(Brn(p + at, n), r.channels, r.sample_rate, r.out_bit_depth, AudioDataEndian::Big, lane.trackOffset);
        }
        d.iNextFrame += r.frames_written;
    }
    if (firstBad == 2) THROW(CodecStreamFeatureUnsupported);
    if (firstBad == 1) THROW(CodecStreamCorrupt);
}

} // namespace Media
} // namespace OpenHome
