// FlacDecoder.cpp -- see FlacDecoder.h.
#include "FlacDecoder.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Media {

FlacBatchDecoder::FlacBatchDecoder()
    : iInfoKnown(false), iAnnounced(false), iCorrupt(false), iNextSample(0)
{
    memset(&iInfo, 0, sizeof(iInfo));
}

void FlacBatchDecoder::Push(const Brx& aFileBytes)
{
    iPending.insert(iPending.end(), aFileBytes.Ptr(), aFileBytes.Ptr() + aFileBytes.Bytes());
    if (!iInfoKnown) {
        ReadMetadata();
    }
}

void FlacBatchDecoder::ReadMetadata()
{
    // what can be told from the first bytes is told at once; the rest waits until the library finds the metadata whole
    static const TByte kMagic[4] = {'f', 'L', 'a', 'C'};
    const size_t have = iPending.size();
    if (memcmp(iPending.data(), kMagic, std::min<size_t>(have, 4)) != 0 || (have > 4 && (iPending[4] & 0x7f) != 0)) {
        iCorrupt = true;
        THROW(CodecStreamCorrupt);
    }
    uint64_t audio = 0;
    if (ohgpu_flac_streaminfo(iPending.data(), have, &iInfo, &audio) != OHGPU_OK) {
        return;                                                       // (not all of it yet)
    }
    if (iInfo.bits != 8 && iInfo.bits != 16 && iInfo.bits != 24) {
        THROW(CodecStreamFeatureUnsupported);                         // Flac.cpp:404-406
    }
    iPending.erase(iPending.begin(), iPending.begin() + (size_t)audio);
    iInfoKnown = true;
}

void FlacBatchDecoder::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_flac_stream_desc> descs;
    std::vector<size_t> laneOf;
    TUint64 srcTotal = 0, dstTotal = 0, framesMax = 0;
    for (size_t k = 0; k < aCount; k++) {
        FlacBatchDecoder& d = *aLanes[k].decoder;
        if (!d.iInfoKnown || d.iCorrupt || d.iPending.empty()) {
            continue;
        }
        const ohgpu_flac_streaminfo_t& info = d.iInfo;
        ohgpu_flac_stream_desc s;
        memset(&s, 0, sizeof(s));
        // no frame is shorter than its header, a byte per subframe and the CRC-16: that bounds the samples these bytes can hold
        const TUint64 frames = d.iPending.size() / std::max<TUint64>(info.min_framesize, 7u + info.channels) + 1;
        TUint64 samples = std::min<TUint64>(frames * info.max_blocksize, kMaxSamplesPerTick);
        if (info.total_samples != 0) {
            samples = std::min<TUint64>(samples, info.total_samples - std::min<TUint64>(info.total_samples, d.iNextSample));
        }
        s.src_offset = srcTotal;
        s.src_bytes = d.iPending.size();
        s.dst_offset = dstTotal;
        s.first_sample = d.iNextSample;
        s.max_samples = (uint32_t)std::max<TUint64>(samples, info.max_blocksize);
        s.sample_rate = info.sample_rate;
        s.blocksize = info.min_blocksize == info.max_blocksize ? info.max_blocksize : 0;
        s.max_blocksize = info.max_blocksize;
        s.channels = info.channels;
        s.bits = info.bits;
        s.flags = OHGPU_FLAC_FLAG_AT_FRAME | OHGPU_FLAC_OUT_PACKED_BE;
        srcTotal += MsgFactory::ArenaShare(s.src_bytes);
        dstTotal += MsgFactory::ArenaShare((TUint64)s.max_samples * info.channels * (info.bits / 8));
        framesMax += frames;
        descs.push_back(s);
        laneOf.push_back(k);
    }
    if (descs.empty()) {
        return;
    }
    TByte* src = nullptr;
    TByte* dst = nullptr;
    aFactory.ReserveArena((size_t)srcTotal, (size_t)dstTotal, src, dst);
    for (size_t i = 0; i < descs.size(); i++) {
        const FlacBatchDecoder& d = *aLanes[laneOf[i]].decoder;
        memcpy(src + descs[i].src_offset, d.iPending.data(), d.iPending.size());
    }
    std::vector<ohgpu_flac_stream_result> results(descs.size());
    std::vector<ohgpu_flac_frame> frames((size_t)framesMax);
    size_t nFrames = 0;
    const int err = ohgpu_flac_process_host(aFactory.Gpu(), descs.data(), descs.size(), src, srcTotal, dst, dstTotal, results.data(),
                                            frames.data(), frames.size(), &nFrames);
    ASSERT(err == OHGPU_OK && nFrames <= frames.size());
    static const TByte kName[] = {'F', 'L', 'A', 'C'};
    size_t at = 0, firstBad = descs.size();
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        FlacBatchDecoder& d = *lane.decoder;
        const ohgpu_flac_streaminfo_t& info = d.iInfo;
        const TUint sampleBytes = (info.bits / 8u) * info.channels;
        if (!d.iAnnounced) {
            // Flac.cpp:427-441: bit rate = rate x depth x channels, lossless
            lane.controller->OutputDecodedStream(info.sample_rate * info.bits * info.channels, info.bits, info.sample_rate, info.channels,
                                                 Brn(kName, sizeof(kName)), info.total_samples * Jiffies::kPerSecond / info.sample_rate, 0, true);
            d.iAnnounced = true;
        }
        for (; at < nFrames && frames[at].stream == i; at++) {
            // Flac.cpp:379-417: a frame leaves in pieces of whole samples within kMaxPieceBytes, the count restarting with every frame
            const TByte* audio = dst + descs[i].dst_offset + (frames[at].first_sample - descs[i].first_sample) * sampleBytes;
            const TUint perPiece = PieceSamples(info.channels, info.bits);
            for (TUint done = 0; done < frames[at].blocksize; ) {
                const TUint n = std::min(perPiece, frames[at].blocksize - done);
                lane.trackOffset += lane.controller->OutputAudioPcm(Brn(audio + (size_t)done * sampleBytes, n * sampleBytes), info.channels, info.sample_rate,
                                                                    info.bits, AudioDataEndian::Big, lane.trackOffset);
                done += n;
            }
        }
        d.iNextSample += results[i].samples;
        d.iPending.erase(d.iPending.begin(), d.iPending.begin() + (size_t)results[i].bytes_consumed);
        // (OHGPU_FLAC_OVERFLOW is this tick's arena being full: the rest is the next tick's)
        if (results[i].status == OHGPU_FLAC_CORRUPT || results[i].status == OHGPU_FLAC_UNSUPPORTED) {
            d.iCorrupt = true;
            if (firstBad == descs.size()) firstBad = i;
        }
    }
    if (firstBad != descs.size()) {
        if (results[firstBad].status == OHGPU_FLAC_UNSUPPORTED) THROW(CodecStreamFeatureUnsupported);
        THROW(CodecStreamCorrupt);                                    // Flac.cpp:421-425
    }
}

} // namespace Media
} // namespace OpenHome
