// DsdPcmConverter.cpp -- see DsdPcmConverter.h.
#include "DsdPcmConverter.h"

#include <algorithm>
#include <cstring>

#include "../../include/ohgpu.h"

namespace OpenHome {
namespace Media {

DsdPcmFilter::DsdPcmFilter(MsgFactory& aFactory, TUint aDsdRate, TUint aPcmRate, TUint aTapsPerOutput, double aBeta, double aPassHz,
                           double aGain)
    : iFactory(aFactory)
    , iDsdRate(aDsdRate)
    , iPcmRate(aPcmRate)
    , iTaps(aTapsPerOutput)
    , iDecimation(0)
    , iHandle(nullptr)
{
    uint32_t decimation = 0;
    ASSERT(ohgpu_dsd_pcm_design(aDsdRate, aPcmRate, aTapsPerOutput, aBeta, aPassHz, aGain, nullptr, 0, &decimation) == OHGPU_OK);
    iDecimation = decimation;
    iCoef.resize((size_t)decimation * aTapsPerOutput);
    ASSERT(ohgpu_dsd_pcm_design(aDsdRate, aPcmRate, aTapsPerOutput, aBeta, aPassHz, aGain, iCoef.data(), iCoef.size(), &decimation) == OHGPU_OK);
    if (aFactory.HasGpu()) {
        ASSERT(ohgpu_dsd_pcm_create(aFactory.Gpu(), iDecimation, iTaps, iCoef.data(), &iHandle) == OHGPU_OK);
    }
}

DsdPcmFilter::~DsdPcmFilter()
{
    if (iHandle != nullptr) {
        (void)ohgpu_dsd_pcm_destroy(iFactory.Gpu(), iHandle);
    }
}

DsdPcmConverter::DsdPcmConverter(const DsdPcmFilter& aFilter, TUint aSampleBlockWords, TUint aPadBytesPerChunk)
    : iFilter(aFilter)
    , iSampleBlockWords(aSampleBlockWords)
    , iPadBytesPerChunk(aPadBytesPerChunk)
    , iChunkBytes(4 + aPadBytesPerChunk)
{
    uint64_t src = 0, dst = 0;                                        // the library's own rule for (W, P)
    ASSERT(ohgpu_dsd_layout(OHGPU_DSD_PASS, aSampleBlockWords, aPadBytesPerChunk, 0, &src, &dst) == OHGPU_OK);
}

void DsdPcmConverter::Push(const Brx& aDsd)
{
    ASSERT(aDsd.Bytes() % iChunkBytes == 0);
    iPending.insert(iPending.end(), aDsd.Ptr(), aDsd.Ptr() + aDsd.Bytes());
}

TUint DsdPcmConverter::ConvertibleFrames() const
{
    // frame m is whole once bit (m + 1) * D - 1 is in: 16 bits a chunk
    const TUint64 frames = (iChunk0 + ChunksHeld()) * 16 / iFilter.Decimation();
    return (TUint)(frames - std::min(frames, iFramesOut));
}

TBool DsdPcmConverter::Window(TUint64& aLo, TUint64& aHi) const
{
    const TUint frames = ConvertibleFrames();
    if (frames == 0) {
        return false;
    }
    uint64_t lo = 0, hi = 0;
    ASSERT(ohgpu_dsd_pcm_window(iFramesOut, frames, iFilter.Decimation(), iFilter.TapsPerOutput(), &lo, &hi) == OHGPU_OK);
    ASSERT(lo >= iChunk0 && hi <= iChunk0 + ChunksHeld());            // the history was kept
    aLo = lo;
    aHi = hi;
    return true;
}

void DsdPcmConverter::Deliver(Lane& aLane, const TByte* aPcm, TUint aFrames)
{
    DsdPcmConverter& c = *aLane.converter;
    const DsdPcmFilter& f = c.iFilter;
    if (!c.iAnnounced) {
        static const TByte kName[] = {'D', 'S', 'D'};
        aLane.controller->OutputDecodedStream(f.PcmRate() * kBitDepth * kChannels, kBitDepth, f.PcmRate(), kChannels, Brn(kName, sizeof(kName)), 0, 0, true);
        c.iAnnounced = true;
    }
    for (TUint done = 0; done < aFrames; ) {
        const TUint n = std::min(kPieceFrames, aFrames - done);
        aLane.trackOffset += aLane.controller->OutputAudioPcm(Brn(aPcm + (size_t)done * kFrameBytes, n * kFrameBytes), kChannels, f.PcmRate(), kBitDepth,
                                                              AudioDataEndian::Big, aLane.trackOffset);
        done += n;
    }
    c.iFramesOut += aFrames;
    // the next frame's oldest bit is (iFramesOut + 1) * D - N: chunks before its chunk are history nobody reads
    const TUint64 D = f.Decimation(), N = D * f.TapsPerOutput(), next = (c.iFramesOut + 1) * D;
    const TUint64 keepFrom = std::min<TUint64>(next > N ? (next - N) / 16 : 0, c.iChunk0 + c.ChunksHeld());
    if (keepFrom > c.iChunk0) {
        c.iPending.erase(c.iPending.begin(), c.iPending.begin() + (size_t)(keepFrom - c.iChunk0) * c.iChunkBytes);
        c.iChunk0 = keepFrom;
    }
}

void DsdPcmConverter::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_dsd_pcm_msg_desc> descs;
    std::vector<size_t> laneOf;
    const DsdPcmFilter* filter = nullptr;
    TUint64 srcTotal = 0, dstTotal = 0;
    for (size_t k = 0; k < aCount; k++) {
        const DsdPcmConverter& c = *aLanes[k].converter;
        uint64_t lo = 0, hi = 0;
        if (!c.Window(lo, hi)) {
            continue;
        }
        ASSERT(filter == nullptr || filter == &c.iFilter);            // one filter per call
        filter = &c.iFilter;
        ohgpu_dsd_pcm_msg_desc d;
        memset(&d, 0, sizeof(d));
        d.src_offset = srcTotal;
        d.src_chunk0 = lo;                                            // only the window crosses the link
        d.src_chunks = hi - lo;
        d.out_frame0 = c.iFramesOut;
        d.dst_offset = dstTotal;
        d.n_frames = c.ConvertibleFrames();
        d.sample_block_words = (uint8_t)c.iSampleBlockWords;
        d.pad_bytes_per_chunk = (uint8_t)c.iPadBytesPerChunk;
        d.dst_endian = OHGPU_ENDIAN_BIG;
        srcTotal += MsgFactory::ArenaShare(d.src_chunks * c.iChunkBytes);
        dstTotal += MsgFactory::ArenaShare((TUint64)d.n_frames * kFrameBytes);
        descs.push_back(d);
        laneOf.push_back(k);
    }
    if (descs.empty()) {
        return;
    }
    ASSERT(filter->Handle() != nullptr);                              // (a control-plane factory converts nothing)
    TByte* src = nullptr;
    TByte* dst = nullptr;
    aFactory.ReserveArena((size_t)srcTotal, (size_t)dstTotal, src, dst);
    for (size_t i = 0; i < descs.size(); i++) {
        const DsdPcmConverter& c = *aLanes[laneOf[i]].converter;
        memcpy(src + descs[i].src_offset, c.iPending.data() + (size_t)(descs[i].src_chunk0 - c.iChunk0) * c.iChunkBytes,
               (size_t)descs[i].src_chunks * c.iChunkBytes);
    }
    const int err = ohgpu_dsd_pcm_process_host(aFactory.Gpu(), filter->Handle(), descs.data(), descs.size(), src, srcTotal, dst, dstTotal);
    ASSERT(err == OHGPU_OK);
    for (size_t i = 0; i < descs.size(); i++) {
        Deliver(aLanes[laneOf[i]], dst + descs[i].dst_offset, descs[i].n_frames);
    }
}

} // namespace Media
} // namespace OpenHome
