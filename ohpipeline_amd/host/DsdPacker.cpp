// DsdPacker.cpp -- see DsdPacker.h.
#include "DsdPacker.h"

#include <algorithm>
#include <cstring>

#include "../../include/ohgpu.h"

namespace OpenHome {
namespace Media {

static uint8_t GpuKind(DsdPacker::EKind aKind)
{
    return aKind == DsdPacker::EKind::Dsf ? OHGPU_DSD_DSF : (aKind == DsdPacker::EKind::Dff ? OHGPU_DSD_DFF : OHGPU_DSD_RAW);
}

DsdPacker::DsdPacker(EKind aKind, TUint aSampleBlockWords, TUint aPadBytesPerChunk)
    : iKind(aKind)
    , iSampleBlockWords(aSampleBlockWords)
    , iPadBytesPerChunk(aPadBytesPerChunk)
    , iChunksPerBlock(aSampleBlockWords - aPadBytesPerChunk)
{
    uint64_t src = 0, dst = 0;                                        // the library's own rule for (W, P)
    ASSERT(ohgpu_dsd_layout(GpuKind(aKind), aSampleBlockWords, aPadBytesPerChunk, 0, &src, &dst) == OHGPU_OK);
    // a DSF run is converted from the first chunk of a plane pair: runs must end where pairs do
    ASSERT(aKind != EKind::Dsf || kDsfPairChunks % iChunksPerBlock == 0);
}

void DsdPacker::Push(const Brx& aFileBytes)
{
    ASSERT(!iDraining);
    iPending.insert(iPending.end(), aFileBytes.Ptr(), aFileBytes.Ptr() + aFileBytes.Bytes());
}

void DsdPacker::SetStreamChunks(TUint64 aChunks)
{
    ASSERT(iKind == EKind::Dsf);
    iStreamChunks = aChunks;
}

void DsdPacker::Drain()
{
    iDraining = true;
    if (iKind == EKind::Raw) {
        // DsdFiller.cpp:52-65: the last input block is completed with silence before it is padded
        const size_t blockBytes = (size_t)iChunksPerBlock * 4;
        iPending.resize((iPending.size() + blockBytes - 1) / blockBytes * blockBytes, OHGPU_DSD_SILENCE_BYTE);
    }
}

TUint DsdPacker::ConvertibleChunks() const
{
    TUint64 chunks;
    if (iKind == EKind::Dsf) {
        chunks = (TUint64)(iPending.size() / (2 * kDsfPlaneBytes)) * kDsfPairChunks;   // whole pairs only: a chunk needs both planes
        chunks = std::min<TUint64>(chunks, iStreamChunks - std::min(iStreamChunks, iChunksOut));
        if (!iDraining && chunks % kDsfPairChunks != 0) chunks -= chunks % kDsfPairChunks;   // (the stream's end lies in this pair: wait for Drain)
    }
    else {
        chunks = iPending.size() / 4;
        if (!iDraining) chunks -= chunks % iChunksPerBlock;           // whole sample blocks while the stream runs
    }
    return (TUint)chunks;
}

TUint DsdPacker::SourceBytes(TUint aChunks) const
{
    if (iKind == EKind::Dsf) {
        return (aChunks + kDsfPairChunks - 1) / kDsfPairChunks * 2 * kDsfPlaneBytes;
    }
    return aChunks * 4;
}

void DsdPacker::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_dsd_desc> descs;
    std::vector<size_t> laneOf;
    TUint64 srcTotal = 0, dstTotal = 0;
    for (size_t k = 0; k < aCount; k++) {
        DsdPacker& p = *aLanes[k].packer;
        ASSERT(aLanes[k].channels == 2);                              // the packers are stereo (DsdDsf.cpp:483)
        const TUint chunks = p.ConvertibleChunks();
        if (chunks == 0) {
            continue;
        }
        ohgpu_dsd_desc d;
        memset(&d, 0, sizeof(d));
        uint64_t srcBytes = 0, dstBytes = 0;
        ASSERT(ohgpu_dsd_layout(GpuKind(p.iKind), p.iSampleBlockWords, p.iPadBytesPerChunk, chunks, &srcBytes, &dstBytes) == OHGPU_OK);
        ASSERT(srcBytes == p.SourceBytes(chunks));
        d.kind = GpuKind(p.iKind);
        d.sample_block_words = (uint8_t)p.iSampleBlockWords;
        d.pad_bytes_per_chunk = (uint8_t)p.iPadBytesPerChunk;
        d.n_chunks = chunks;
        d.src_offset = srcTotal;                                      // 16-byte aligned, both: the wide path
        d.dst_offset = dstTotal;
        srcTotal += (srcBytes + 15u) & ~(TUint64)15u;
        dstTotal += (dstBytes + 15u) & ~(TUint64)15u;
        descs.push_back(d);
        laneOf.push_back(k);
    }
    if (descs.empty()) {
        return;
    }
    TByte* src = nullptr;
    TByte* dst = nullptr;
    aFactory.ReserveArena((size_t)srcTotal, (size_t)dstTotal, src, dst);
    for (size_t i = 0; i < descs.size(); i++) {
        const DsdPacker& p = *aLanes[laneOf[i]].packer;
        memcpy(src + descs[i].src_offset, p.iPending.data(), p.SourceBytes(descs[i].n_chunks));
    }
    const int err = ohgpu_dsd_process_host(aFactory.Gpu(), descs.data(), descs.size(), src, srcTotal, dst, dstTotal);
    ASSERT(err == OHGPU_OK);
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        DsdPacker& p = *lane.packer;
        uint64_t dstBytes = 0;
        (void)ohgpu_dsd_layout(descs[i].kind, p.iSampleBlockWords, p.iPadBytesPerChunk, descs[i].n_chunks, nullptr, &dstBytes);
        lane.trackOffset += lane.controller->OutputAudioDsd(Brn(dst + descs[i].dst_offset, (TUint)dstBytes), lane.channels, lane.sampleRate,
                                                            p.iSampleBlockWords, lane.trackOffset, p.iPadBytesPerChunk);
        p.iPending.erase(p.iPending.begin(), p.iPending.begin() + p.SourceBytes(descs[i].n_chunks));
        p.iChunksOut += descs[i].n_chunks;
    }
}

} // namespace Media
} // namespace OpenHome
