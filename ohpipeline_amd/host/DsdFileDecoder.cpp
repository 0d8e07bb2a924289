// DsdFileDecoder.cpp -- see DsdFileDecoder.h.
#include "DsdFileDecoder.h"

#include <algorithm>
#include <cstring>

#include "Ramp.h"

namespace OpenHome {
namespace Media {

TBool DsfRecognise(const Brx& aBytes) { return aBytes.Bytes() >= 4 && memcmp(aBytes.Ptr(), "DSD ", 4) == 0; }
TBool DffRecognise(const Brx& aBytes)
{
    return aBytes.Bytes() >= 16 && memcmp(aBytes.Ptr(), "FRM8", 4) == 0 && memcmp(aBytes.Ptr() + 12, "DSD ", 4) == 0;
}

DsdFileBatchDecoder::DsdFileBatchDecoder(TUint aSampleBlockWords, TUint aPadBytesPerChunk)
    : iSampleBlockWords(aSampleBlockWords), iPadBytesPerChunk(aPadBytesPerChunk), iChunksPerBlock(aSampleBlockWords - aPadBytesPerChunk)
    , iNextChunk(0), iEnded(false), iAnnounced(false), iDropped(false)
{
    uint64_t src = 0, dst = 0;                                        // the library's own rule for (W, P)
    ASSERT(ohgpu_dsd_layout(OHGPU_DSD_DFF, aSampleBlockWords, aPadBytesPerChunk, 0, &src, &dst) == OHGPU_OK);
    memset(&iResult, 0, sizeof(iResult));
}

void DsdFileBatchDecoder::Push(const Brx& aFileBytes)
{
    ASSERT(iFile.size() + aFileBytes.Bytes() < 0x80000000ull);
    iFile.insert(iFile.end(), aFileBytes.Ptr(), aFileBytes.Ptr() + aFileBytes.Bytes());
}

ohgpu_dsd_file_stream_result DsdFileBatchDecoder::Head() const
{
    ohgpu_dsd_file_stream_result r;
    const int err = ohgpu_dsd_file_head(iFile.data(), iFile.size(), iSampleBlockWords, iPadBytesPerChunk, &r);
    ASSERT(err == OHGPU_OK);
    return r;
}

void DsdFileBatchDecoder::Announce(CodecController& aController, TUint64 aSampleStart)
{
    const ohgpu_dsd_file_stream_result& r = iResult;
    const TUint64 length = r.sample_count * Jiffies::PerSample(r.sample_rate);
    aController.OutputDecodedStreamDsd(r.sample_rate, r.channels, Brn((const TByte*)"DSD", 3), length, aSampleStart);
}

TBool DsdFileBatchDecoder::TrySeek(Lane& aLane, TUint64 aSample)
{
    DsdFileBatchDecoder& d = *aLane.decoder;
    if (!d.iAnnounced || d.iDropped || aSample >= d.iResult.sample_count) return false;
    uint64_t first = 0, rounded = 0;
    const int err = ohgpu_dsd_file_seek(d.iResult.kind, aSample, &first, &rounded);
    ASSERT(err == OHGPU_OK);
    d.iNextChunk = first;
    // (the reference's own two formulas: a DSF offset in whole jiffies a sample, a DFF offset through the second)
    aLane.trackOffset = d.iResult.kind == OHGPU_DSD_FILE_KIND_DSF ? rounded * Jiffies::PerSample(d.iResult.sample_rate)
                                                                  : rounded * Jiffies::kPerSecond / d.iResult.sample_rate;
    d.Announce(*aLane.controller, rounded);
    return true;
}

void DsdFileBatchDecoder::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_dsd_file_stream_desc> descs;
    std::vector<size_t> laneOf;
    std::vector<TByte> src;
    TUint64 room = 0;
    for (size_t k = 0; k < aCount; k++) {
        DsdFileBatchDecoder& d = *aLanes[k].decoder;
        if (d.iDropped || d.iFile.empty()) continue;
        if (!d.iAnnounced) {                                                  // what needs no device is settled without one
            const ohgpu_dsd_file_stream_result head = d.Head();
            if (head.status == OHGPU_DSD_FILE_TRUNCATED && !d.iEnded) continue;   // its chunks have not all arrived
            if (head.status == OHGPU_DSD_FILE_NOT_DSD && (d.iFile.size() >= 16 || d.iEnded)) {
                d.iResult = head;
                d.iDropped = true;                                            // not recognised
                continue;
            }
            if (head.status == OHGPU_DSD_FILE_NOT_DSD) continue;              // fewer than sixteen bytes so far
        }
        ohgpu_dsd_file_stream_desc s;
        memset(&s, 0, sizeof(s));
        s.src_offset = src.size();
        s.src_bytes = (uint32_t)d.iFile.size();
        s.dst_offset = room;
        // (the audio is no larger than the file it lies in: its chunks, and a block for the last one's fill)
        s.dst_bytes_capacity = (d.iFile.size() / 4u / d.iChunksPerBlock + 1u) * d.iSampleBlockWords * 4u;
        s.chunk_first = d.iNextChunk;
        s.sample_block_words = d.iSampleBlockWords;
        s.pad_bytes_per_chunk = d.iPadBytesPerChunk;
        src.insert(src.end(), d.iFile.begin(), d.iFile.end());
        src.resize((src.size() + 15u) & ~(size_t)15u, 0);
        room = (room + s.dst_bytes_capacity + 15u) & ~(TUint64)15u;
        descs.push_back(s);
        laneOf.push_back(k);
    }
    if (descs.empty()) return;
    std::vector<ohgpu_dsd_file_stream_result> results(descs.size());
    std::vector<TByte> blocks((size_t)room);
    const int err = ohgpu_dsd_file_process_host(aFactory.Gpu(), descs.data(), descs.size(), src.data(), src.size(), blocks.data(), blocks.size(), results.data());
    ASSERT(err == OHGPU_OK);
    int firstBad = 0;                                                         // 1: corrupt, 2: unsupported
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        DsdFileBatchDecoder& d = *lane.decoder;
        const ohgpu_dsd_file_stream_result& r = results[i];
        if (r.status == OHGPU_DSD_FILE_TRUNCATED && !d.iEnded) continue;
        if (r.status != OHGPU_DSD_FILE_OK) {
            d.iResult = r;
            d.iDropped = true;
            if (!firstBad && r.status != OHGPU_DSD_FILE_NOT_DSD) firstBad = r.status == OHGPU_DSD_FILE_UNSUPPORTED ? 2 : 1;
            continue;
        }
        d.iResult = r;
        if (!d.iAnnounced) {
            d.iAnnounced = true;
            d.Announce(*lane.controller, 0);
        }
        if (r.bytes_written) {
            lane.trackOffset += lane.controller->OutputAudioDsd(Brn(blocks.data() + descs[i].dst_offset, (TUint)r.bytes_written), r.channels, r.sample_rate,
                                                                d.iSampleBlockWords, lane.trackOffset, d.iPadBytesPerChunk);
        }
        d.iNextChunk += r.chunks_written;
    }
    if (firstBad == 2) THROW(CodecStreamFeatureUnsupported);
    if (firstBad == 1) THROW(CodecStreamCorrupt);
}

} // namespace Media
} // namespace OpenHome
