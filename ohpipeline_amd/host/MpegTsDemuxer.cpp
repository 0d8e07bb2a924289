// MpegTsDemuxer.cpp -- see MpegTsDemuxer.h
#include "MpegTsDemuxer.h"

#include <algorithm>
#include <cstring>

#include "DecodedAudioAggregator.h"

namespace OpenHome {
namespace Media {

TBool MpegTsRecognise(const Brx& aBytes) { return aBytes.Bytes() > 0 && aBytes.Ptr()[0] == 0x47; }

TBool AdtsRecognise(const Brx& aBytes, TUint* aStart)
{
    const TByte* p = aBytes.Ptr();
    const TUint n = aBytes.Bytes();
    for (TUint start = 0; start <= OHGPU_ADTS_RECOGNISE_LAST_START; start++) {
        TUint64 at = start;
        TUint k = 0;
        for (; k < OHGPU_ADTS_RECOGNISE_FRAMES; k++) {
            ohgpu_adts_frame f;
            if (at + 10 > n || ohgpu_adts_header(p + at, (size_t)(n - at), &f) != OHGPU_OK) break;
            at += f.bytes;
        }
        if (k == OHGPU_ADTS_RECOGNISE_FRAMES) {
            if (aStart) *aStart = start;
            return true;
        }
    }
    return false;
}

TUint64 Id3v2Skip(const Brx& aBytes) { return ohgpu_id3v2_skip(aBytes.Ptr(), aBytes.Bytes()); }

MpegTsAdtsBatchDemuxer::MpegTsAdtsBatchDemuxer(IAdtsFrameSink& aSink)
    : iSink(aSink), iEsBase(0), iFrames(0), iPmtPid(0), iAudioPid(0), iPesOpenBytes(0), iStatus(OHGPU_TS_OK), iRecognised(false), iCorrupt(false)
{
}

void MpegTsAdtsBatchDemuxer::Push(const Brx& aBytes)
{
    if (iCorrupt) return;                                              // (the stream ended at the corrupt packet, for every PID)
    iPending.insert(iPending.end(), aBytes.Ptr(), aBytes.Ptr() + aBytes.Bytes());
}

void MpegTsAdtsBatchDemuxer::Collect(TUint64 aSrcBase, TUint64 aDstBase, TUint aPesFirst, TUint aFrameFirst, ohgpu_ts_stream_desc& aTs, ohgpu_adts_stream_desc& aAdts) const
{
    const TUint packets = PendingPackets();
    memset(&aTs, 0, sizeof(aTs));
    memset(&aAdts, 0, sizeof(aAdts));
    aTs.src_offset = aSrcBase;
    aTs.src_bytes = packets * OHGPU_TS_PACKET_BYTES;
    aTs.dst_offset = aDstBase + iKept.size();
    aTs.dst_capacity = (TUint64)packets * 184u;
    aTs.flags = iPesOpenBytes ? OHGPU_TS_PES_OPEN : 0u;
    aTs.pmt_pid = iPmtPid; aTs.audio_pid = iAudioPid; aTs.pes_open_bytes = iPesOpenBytes;
    aTs.pes_first = aPesFirst; aTs.pes_capacity = packets;            // (a PES packet has a packet at least)
    aAdts.src_offset = aDstBase;
    aAdts.flags = iRecognised ? 0u : OHGPU_ADTS_RECOGNISE;
    aAdts.frame_first = aFrameFirst;
    aAdts.frame_capacity = (TUint)((iKept.size() + (TUint64)packets * 184u) / 7u) + 1u;   // (a frame has seven bytes at least)
}

void MpegTsAdtsBatchDemuxer::Apply(const ohgpu_ts_stream_result& aTs, const ohgpu_ts_pes* aPes, const ohgpu_adts_stream_result& aAdts, const ohgpu_adts_frame* aFrames,
                                   const TByte* aEs)
{
    const TUint packets = PendingPackets();
    const TUint64 runBase = iEsBase + iKept.size();                    // the elementary offset of this tick's run
    iStatus = aTs.status;
    iPmtPid = aTs.pmt_pid; iAudioPid = aTs.audio_pid; iPesOpenBytes = aTs.pes_open_bytes;
    if (aTs.status == OHGPU_TS_CORRUPT) iCorrupt = true;
    for (TUint k = 0; k < std::min<TUint>(aTs.pes_packets, packets); k++)
        if (!(aPes[k].flags & OHGPU_TS_PES_CONTINUATION)) iStamps.push_back(Stamp{runBase + aPes[k].es_offset, aPes[k].pts});
    const TUint64 total = iKept.size() + aTs.bytes_delivered;
    TUint64 consumed = 0;
    if (aAdts.status == OHGPU_ADTS_OK) {
        iRecognised = iRecognised || aAdts.frames > 0 || aAdts.bytes_consumed > 0;
        for (TUint k = 0; k < aAdts.frames; k++) {
            const ohgpu_adts_frame& f = aFrames[k];
            const TUint64 at = iEsBase + f.offset;
            while (iStamps.size() > 1 && iStamps[1].esOffset <= at) iStamps.pop_front();   // the last PES packet that begins at or in front of the frame
            const TUint64 pts = !iStamps.empty() && iStamps[0].esOffset <= at ? iStamps[0].pts : OHGPU_TS_NO_PTS;
            iSink.OutputAdtsFrame(at, Brn(aEs + f.offset, f.bytes), f, pts);
            iFrames++;
        }
        consumed = aAdts.bytes_consumed;
    }
    std::vector<TByte> kept(aEs + consumed, aEs + total);
    iKept.swap(kept);
    iEsBase += consumed;
    if (iKept.size() > kMaxKeptBytes) iCorrupt = true;
    iPending.erase(iPending.begin(), iPending.begin() + (size_t)packets * OHGPU_TS_PACKET_BYTES);
    if (iCorrupt) iPending.clear();
}

void MpegTsAdtsBatchDemuxer::Tick(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_ts_stream_desc> ts(aCount);
    std::vector<ohgpu_adts_stream_desc> adts(aCount);
    std::vector<TUint64> dstBase(aCount);
    std::vector<TByte> src, dst;
    TUint nPes = 0, nFrames = 0;
    for (size_t i = 0; i < aCount; i++) {
        MpegTsAdtsBatchDemuxer& d = *aLanes[i].demuxer;
        const TUint64 srcBase = src.size();
        dstBase[i] = dst.size();
        d.Collect(srcBase, dstBase[i], nPes, nFrames, ts[i], adts[i]);
        src.insert(src.end(), d.iPending.begin(), d.iPending.begin() + ts[i].src_bytes);
        src.resize((src.size() + 15u) & ~(size_t)15u);
        dst.insert(dst.end(), d.iKept.begin(), d.iKept.end());
        dst.resize((dst.size() + ts[i].dst_capacity + 15u) & ~(size_t)15u);
        nPes += ts[i].pes_capacity;
        nFrames += adts[i].frame_capacity;
    }
    if (src.empty()) return;
    std::vector<ohgpu_ts_stream_result> tres(aCount);
    std::vector<ohgpu_adts_stream_result> ares(aCount);
    std::vector<ohgpu_ts_pes> pes(nPes ? nPes : 1);
    std::vector<ohgpu_adts_frame> frames(nFrames ? nFrames : 1);
    if (dst.empty()) dst.resize(16);
    const int err = ohgpu_ts_adts_process_host(aFactory.Gpu(), ts.data(), adts.data(), aCount, nPes, nFrames, src.data(), src.size(), dst.data(), dst.size(),
                                               tres.data(), pes.data(), ares.data(), frames.data());
    if (err != OHGPU_OK) THROW(CodecStreamCorrupt);
    TBool bad = false;
    for (size_t i = 0; i < aCount; i++) {
        MpegTsAdtsBatchDemuxer& d = *aLanes[i].demuxer;
        d.Apply(tres[i], pes.data() + ts[i].pes_first, ares[i], frames.data() + adts[i].frame_first, dst.data() + dstBase[i]);
        bad = bad || d.iCorrupt;
    }
    if (bad) THROW(CodecStreamCorrupt);
}

} // namespace Media
} // namespace OpenHome
