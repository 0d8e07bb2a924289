// MpegTsDemuxer.h -- the container side of HLS audio and of plain .aac streams: transport bytes in, ADTS frames out, the packet walk,
// PAT / PMT, PES and the frame chain all on the device.
//
// Stands where these stand in the reference (file:line relative to the reference tree):
//   MpegTsContainer (MpegTs, MpegPes)    OpenHome/Media/Codec/MpegTs.cpp           188-byte packets -> PAT, PMT -> PES -> elementary bytes
//   MpegTsContainer::Recognise           OpenHome/Media/Codec/MpegTs.cpp           first byte 0x47, the whole test
//   CodecAacFdkAdts::Recognise, ProcessAdts   OpenHome/Media/Codec/AacFdkAdts.cpp:200-241   five headers in a row; header, frame, next header
//   Id3v2                                OpenHome/Media/Codec/Id3v2.cpp            the tag in front of HLS "packed audio"
// Shape of this implementation (host/OggFlacDecoder.h's): a demuxer is a byte queue.  Tick() takes every lane, lays the whole packets
// that have arrived into one arena and makes ONE fused device call (ohgpu_ts_adts_process_host).  pmt_pid, audio_pid and pes_open_bytes
// go from a tick's result to the next tick's descriptor.  Each tick's run is delivered right behind the elementary bytes the last
// tick's chain left unconsumed, so the elementary stream stays one contiguous run and the chain starts at bytes_consumed.  The frames
// leave through IAdtsFrameSink with the PTS of the PES record that holds their first byte (a search on the host).  No AAC is decoded.
#pragma once

#include <deque>
#include <vector>

#include "../../include/ohgpu.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

/** MpegTsContainer::Recognise's rule: the first byte is the sync byte. */
TBool MpegTsRecognise(const Brx& aBytes);
/** CodecAacFdkAdts::Recognise's rule on the host (ohgpu_adts_header along the chain): five valid headers in a row from a start in
 *  [0, 1001], each with 10 bytes present.  aStart: where. */
TBool AdtsRecognise(const Brx& aBytes, TUint* aStart = nullptr);
/** The bytes of the ID3v2 tags at the head of aBytes (ohgpu_id3v2_skip); 0: no tag. */
TUint64 Id3v2Skip(const Brx& aBytes);

class IAdtsFrameSink {
public:
    /** One frame, header included.  aEsOffset: of its first byte in the elementary stream since the demuxer began.  aPts: of the PES
     *  packet that holds that byte, or OHGPU_TS_NO_PTS. */
    virtual void OutputAdtsFrame(TUint64 aEsOffset, const Brx& aFrame, const ohgpu_adts_frame& aHeader, TUint64 aPts) = 0;
    virtual ~IAdtsFrameSink() {}
};

class MpegTsAdtsBatchDemuxer {
public:
    static const TUint kMaxKeptBytes = 1u << 20;        // elementary bytes without a frame: beyond this the stream is no ADTS stream
public:
    explicit MpegTsAdtsBatchDemuxer(IAdtsFrameSink& aSink);
    /** Transport bytes as they come, from a packet's first byte on.  Dropped once the stream is corrupt. */
    void Push(const Brx& aBytes);
    /** As MpegTsContainer::TrySeek: a transport stream is not seekable here. */
    TBool TrySeek(TUint aStreamId, TUint64 aOffset) { (void)aStreamId; (void)aOffset; return false; }
    TUint PendingBytes() const { return (TUint)iPending.size(); }      // transport bytes no Tick has taken yet
    TUint KeptBytes() const { return (TUint)iKept.size(); }            // elementary bytes behind the last frame
    TUint64 EsBytes() const { return iEsBase + iKept.size(); }          // elementary bytes delivered so far
    TUint64 Frames() const { return iFrames; }
    TUint PmtPid() const { return iPmtPid; }
    TUint AudioPid() const { return iAudioPid; }
    TUint PesOpenBytes() const { return iPesOpenBytes; }
    TUint Status() const { return iStatus; }                           // the last tick's OHGPU_TS_*
    TBool Recognised() const { return iRecognised; }
    TBool Corrupt() const { return iCorrupt; }

    struct Lane { MpegTsAdtsBatchDemuxer* demuxer; };
    /** One fused device call for all lanes.  A lane whose stream turns out corrupt (an adaptation field beyond its packet) or not to
     *  be ADTS delivers what precedes; once every lane has been served the first such lane's CodecStreamCorrupt is thrown. */
    static void Tick(MsgFactory& aFactory, Lane* aLanes, size_t aCount);

    /** The halves of Tick around the device call, apart so that a test can stand in for the device.  Collect: this lane's two
     *  descriptors; its packets lie at aSrcBase of the source arena (PendingPackets()), its kept bytes at aDstBase of the destination
     *  arena (Kept()) with room for the run behind them.  Apply: what the device answered; aEs = the destination arena at aDstBase. */
    void Collect(TUint64 aSrcBase, TUint64 aDstBase, TUint aPesFirst, TUint aFrameFirst, ohgpu_ts_stream_desc& aTs, ohgpu_adts_stream_desc& aAdts) const;
    TUint PendingPackets() const { return (TUint)(iPending.size() / OHGPU_TS_PACKET_BYTES); }
    const std::vector<TByte>& Pending() const { return iPending; }
    const std::vector<TByte>& Kept() const { return iKept; }
    void Apply(const ohgpu_ts_stream_result& aTs, const ohgpu_ts_pes* aPes, const ohgpu_adts_stream_result& aAdts, const ohgpu_adts_frame* aFrames, const TByte* aEs);
private:
    struct Stamp { TUint64 esOffset; TUint64 pts; };                  // a PES packet: where its bytes begin in the elementary stream
    IAdtsFrameSink& iSink;
    std::vector<TByte> iPending, iKept;
    std::deque<Stamp> iStamps;
    TUint64 iEsBase;                                                   // the elementary offset of iKept's first byte
    TUint64 iFrames;
    TUint iPmtPid, iAudioPid, iPesOpenBytes, iStatus;
    TBool iRecognised, iCorrupt;
};

} // namespace Media
} // namespace OpenHome
