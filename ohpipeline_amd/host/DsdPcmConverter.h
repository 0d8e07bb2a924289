// DsdPcmConverter.h -- DSD in, PCM out: the element that stands between a DSD source and everything built behind PCM.
//
// The reference has no such element: a DSD stream is announced Multiroom::Forbidden (Codec/CodecController.cpp:758),
// Sender::ProcessMsg(MsgAudioDsd*) asserts (Av/Songcast/Sender.cpp:251-254), RampApplicator never sees DSD, and an animator that
// reports aDsd = 0 cannot play it.  This one turns the pipeline's DSD format into 24-bit stereo PCM at dsd_rate / D by the project's
// own integer specification (include/ohgpu.h), so that the stream leaves as MsgDecodedStream + MsgAudioPcm like any codec's output.
// Shape (FlacBatchDecoder's, DsdPacker's): a converter is a queue of chunks per stream; Push only queues.  Flush() takes every lane of
// a tick, lays each lane's WINDOW -- the chunks its new frames read, N - D bits of history included -- into one arena and makes ONE
// device call (ohgpu_dsd_pcm_process_host); each lane's frames then leave through CodecController::OutputAudioPcm in pieces of at
// most DecodedAudio::kMaxBytes.  A lane keeps the history its next frames need and nothing older; a stream start reads the idle
// pattern; a lane flushed tick by tick gives bit for bit what one conversion of its whole stream gives.
#pragma once

#include <vector>

#include "DecodedAudioAggregator.h"
#include "Msg.h"

struct ohgpu_dsd_pcm;

namespace OpenHome {
namespace Media {

/** A decimator designed by ohgpu_dsd_pcm_design and, when the factory has a device, uploaded; shared by the lanes of a Flush. */
class DsdPcmFilter {
public:
    DsdPcmFilter(MsgFactory& aFactory, TUint aDsdRate, TUint aPcmRate, TUint aTapsPerOutput = 16, double aBeta = 14.0,
                 double aPassHz = 20000.0, double aGain = 1.0);
    ~DsdPcmFilter();
    DsdPcmFilter(const DsdPcmFilter&) = delete;
    DsdPcmFilter& operator=(const DsdPcmFilter&) = delete;
    TUint DsdRate() const { return iDsdRate; }
    TUint PcmRate() const { return iPcmRate; }
    TUint Decimation() const { return iDecimation; }
    TUint TapsPerOutput() const { return iTaps; }
    const std::vector<int32_t>& Coefficients() const { return iCoef; }
    const ohgpu_dsd_pcm* Handle() const { return iHandle; }
private:
    MsgFactory& iFactory;
    const TUint iDsdRate, iPcmRate, iTaps;
    TUint iDecimation;
    std::vector<int32_t> iCoef;
    ohgpu_dsd_pcm* iHandle;
};

class DsdPcmConverter {
public:
    static const TUint kBitDepth = 24, kChannels = 2, kFrameBytes = 6;
    static const TUint kPieceFrames = DecodedAudio::kMaxBytes / kFrameBytes;     // 1536: whole frames within 9216 bytes
public:
    DsdPcmConverter(const DsdPcmFilter& aFilter, TUint aSampleBlockWords, TUint aPadBytesPerChunk);
    /** Whole chunks in the pipeline's DSD format -- a MsgAudioDsd's or a DSD playable's bytes -- in stream order. */
    void Push(const Brx& aDsd);
    /** Output frames the next Flush delivers: those whose newest bit has arrived. */
    TUint ConvertibleFrames() const;
    /** The chunks [aLo, aHi) the next Flush sends (ohgpu_dsd_pcm_window of its frames); false when it has no frame to deliver. */
    TBool Window(TUint64& aLo, TUint64& aHi) const;
    TUint64 FramesOut() const { return iFramesOut; }
    TUint64 FirstChunkHeld() const { return iChunk0; }
    TUint64 ChunksHeld() const { return iPending.size() / iChunkBytes; }
    const DsdPcmFilter& Filter() const { return iFilter; }

    /** One stream of a tick: its converter, where its messages go and the stream's position (advanced by what was output). */
    struct Lane {
        DsdPcmConverter* converter;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** Converts what every lane has pending in one device call and hands each lane's frames to its controller. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
    /** The second half of Flush for one lane: announces the stream before its first audio (pcm rate, 24 bit, 2 channels: multiroom
     *  allowed by the rate, CodecController.cpp:729-732), hands aFrames frames of packed big-endian S24 on in pieces of at most
     *  kPieceFrames, counts them as output and drops the chunks no later frame reads. */
    static void Deliver(Lane& aLane, const TByte* aPcm, TUint aFrames);
private:
    const DsdPcmFilter& iFilter;
    const TUint iSampleBlockWords, iPadBytesPerChunk, iChunkBytes;
    std::vector<TByte> iPending;                         // chunks iChunk0 .. of the stream
    TUint64 iChunk0 = 0, iFramesOut = 0;
    TBool iAnnounced = false;
};

} // namespace Media
} // namespace OpenHome
