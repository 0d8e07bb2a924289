// Mpeg4AlacDecoder.h -- the codec side of Apple Lossless in an MPEG-4 file: file bytes in, MsgAudioPcm out, the container's boxes and
// sample tables read on the device in front of host/AlacDecoder.h's packet decoder (5.12).
//
// Stands in for the container element and what CodecAlacApple takes from it (file:line relative to the reference tree):
//   Mpeg4Container::Recognise          OpenHome/Media/Codec/Mpeg4.cpp:4692          "ftyp" at bytes 4..8
//   CodecAlacApple::StreamInitialise   OpenHome/Media/Codec/AlacApple.cpp:92-186    configuration, timescale, duration out of the container
//   CodecAlacApple::TrySeek            OpenHome/Media/Codec/AlacApple.cpp:188-218   a frame -> a packet through the seek table
// Shape of this implementation: host/OggFlacDecoder.h's.  A decoder is a byte queue.  Push() looks at nothing but the top-level box
// headers (8 or 16 bytes each) to learn when `moov` is whole -- with `moov` behind `mdat` that is when the file is -- and how far the
// boxes seen so far reach.  Flush() takes every lane of a tick: ONE ohgpu_mp4_process_host for the lanes whose head became whole this
// tick (the bytes at hand, zeros where the file has not arrived yet, up to the end of the boxes seen: the tables are expanded once),
// then every packet that has arrived whole goes to the lane's AlacBatchDecoder, and ONE AlacBatchDecoder::Flush decodes all lanes.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "AlacDecoder.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

/** Mpeg4Container::Recognise's rule over the first bytes of a stream. */
TBool Mpeg4Recognise(const Brx& aBytes);

class Mpeg4AlacBatchDecoder {
public:
    Mpeg4AlacBatchDecoder();
    /** File bytes as they come, from the file's first byte on.  Throws CodecStreamCorrupt at the eighth byte when they are no MPEG-4 file. */
    void Push(const Brx& aFileBytes);
    TBool HeadWhole() const { return iHeadWhole; }          // `moov` and every top-level header in front of it have arrived
    TBool HeadRead() const { return iHeadRead; }            // ... and the device has read them
    TUint64 BytesPushed() const { return iFile.size(); }
    TUint64 Extent() const { return iExtent; }              // how far the top-level boxes seen so far reach
    TUint TopLevelBoxes() const { return iBoxes; }
    TUint64 NextPacket() const { return iNext; }
    TBool Corrupt() const { return iBad; }
    const ohgpu_mp4_stream_result& Result() const { ASSERT(iHeadRead); return iResult; }
    AlacBatchDecoder& Alac() { return iAlac; }
    /** The packet that holds audio frame aFrame becomes the next one handed on; aFirstFrame is that packet's first frame.  False
     *  (nothing changes) while the head has not been read or when the frame lies behind the track. */
    TBool TrySeek(TUint64 aFrame, TUint64& aFirstFrame);

    struct Lane {
        Mpeg4AlacBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** One tick for all lanes.  A lane whose file is refused (any status but OK: CodecStreamCorrupt; UNSUPPORTED and NOT_ALAC:
     *  CodecStreamFeatureUnsupported) or whose packets do not decode delivers what precedes; the first such lane's exception is thrown
     *  once every lane has been served. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
private:
    void Peek();
private:
    std::vector<TByte> iFile;
    TUint64 iPeekAt, iExtent, iMoovEnd, iNext;
    TUint iBoxes;
    TBool iMoovSeen, iMdatSeen, iStuck, iHeadWhole, iHeadRead, iBad;
    ohgpu_mp4_stream_result iResult;
    std::vector<ohgpu_alac_packet> iPackets;    // offsets from the file's first byte
    std::vector<ohgpu_mp4_sample> iSamples;
    AlacBatchDecoder iAlac;
};

} // namespace Media
} // namespace OpenHome
