// PcmFileDecoder.h -- the codec side of PCM files: the bytes of a WAV, AIFF or AIFC file in, MsgAudioPcm out, the chunks read and the
// audio made big-endian on the device.
//
// Stands in for (file:line relative to the reference tree):
//   CodecWav::Recognise / CodecAiffBase::Recognise   OpenHome/Media/Codec/Wav.cpp, AiffBase.cpp   the form header's twelve bytes
//   CodecWav::StreamInitialise, ::Process            OpenHome/Media/Codec/Wav.cpp                 `fmt `, `data`, the byte-order change
//   CodecAiffBase::StreamInitialise, ::Process       OpenHome/Media/Codec/AiffBase.cpp            `COMM`, `SSND`
//   CodecAiff / CodecAifc                            OpenHome/Media/Codec/Aiff.cpp, Aifc.cpp      the two COMM forms, `sowt`
//   CodecWav::TrySeek / CodecAiffBase::TrySeek                                                    a sample -> a byte position
// Shape of this implementation: host/Mpeg4AlacDecoder.h's.  A decoder is a byte queue.  Flush() takes every lane of a tick: ONE
// ohgpu_iff_process_host over every lane's bytes at hand, from the frame the lane stands at.  A lane's first OK result announces its
// stream; the frames that came home leave through CodecController::OutputAudioPcm in pieces of at most DecodedAudio::kMaxBytes, whole
// frames each.  While a file's chunks have not all arrived its status is TRUNCATED: the lane waits, unless End() said that no more
// bytes will come.  The whole file at hand goes to the device at every tick (the walk wants the chunks where they lie): DESIGN.md 8.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "DecodedAudioAggregator.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

/** The rules of the three Recognise functions over the first bytes of a stream: twelve bytes decide. */
TBool WavRecognise(const Brx& aBytes);
TBool AiffRecognise(const Brx& aBytes);
TBool AifcRecognise(const Brx& aBytes);

class PcmFileBatchDecoder {
public:
    /** aMaxBitDepth: iController->MaxBitDepth(), 24 or 32; aWav8Unsigned: OHGPU_IFF_FLAG_WAV8_UNSIGNED for this lane. */
    explicit PcmFileBatchDecoder(TUint aMaxBitDepth = 24, TBool aWav8Unsigned = false);
    /** File bytes as they come, from the file's first byte on. */
    void Push(const Brx& aFileBytes);
    /** No more bytes will come: a TRUNCATED file is reported at the next tick. */
    void End() { iEnded = true; }
    TUint64 BytesPushed() const { return iFile.size(); }
    TBool Announced() const { return iAnnounced; }          // the stream's first OK result has been seen
    TBool Dropped() const { return iDropped; }              // a status other than OK was reported: the lane is served no more
    TUint64 NextFrame() const { return iNextFrame; }
    const ohgpu_iff_stream_result& Result() const { ASSERT(iAnnounced || iDropped); return iResult; }

    struct Lane {
        PcmFileBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** One tick for all lanes.  A lane whose file is refused (UNSUPPORTED: CodecStreamFeatureUnsupported; any other status but OK:
     *  CodecStreamCorrupt) is dropped; the first such lane's exception is thrown once every lane has been served. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
    /** The lane goes on at frame aSample: its track offset becomes aSample x Jiffies::kPerSecond / rate and a new MsgDecodedStream
     *  says so.  False (nothing changes) before the stream has been announced or beyond the track's length. */
    static TBool TrySeek(Lane& aLane, TUint64 aSample);
private:
    void Announce(CodecController& aController);
private:
    std::vector<TByte> iFile;
    TUint iMaxBitDepth, iFlags;
    TUint64 iNextFrame;
    TBool iEnded, iAnnounced, iDropped;
    ohgpu_iff_stream_result iResult;
};

} // namespace Media
} // namespace OpenHome
