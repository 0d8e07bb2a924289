// Mpeg4FragmentDecoder.h -- the codec side of fragmented MPEG-4 (DASH / CMAF segments) with a fLaC or an alac track: stream bytes in,
// MsgAudioPcm out, the fragments read on the device in front of the FLAC phases (5.10) or host/AlacDecoder.h's packet
// decoder (5.12).
//
// Stands where the reference's container hands a fragmented stream to its codecs (file:line relative to the reference tree):
//   Mpeg4Container::Recognise          OpenHome/Media/Codec/Mpeg4.cpp:4692          "ftyp" at bytes 4..8
//   the moof switcher                  OpenHome/Media/Codec/Mpeg4.cpp:4563-4568     a fragment after the other, to CodecFlac or CodecAlacApple
//   Mpeg4Container::TrySeek            OpenHome/Media/Codec/Mpeg4.cpp:4778-4794     (the reference does not seek in fragmented FLAC; this does)
// Shape of this implementation: host/Mpeg4AlacDecoder.h's.  A decoder is a byte queue that keeps the stream so far.  Push() looks at
// nothing but the top-level box headers, to learn how far the boxes that have arrived WHOLE reach, and reads the head on the host
// (ohgpu_mp4f_head) as soon as `moov` is whole: that routes the lane by its codec.  Flush() takes every lane of a tick: ONE
// ohgpu_mp4f_flac_process_host for the fLaC lanes that have new whole boxes (the stream up to them; the gather starts at the first row
// that was not delivered yet; the frames leave as host/OggFlacDecoder.h's do), ONE ohgpu_mp4f_process_host for the alac lanes, whose new
// packets go to the lane's AlacBatchDecoder, and ONE AlacBatchDecoder::Flush for all of those.  TrySeek() is ohgpu_mp4_seek on the
// sample rows of the fragments read so far: the row becomes the gather's first row (fLaC) or the next packet (alac).
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "AlacDecoder.h"
#include "FlacDecoder.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

enum class Mpeg4FragmentKind { None, NeedMore, Flac, Alac, Plain, Other };
/** What the first bytes of a stream are: None (no "ftyp" at bytes 4..8), NeedMore (`moov` has not arrived whole), Flac / Alac (a
 *  fragmented stream with such a track: this element's), Plain (a file with sample tables: host/Mpeg4AlacDecoder.h's), Other (an MPEG-4
 *  stream this element refuses). */
Mpeg4FragmentKind Mpeg4FragmentRecognise(const Brx& aBytes);

class Mpeg4FragmentBatchDecoder {
public:
    Mpeg4FragmentBatchDecoder();
    /** Stream bytes as they come, from the first byte on.  Throws CodecStreamCorrupt at the eighth byte when they are no MPEG-4 stream. */
    void Push(const Brx& aBytes);
    TBool HeadRead() const { return iHeadRead; }            // `moov` has arrived whole and was read (on the host)
    Mpeg4FragmentKind Kind() const { return iKind; }        // NeedMore until then
    const ohgpu_mp4f_stream_result& Head() const { ASSERT(iHeadRead); return iHead; }
    TUint64 BytesPushed() const { return iFile.size(); }
    TUint64 WholeExtent() const { return iWhole; }          // how far the top-level boxes that have arrived whole reach
    TUint64 NextRow() const { return iNextRow; }            // the first sample that was not delivered yet
    TUint64 RowsKnown() const { return iSamples.size(); }   // the samples of the fragments read so far
    TBool Corrupt() const { return iBad; }
    AlacBatchDecoder& Alac() { return iAlac; }
    /** The sample that holds audio frame aFrame becomes the next one delivered; aFirstFrame is that sample's first frame.  False
     *  (nothing changes) before a Flush has read a fragment or when the frame lies behind the fragments read so far. */
    TBool TrySeek(TUint64 aFrame, TUint64& aFirstFrame);

    struct Lane {
        Mpeg4FragmentBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** One tick for all lanes.  A lane whose stream is refused (UNSUPPORTED, NOT_CODEC, NOT_FRAGMENTED: CodecStreamFeatureUnsupported;
     *  any other status but OK: CodecStreamCorrupt) or whose samples do not decode delivers what precedes; the first such lane's
     *  exception is thrown once every lane has been served. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
private:
    void Peek();
    int Judge(const ohgpu_mp4f_stream_result& aResult, TUint aCapacity);
    void Describe(ohgpu_mp4f_stream_desc& aDesc, TUint64 aSrcOffset, TUint64 aRow, TUint64 aRun) const;
private:
    std::vector<TByte> iFile;
    TUint64 iPeekAt, iWhole, iMoovEnd, iServed, iNextRow, iNextSample;
    TBool iStuck, iHeadRead, iBad, iAnnounced, iConfigured;
    Mpeg4FragmentKind iKind;
    ohgpu_mp4f_stream_result iHead;
    std::vector<ohgpu_mp4_sample> iSamples;
    AlacBatchDecoder iAlac;
};

} // namespace Media
} // namespace OpenHome
