// VorbisDecoder.h -- the codec side of Ogg Vorbis: file or radio bytes in, MsgAudioPcm out, pages and packets both handled on the device
// (DESIGN.md 5.15 in front of 5.23).
//
// Stands in for what CodecVorbis does through Tremor (file:line relative to the reference tree):
//   CodecVorbis::Recognise         OpenHome/Media/Codec/Vorbis.cpp    Tremor's test open: an Ogg page whose first packet is a Vorbis identification header
//   CodecVorbis::StreamInitialise  OpenHome/Media/Codec/Vorbis.cpp    channels, rate, 16 bits -> OutputDecodedStream
//   CodecVorbis::Process           OpenHome/Media/Codec/Vorbis.cpp    big-endian 16-bit samples -> OutputAudioPcm in pieces within DecodedAudio::kMaxBytes
// Shape of this implementation: host/OggFlacDecoder.h's.  A decoder is a byte queue.  The first bytes are the head -- the pages that hold
// the three header packets -- read on the host once all of it is there (ohgpu_vorbis_head), which gives the setup image and says on which
// page, at which segment and with which page number the audio begins.  Tick() takes every lane and makes ONE device call
// (ohgpu_ogg_vorbis_process_host).  The first packet of a call only primes the overlap, so the queue keeps the bytes from the page on
// which the LAST packet a tick consumed began, with that page's number and the packet's segment: the next tick sends that packet again in
// front of the new ones.  At the page with the "last page" flag the output is trimmed to that page's granule position.
// Not done: seeking, chained streams, comments, a first granule other than the first block's.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "DecodedAudioAggregator.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

/** An Ogg page at the first byte whose first packet begins with a Vorbis identification header's type and name. */
TBool VorbisRecognise(const Brx& aBytes);

class OggVorbisBatchDecoder {
public:
    static const TUint kMaxPacketsPerTick = 256;      // a tick's packet records (and, times half the long block, its samples a channel)
public:
    OggVorbisBatchDecoder();
    /** Bytes as they come, from "OggS" on.  Throws CodecStreamCorrupt when they do not start an Ogg Vorbis stream,
     *  CodecStreamFeatureUnsupported for a setup the decoder does not take (floor 0, more than 8 channels). */
    void Push(const Brx& aBytes);
    TBool HeadKnown() const { return iHeadKnown; }
    const ohgpu_vorbis_info& Info() const { ASSERT(iHeadKnown); return iInfo; }
    /** Bytes queued from the resume page on. */
    TUint PendingBytes() const { return iHeadKnown ? (TUint)iPending.size() : 0; }
    /** Where the queue's first byte lies in the stream. */
    TUint64 ConsumedBytes() const { return iConsumed; }
    TUint64 SamplesOutput() const { return iSamples; }
    TBool Corrupt() const { return iCorrupt; }
    TBool Finished() const { return iFinished; }      // the page with the "last page" flag has been played
    TUint Serial() const { return iSerial; }
    TUint NextPageNumber() const { return iNextSeq; }
    TUint ResumeSegment() const { return iResumeSegment; }

    struct Lane {
        OggVorbisBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** One fused device call for all lanes: PCM to each lane's controller.  A lane whose pages stop (lost sync, a hole) delivers what
     *  precedes the break; once every lane has been served the first such lane's CodecStreamCorrupt is thrown. */
    static void Tick(MsgFactory& aFactory, Lane* aLanes, size_t aCount);

    /** The halves of Tick around the device call, apart so that a test can stand in for the device.  Collect: this decoder's rows of
     *  a tick's tables (false: nothing to do), its bytes at aSrcBase of the source arena, its packets' bytes at aMidBase of the middle
     *  arena, its samples at aDstBase, its records from aPacketFirst on, its image at aImageOffset of the tick's images.  Apply: what
     *  the fused call answered for them; aPcm the samples it wrote at aDstBase. */
    TBool Collect(TUint64 aSrcBase, TUint64 aMidBase, TUint64 aDstBase, TUint aPacketFirst, TUint64 aImageOffset, ohgpu_ogg_stream_desc& aOgg, ohgpu_vorbis_stream_desc& aVorbis) const;
    const std::vector<TByte>& PendingArena() const { return iPending; }
    const std::vector<TByte>& Image() const { return iImage; }
    /** Returns false when the lane has turned corrupt. */
    TBool Apply(const ohgpu_ogg_stream_desc& aOgg, const ohgpu_ogg_stream_result& aDemuxed, const ohgpu_ogg_packet* aRecords, const ohgpu_vorbis_stream_result& aDecoded,
                const TByte* aPcm, CodecController& aController, TUint64& aTrackOffset);
private:
    void ReadHead();
private:
    std::vector<TByte> iPending;        // until the head is whole: the stream from its start; then: the bytes from the resume page on
    std::vector<TByte> iImage;
    ohgpu_vorbis_info iInfo;
    TBool iHeadKnown, iAnnounced, iCorrupt, iFinished;
    TUint64 iSamples, iConsumed;
    TUint iSerial, iNextSeq, iResumeSegment;
};

} // namespace Media
} // namespace OpenHome
