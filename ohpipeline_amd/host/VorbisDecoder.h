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
// Chained streams (internet radio: every track a link with its own serial, headers, channels, rate and granule positions).  Tick() makes
// the links call (ohgpu_ogg_vorbis_links_process_host) and gets a row a link.  At a link boundary, in CodecVorbis::Process's order
// (Vorbis.cpp:398-438): the old link's PCM, trimmed at its last page; a new decoded-stream message if channels or rate changed; the
// link's comment packet to the observer (CodecVorbis::OutputMetaData's place); the new link's PCM.  trackOffset runs on.  The element
// reads the new link's head from its own queue (Info(), Image(), Serial() are the current link's).  A link whose header packets are not
// all there (OHGPU_VORBIS_LINK_HEAD_OPEN), or for which the tick's region had no room, is cut off at its first page: the queue waits
// there until the head is whole, as at the very start of a stream.  Granule positions are per link: g0 = the first granule-bearing
// audio page's granule minus what the packets completed up to it deliver; the link's last page keeps granule - g0 samples; a negative
// g0 (the specification's start trim) drops the excess from the front of the output of the packet that carries that granule, which is
// what Tremor's vorbis_synthesis_blockin does (tests/test_chained_tremor.py).  After a link's last page the lane is Finished() until
// bytes of a further link arrive.
// Not done: seeking.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "DecodedAudioAggregator.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

/** An Ogg page at the first byte whose first packet begins with a Vorbis identification header's type and name. */
TBool VorbisRecognise(const Brx& aBytes);

/** Where a link's comment header packet goes (type 3, "vorbis", vendor, comments): at the stream's start and at every link. */
class IVorbisCommentObserver {
public:
    virtual ~IVorbisCommentObserver() {}
    virtual void NotifyVorbisComment(const Brx& aCommentPacket) = 0;
};

class OggVorbisBatchDecoder {
public:
    static const TUint kMaxPacketsPerTick = 256;      // a tick's packet records (and, times half the long block, its samples a channel)
    static const TUint kMinRegionBytes = 256 * 1024;  // a tick's PCM region is twice the current link's need and this at least
public:
    OggVorbisBatchDecoder();
    void SetCommentObserver(IVorbisCommentObserver* aObserver) { iObserver = aObserver; }
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
    /** The same halves for the links call, which Tick() makes.  CollectLinks: Collect's rows and the bytes of the lane's PCM region.
     *  ApplyLinks: aRecords and aPacketResults are the lane's rows of the Ogg table (from aOgg.packet_first on), aLinks its link rows,
     *  aDst the destination arena (the rows' dst_offset counts from it).  Returns false when the lane has turned corrupt. */
    TBool CollectLinks(TUint64 aSrcBase, TUint64 aMidBase, TUint64 aDstBase, TUint aPacketFirst, TUint64 aImageOffset, ohgpu_ogg_stream_desc& aOgg,
                       ohgpu_vorbis_stream_desc& aVorbis, TUint64& aRegionBytes) const;
    TBool ApplyLinks(const ohgpu_ogg_stream_desc& aOgg, const ohgpu_vorbis_stream_desc& aVorbis, TUint64 aRegionBytes, const ohgpu_ogg_stream_result& aDemuxed,
                     const ohgpu_ogg_packet* aRecords, const ohgpu_vorbis_packet_result* aPacketResults, const ohgpu_vorbis_link* aLinks, size_t aLinkCount,
                     const TByte* aDst, CodecController& aController, TUint64& aTrackOffset);
private:
    void ReadHead();
    int ParseHeadAt(size_t aOffset, uint64_t& aAudioPage);
    void BeginLink(CodecController& aController);
    void WaitForHeadAt(size_t aQueueOffset);
    void Output(const TByte* aPcm, TUint64 aSamples, CodecController& aController, TUint64& aTrackOffset);
private:
    std::vector<TByte> iPending;        // until the head is whole: the stream from its start; then: the bytes from the resume page on
    std::vector<TByte> iImage;
    ohgpu_vorbis_info iInfo;
    TBool iHeadKnown, iAnnounced, iCorrupt, iFinished;
    TUint64 iSamples, iConsumed;
    TUint iSerial, iNextSeq, iResumeSegment;
    // the current link
    IVorbisCommentObserver* iObserver;
    std::vector<TByte> iComment;        // its comment packet, until it has gone to the observer
    TBool iCommentPending, iResent, iG0Known;
    TUint iAnnouncedChannels, iAnnouncedRate;
    TUint64 iLinkDecoded;               // samples a channel its packets have delivered, before any trim
    TInt64 iG0;
};

} // namespace Media
} // namespace OpenHome
