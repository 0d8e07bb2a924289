// AlacDecoder.h -- the codec side of Apple Lossless: the container's packets in, MsgAudioPcm out, the packets decoded on the device
// (DESIGN.md 5.12).
//
// Stands in for CodecAlacApple and the Apple decoder under it (file:line relative to the reference tree):
//   CodecAlacApple::StreamInitialise   OpenHome/Media/Codec/AlacApple.cpp:92-186    the 24-byte configuration, the container's
//                                                                                   timescale and duration -> OutputDecodedStream
//   CodecAlacAppleBase::Decode         OpenHome/Media/Codec/AlacAppleBase.cpp:66-115  a packet -> little-endian pieces -> OutputAudioPcm
// Shape of this implementation (host/FlacDecoder.h's): a decoder is a packet queue; nothing is decoded when packets arrive.  The
// MPEG-4 container is not in this element (on the device it is ohgpu_mp4_*, DESIGN.md 5.16, whose results and packet rows are what
// goes in here): SetConfig takes what StreamInitialise reads out of it, PushPacket takes one sample of the 'mdat' box as the sample
// table delimits it.  Flush() takes every lane of a tick, lays the queued packets of all of them into one arena and
// makes ONE device call (ohgpu_alac_process_host, packed little-endian output -- the reference decoder's own buffer); each packet
// leaves through CodecController::OutputAudioPcm in Decode's pieces.  Packets are independent, so a seek is a change of the index the
// next packet is counted from (SeekToPacket); the sample table that turns a time into that index is the container's.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "DecodedAudioAggregator.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

class AlacBatchDecoder {
public:
    static const TUint kMaxPieceBytes = DecodedAudio::kMaxBytes;    // AlacAppleBase.cpp:96
    static const TUint kChannelsMost = 2;                             // (kMaxChannels and kMaxSamplesPerFrame of AlacAppleBase.h: the decoded buffer's capacity)
    static const TUint kFrameLengthMost = 4096;
public:
    AlacBatchDecoder();
    /** What StreamInitialise takes from the container: the configuration (with or without the atoms in front of it), the track's
     *  timescale -- the sample rate that is announced -- and its duration in units of it.  Throws CodecStreamCorrupt for a
     *  configuration that does not parse, more than two channels or a frame length above 4096 (AlacApple.cpp:147-157). */
    void SetConfig(const Brx& aCookie, TUint aTimescale, TUint64 aDuration);
    TBool Configured() const { return iConfigured; }
    const ohgpu_alac_config& Config() const { ASSERT(iConfigured); return iConfig; }
    /** One packet; queued until the next Flush. */
    void PushPacket(const Brx& aPacket);
    TUint PendingPackets() const { return (TUint)iSizes.size(); }
    TUint PendingBytes() const { return (TUint)iPending.size(); }
    TUint64 SamplesDecoded() const { return iSamples; }
    TUint64 NextPacket() const { return iNextPacket; }
    TBool Corrupt() const { return iCorrupt; }
    /** The next packet pushed is the stream's packet aIndex: drops what is queued.  Packets do not depend on each other, so nothing
     *  else changes (CodecAlacApple::TrySeek, AlacApple.cpp:188-218, does the same after asking the sample table for the index). */
    void SeekToPacket(TUint64 aIndex);
    /** How Decode cuts a packet's aBytes of audio: pieces of kMaxPieceBytes and the rest (AlacAppleBase.cpp:94-111). */
    static TUint Pieces(TUint aBytes) { return (aBytes + kMaxPieceBytes - 1) / kMaxPieceBytes; }

    /** One stream of a tick: its decoder, where its messages go and the stream's position (advanced by what was output). */
    struct Lane {
        AlacBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** Decodes what every lane has queued in one device call and hands each lane's packets to its controller.  A lane with a packet
     *  that does not decode delivers the packets before it; once every lane has been served the first such lane's
     *  CodecStreamCorrupt (a 20-bit stream: CodecStreamFeatureUnsupported) is thrown. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
private:
    ohgpu_alac_config iConfig;
    TUint iRate;
    TUint64 iLengthJiffies;
    std::vector<TByte> iPending;        // the queued packets, back to back
    std::vector<TUint> iSizes;          // ... and their sizes
    TBool iConfigured, iAnnounced, iCorrupt;
    TUint64 iNextPacket, iSamples;
};

// The Apple Lossless output path, which host/RaopDecoder.h shares: RAOP's streams are Apple Lossless streams behind a cipher.
/** What StreamInitialise asks of a configuration, in its order: aParsed, a frame length of 1..4096 and one or two channels (else
 *  CodecStreamCorrupt), a bit depth of 16, 20, 24 or 32 (else CodecStreamFeatureUnsupported).  Sets aCorrupt before it throws. */
void AlacCheckConfig(TBool aParsed, const ohgpu_alac_config& aConfig, TBool& aCorrupt);
/** A stream's share of a tick's output: the stream announced once (aRate and aLengthJiffies are the caller's), then every packet in
 *  front of the first that did not decode, in CodecAlacAppleBase::Decode's pieces.  False when there was such a packet. */
TBool AlacDeliver(CodecController& aController, TUint64& aTrackOffset, TBool& aAnnounced, TUint aRate, TUint64 aLengthJiffies,
                  const ohgpu_alac_stream_desc& aDesc, const ohgpu_alac_stream_result& aResult, const ohgpu_alac_packet_result* aEach, const TByte* aDst);
/** Once every lane has been served: the first bad lane's exception (aFirstBad null: none was bad). */
void AlacThrowFirstBad(const ohgpu_alac_stream_result* aFirstBad);

} // namespace Media
} // namespace OpenHome
