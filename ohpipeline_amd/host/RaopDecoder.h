// RaopDecoder.h -- the codec side of RAOP (AirPlay) audio: RTP datagrams in, MsgAudioPcm out, the payloads decrypted AND decoded on the
// device.
//
// Stands where these stand in the reference (file:line relative to the reference tree):
//   RtpPacketRaop::Set, RaopPacketAudio::Set   OpenHome/Av/Raop/ProtocolRaop.cpp:57-92, 166-177, 217-247   the 4 + 8 header bytes
//   RaopAudioDecryptor::Decrypt                OpenHome/Av/Raop/ProtocolRaop.cpp:1477-1502                 AES-128-CBC per packet
//   CodecRaopApple::StreamInitialise, Process  OpenHome/Av/Raop/CodecRaopApple.cpp:61-119, 133-171         fmtp -> configuration,
//                                                                                                          packet -> OutputAudioPcm
// Shape of this implementation (host/AlacDecoder.h's): a decoder is a queue of encrypted payloads; nothing is decrypted or decoded
// when datagrams arrive.  Flush() takes every lane of a tick, lays the queued payloads of all of them into one arena and makes ONE
// device call (ohgpu_raop_process_host, packed little-endian output); each packet leaves through CodecController::OutputAudioPcm in
// CodecAlacAppleBase::Decode's pieces.  The host never touches a sample, nor a plaintext byte.
// Packets are expected in playing order: the resend / repair machinery in front (ProtocolRaop's Repairer) and the control port are
// host/RaopReceiver.h's, which takes the datagrams as they arrive; the RSA unwrap of the session key, RTSP / SDP and the timing port
// stay the host's.  This codec cannot seek (CodecRaopApple::TrySeek returns
// false): there is no counterpart.
#pragma once

#include <vector>

#include "AlacDecoder.h"

namespace OpenHome {
OH_EXCEPTION(InvalidRaopPacket);
namespace Media {

class RaopBatchDecoder {
public:
    static const TUint kMaxPieceBytes = DecodedAudio::kMaxBytes;    // AlacAppleBase.cpp:96
    static const TUint kChannelsMost = 2;                             // CodecRaopApple.cpp:85-94 (kMaxChannels, kMaxSamplesPerFrame of AlacAppleBase.h)
    static const TUint kFrameLengthMost = 4096;
    static_assert(kMaxPieceBytes == AlacBatchDecoder::kMaxPieceBytes && kChannelsMost == AlacBatchDecoder::kChannelsMost
                  && kFrameLengthMost == AlacBatchDecoder::kFrameLengthMost, "the Apple Lossless output path (AlacDecoder.h) applies AlacBatchDecoder's");
    static const TUint kMaxDatagramBytes = 1472;                      // RtpPacketRaop::kMaxPacketBytes
    static const TUint kRtpHeaderBytes = 4;                           // RtpHeaderRaop::kBytes
    static const TUint kAudioHeaderBytes = 8;                         // RaopPacketAudio::kAudioSpecificHeaderBytes: timestamp, ssrc
    static const TUint kKeyBytes = 16;
    static const TUint kPayloadAlign = 16;                            // where a queued payload starts in the pending arena
public:
    RaopBatchDecoder();
    ~RaopBatchDecoder();
    /** What the session's SDP and the RSA unwrap give: the fmtp string (CodecRaopApple::ParseFmtp), the AES key and IV
     *  (RaopAudioDecryptor::Init).  Throws CodecStreamCorrupt for an fmtp that does not parse, a frame length above 4096 or more than
     *  two channels; asserts on a key or IV that is not 16 bytes.  Drops what is queued. */
    void SetSession(const Brx& aFmtp, const Brx& aKey, const Brx& aIv);
    TBool Configured() const { return iConfigured; }
    const ohgpu_alac_config& Config() const { ASSERT(iConfigured); return iConfig; }
    /** One audio datagram as it came off the socket; its payload is queued until the next Flush.  Throws InvalidRaopPacket for fewer
     *  than 4 header bytes, fewer than 8 bytes behind them, or more than kMaxDatagramBytes; RTP version and payload type are not
     *  looked at (some senders set both to 0 on resent packets: ProtocolRaop.cpp:66-73, 231-238). */
    void PushDatagram(const Brx& aRtp);
    TUint LastSeq() const { return iLastSeq; }
    TUint LastTimestamp() const { return iLastTimestamp; }
    TUint LastSsrc() const { return iLastSsrc; }
    TUint PendingPackets() const { return (TUint)iSizes.size(); }
    TUint PendingBytes() const { return iPendingBytes; }               // payload bytes, without the padding between them
    TUint PendingOffset(TUint aIndex) const { ASSERT(aIndex < iOffsets.size()); return iOffsets[aIndex]; }
    TUint64 SamplesDecoded() const { return iSamples; }
    TUint64 PacketsDecoded() const { return iPackets; }
    TBool Corrupt() const { return iCorrupt; }
    static TUint Pieces(TUint aBytes) { return (aBytes + kMaxPieceBytes - 1) / kMaxPieceBytes; }

    /** One stream of a tick: its decoder, where its messages go and the stream's position (advanced by what was output). */
    struct Lane {
        RaopBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** Decrypts and decodes what every lane has queued in one device call and hands each lane's packets to its controller.  A lane
     *  with a packet that does not decode delivers the packets before it; once every lane has been served the first such lane's
     *  CodecStreamCorrupt (a 20-bit stream: CodecStreamFeatureUnsupported) is thrown. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
private:
    void Drop();
private:
    ohgpu_alac_config iConfig;
    TByte iKey[kKeyBytes], iIv[kKeyBytes];
    std::vector<TByte> iPending;        // the queued payloads, each at a multiple of kPayloadAlign
    std::vector<TUint> iOffsets, iSizes;
    TUint iPendingBytes;
    TUint iLastSeq, iLastTimestamp, iLastSsrc;
    TBool iConfigured, iAnnounced, iCorrupt;
    TUint64 iSamples, iPackets;
};

} // namespace Media
} // namespace OpenHome
