// RaopReceiver.h -- the receiving side of RAOP (AirPlay) audio in front of the codec: the datagrams of the audio and control ports in,
// MsgAudioPcm out, with parse, repair, ordering, decryption and decoding all on the device.
//
// Stands where these stand in the reference (file:line relative to the reference tree):
//   RaopAudioServer::Run, RaopControlServer::Run     OpenHome/Av/Raop/ProtocolRaop.cpp:1414-1466, 1145-1248   datagram -> packet, sync -> latency
//   ProtocolRaop::ProcessPacket, OutputAudio         OpenHome/Av/Raop/ProtocolRaop.cpp:782-880, 705-743       flush window, session, start / resume, delay
//   Repairer<kMaxRepairFrames>                       OpenHome/Av/Raop/ProtocolRaop.h:466-789                  repair, and its timer's resend requests
//   RaopResendRangeRequester, RaopPacketResendRequest OpenHome/Av/Raop/ProtocolRaop.cpp:1290-1301, 383-396    range -> (start, count) -> 8 wire bytes
// Shape of this implementation (host/RaopDecoder.h's): a receiver is a queue of datagrams as they came off the two sockets; nothing of
// them is looked at when they arrive.  Tick() takes every lane, lays the queued datagrams of all of them into one arena and makes ONE
// fused device call (ohgpu_raop_rx_alac_process_host, packed little-endian output); the datagrams that still wait for a missing frame
// are put back in front of the queue by their `order`, state_out becomes the next tick's state, and each packet leaves through
// CodecController::OutputAudioPcm in CodecAlacAppleBase::Decode's pieces.  Sockets, threads, the RSA unwrap, RTSP / SDP and the
// timing port stay the host's.
#pragma once

#include <vector>

#include "AlacDecoder.h"
#include "RaopDecoder.h"

namespace OpenHome {
namespace Media {

class IRaopResendSink {
public:
    virtual void RequestResend(TUint aSeqStart, TUint aCount) = 0;     // RaopControlServer::RequestResend
    virtual ~IRaopResendSink() {}
};

class IRaopReceiverObserver {
public:
    virtual void NotifyNewStream() = 0;                                // ProcessStreamStartOrResume: a new stream id, the container again
    virtual void NotifyDelay(TUint aLatencySamples) = 0;               // ISupply::OutputDelay(Delay(latency))
    virtual void NotifyDiscontinuity(TUint aStopReason) = 0;           // OutputDiscontinuity: OHGPU_RAOP_RX_STOP_BUFFER_FULL or _RESTARTED
    virtual ~IRaopReceiverObserver() {}
};

class RaopReceiver {
public:
    static const TUint kMaxRepairFrames = 50;                          // ProtocolRaop::kMaxRepairFrames
    static const TUint kInitialRepairTimeoutMs = 10;                   // Repairer::kInitialRepairTimeoutMs (the reference draws 0..10 at random)
    static const TUint kSubsequentRepairTimeoutMs = 30;
    static const TUint kDatagramAlign = 16;                            // where a queued datagram starts in the pending arena
    static const TUint kResendRequestBytes = 8;
public:
    explicit RaopReceiver(IRaopResendSink* aResendSink = nullptr, IRaopReceiverObserver* aObserver = nullptr, TUint aMaxFrames = kMaxRepairFrames);
    ~RaopReceiver();
    /** The session's SDP fmtp string, AES key and IV (after the RSA unwrap).  Drops what is queued and starts a new receiver state. */
    void SetSession(const Brx& aFmtp, const Brx& aKey, const Brx& aIv);
    /** One datagram as recvfrom returned it, from the audio or the control socket.  Queued until the next Tick. */
    void PushAudio(const Brx& aDatagram) { Push(aDatagram, OHGPU_RAOP_RX_PORT_AUDIO); }
    void PushControl(const Brx& aDatagram) { Push(aDatagram, OHGPU_RAOP_RX_PORT_CONTROL); }
    /** ProtocolRaop::SendFlush: packets at or below both are dropped while a resume is pending. */
    void SendFlush(TUint aSeq, TUint aTime);
    /** Repairer::DropAudio: what waits is forgotten, the next frame starts the count again. */
    void DropAudio();
    /** RaopPacketResendRequest::Write: the 8 bytes that ask the sender for aCount packets from aSeqStart. */
    static void WriteResendRequest(TUint aSeqStart, TUint aCount, TByte aOut[kResendRequestBytes]);

    TUint PendingDatagrams() const { return (TUint)iSizes.size(); }
    TUint WaitingFrames() const { return iWaiting; }                   // of the queued datagrams, those kept from the last Tick
    TBool Repairing() const { return iRepairing; }
    TUint64 PacketsOutput() const { return iPackets; }
    const ohgpu_raop_rx_state& State() const { return iState; }

    struct Lane {
        RaopReceiver* receiver;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** One fused device call for all lanes at time aNowMs (any monotonic millisecond clock): PCM to each lane's controller, events and
     *  a stop to its observer, resend requests to its sink -- the first when a repair is kInitialRepairTimeoutMs old, then one every
     *  kSubsequentRepairTimeoutMs, each range as (start, (end - start) + 1). */
    static void Tick(TUint64 aNowMs, MsgFactory& aFactory, Lane* aLanes, size_t aCount);

    /** The halves of Tick around the device call, apart so that a test can stand in for the device.  Collect: this receiver's rows of
     *  a tick's tables, its datagrams from aSrcBase on.  Apply: what the receiver batch answered for them. */
    void Collect(TUint64 aSrcBase, ohgpu_raop_rx_stream& aStream, std::vector<ohgpu_raop_rx_datagram>& aDatagrams) const;
    const std::vector<TByte>& PendingArena() const { return iPending; }
    void Apply(TUint64 aNowMs, const ohgpu_raop_rx_stream_result& aResult, const ohgpu_raop_rx_record* aRecords);
private:
    void Push(const Brx& aDatagram, TUint aPort);
    void Clear();
private:
    IRaopResendSink* iResendSink;
    IRaopReceiverObserver* iObserver;
    TUint iMaxFrames;
    ohgpu_raop_rx_state iState;
    ohgpu_alac_config iConfig;
    TByte iKey[16], iIv[16];
    std::vector<TByte> iPending;
    std::vector<TUint> iOffsets, iSizes;
    std::vector<TByte> iPorts;
    TUint iWaiting;
    TBool iConfigured, iAnnounced, iCorrupt, iRepairing;
    TUint64 iNextRequestMs;
    TUint64 iPackets;
};

} // namespace Media
} // namespace OpenHome
