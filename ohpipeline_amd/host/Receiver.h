// Receiver.h -- the receiving end of Songcast in the host adapter: OHM datagrams in, MsgDecodedStream / MsgAudioPcm out, the parse,
// the frame sequencer and the unpacking of the audio done on the device (include/ohgpu.h, ohgpu_ohm_rx_*).
//
// Stands where these stand in the reference (file:line relative to the reference tree):
//   OhmHeader::Internalise, OhmMsgAudio::Create      OpenHome/Av/Songcast/Ohm.cpp:22-42, OhmMsg.cpp:101-175      } the device's parse
//   ProtocolOhBase::Process(OhmMsgAudio&), Repair,   OpenHome/Av/Songcast/ProtocolOhBase.cpp:254-405, 515-553    } the device's sequencer
//     RepairReset
//   ProtocolOhBase::OutputAudio                      :461-513   its decisions on the device, its calls here: a stream announced at
//                                                               NEW_STREAM, a delay reported at DELAY, the audio handed on, a halt
//   ProtocolOhBase::RequestResend                    :93-110    the datagram built here from the result's frame numbers
//   CodecPcm (big-endian path)                       OpenHome/Media/Codec/Pcm.cpp:102-107   CodecController::OutputAudioPcm(..., Big, ...)
// Shape of this implementation (host/RaopDecoder.h's): a receiver is a queue of datagrams; PushDatagram touches nothing.  Flush()
// takes every lane of a tick, lays the queued datagrams of all of them into one arena and makes ONE device call
// (ohgpu_ohm_rx_process_host); each lane's output then leaves through its CodecController in output order.  The host never reads a
// header field or an audio byte of a datagram: everything it acts on comes from the result records.
// Frames that still wait at the end of a tick (PENDING) stay queued, in the records' replay order, in front of the next tick's
// arrivals; the state ProtocolOhBase carries between datagrams is kept here between ticks.  After a stop (a halt frame, or a frame in
// the past that is no resend) the receiver does what the reference's receive loop does: it drops what is queued and ignores what
// arrives until Restart().
// Left out, and the caller's: track and metatext messages, join / listen / leave, timestamping, sockets, zones, and the repair
// TIMERS (10 ms random, then 30 ms, restarted by ResendSeen) -- the request a timer would send is offered after every Flush.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "DecodedAudioAggregator.h"
#include "Msg.h"

namespace OpenHome {
namespace Av {

class IOhmReceiverObserver {
public:
    virtual ~IOhmReceiverObserver() {}
    virtual void NotifyDelay(TUint aJiffies) = 0;          // ISupply::OutputDelay (ProtocolOhBase.cpp:492-493)
    virtual void NotifyHalt() = 0;                         // OutputWait + OutputHalt (:505-508)
    virtual void NotifyStopped(TUint aReason) = 0;         // OHGPU_OHM_RX_STOP_*, or kStopUnsupported
};

class IOhmResendSink {                                     // where RequestResend calls iSocket.Send (:105)
public:
    virtual ~IOhmResendSink() {}
    virtual void RequestResend(const Brx& aDatagram) = 0;
};

class OhmReceiver {
public:
    static const TUint kDatagramAlign = 16;                // where a queued datagram starts in the pending arena
    static const TUint kMaxDatagramBytes = 65535;          // what OhmHeader's 16-bit total can say
    static const TUint kStopUnsupported = 3;               // a stream was announced in a format the pipeline cannot carry
public:
    explicit OhmReceiver(IOhmReceiverObserver* aObserver = nullptr, IOhmResendSink* aResendSink = nullptr);
    /** One datagram as it came off the socket.  Queued until the next Flush; nothing of it is looked at.  Ignored (and counted) while
     *  the receiver is stopped; asserts on more than kMaxDatagramBytes. */
    void PushDatagram(const Brx& aDatagram);
    /** After a stop: arrivals are taken again; the next audio frame starts a stream. */
    void Restart();
    TBool Stopped() const { return iStopped; }
    TUint StopReason() const { return iStopReason; }
    TUint PendingDatagrams() const { return (TUint)iSizes.size(); }
    TUint PendingOffset(TUint aIndex) const { ASSERT(aIndex < iOffsets.size()); return iOffsets[aIndex]; }
    TUint PendingBytes(TUint aIndex) const { ASSERT(aIndex < iSizes.size()); return iSizes[aIndex]; }
    TUint WaitingFrames() const { return iWaiting; }       // of the queued datagrams, those kept from the last Flush
    TUint IgnoredWhileStopped() const { return iIgnored; }
    TUint64 FramesOutput() const { return iFramesOutput; }
    TUint64 BytesOutput() const { return iBytesOutput; }
    const ohgpu_ohm_rx_state& State() const { return iState; }

    /** One stream of a tick: its receiver, where its messages go and the stream's position (set at a new stream, advanced by what
     *  was output). */
    struct Lane {
        OhmReceiver* receiver;
        Media::CodecController* controller;
        TUint64 trackOffset;
    };
    /** Parses, sequences and gathers what every lane has queued in one device call and hands each lane's output to its controller. */
    static void Flush(Media::MsgFactory& aFactory, Lane* aLanes, size_t aCount);

    /** The two halves of Flush around the device call, apart so that a test can stand in for the device.  Collect: the tables of a
     *  tick (lanes with nothing queued, or stopped, are left out) and the source arena's layout; FillSource: the datagrams into it. */
    struct Tick {
        std::vector<ohgpu_ohm_rx_stream> streams;
        std::vector<ohgpu_ohm_rx_datagram> datagrams;
        std::vector<size_t> laneOf;                        // per stream of the tables: its lane
        std::vector<TUint64> srcBase;                      // ... and where its pending arena goes in the source arena
        TUint64 srcBytes = 0, dstBytes = 0;
    };
    static void Collect(Lane* aLanes, size_t aCount, Tick& aTick);
    static void FillSource(const Lane* aLanes, const Tick& aTick, TByte* aSrc);
    /** Deliver: every lane's records in output order -- OutputDecodedStream at NEW_STREAM, the observer's delay at DELAY, the run's
     *  bytes to OutputAudioPcm, the observer's halt and stop --, the resend request, and the queue for the next tick. */
    static void Deliver(Lane* aLanes, const Tick& aTick, const ohgpu_ohm_rx_stream_result* aResults, const ohgpu_ohm_rx_record* aRecords, const TByte* aDst);
private:
    void Drop();
    void Requeue(const std::vector<TUint>& aKeep);
private:
    IOhmReceiverObserver* iObserver;
    IOhmResendSink* iResendSink;
    ohgpu_ohm_rx_state iState;
    std::vector<TByte> iPending;        // the queued datagrams, each at a multiple of kDatagramAlign
    std::vector<TUint> iOffsets, iSizes;
    TUint iWaiting, iIgnored, iStopReason;
    TBool iStopped;
    TUint64 iFramesOutput, iBytesOutput;
};

} // namespace Av
} // namespace OpenHome
