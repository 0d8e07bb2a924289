// Receiver.cpp -- see Receiver.h.
#include "Receiver.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Av {

using namespace Media;

OhmReceiver::OhmReceiver(IOhmReceiverObserver* aObserver, IOhmResendSink* aResendSink)
    : iObserver(aObserver), iResendSink(aResendSink), iWaiting(0), iIgnored(0), iStopReason(OHGPU_OHM_RX_STOP_NONE), iStopped(false), iFramesOutput(0), iBytesOutput(0)
{
    // ProtocolOhBase's members as its constructor and Stream() leave them (ProtocolOhBase.cpp:203-215)
    memset(&iState, 0, sizeof(iState));
    iState.stream_msg_due = 1;
    iState.last_sample_start = 0xffffffffu;                // UINT_MAX
}

void OhmReceiver::Drop()
{
    iPending.clear();
    iOffsets.clear();
    iSizes.clear();
    iWaiting = 0;
}

void OhmReceiver::PushDatagram(const Brx& aDatagram)
{
    ASSERT(aDatagram.Bytes() <= kMaxDatagramBytes);
    if (iStopped) {
        iIgnored++;
        return;
    }
    const size_t at = (iPending.size() + kDatagramAlign - 1) / kDatagramAlign * kDatagramAlign;
    iPending.resize(at, 0);
    iPending.insert(iPending.end(), aDatagram.Ptr(), aDatagram.Ptr() + aDatagram.Bytes());
    iOffsets.push_back((TUint)at);
    iSizes.push_back(aDatagram.Bytes());
}

void OhmReceiver::Restart()
{
    iStopped = false;
    iStopReason = OHGPU_OHM_RX_STOP_NONE;
}

// The queue becomes the datagrams aKeep (indices into the present queue), in that order.
void OhmReceiver::Requeue(const std::vector<TUint>& aKeep)
{
    std::vector<TByte> pending;
    std::vector<TUint> offsets, sizes;
    for (TUint k : aKeep) {
        const size_t at = (pending.size() + kDatagramAlign - 1) / kDatagramAlign * kDatagramAlign;
        pending.resize(at, 0);
        pending.insert(pending.end(), iPending.begin() + iOffsets[k], iPending.begin() + iOffsets[k] + iSizes[k]);
        offsets.push_back((TUint)at);
        sizes.push_back(iSizes[k]);
    }
    iPending.swap(pending);
    iOffsets.swap(offsets);
    iSizes.swap(sizes);
    iWaiting = (TUint)aKeep.size();
}

void OhmReceiver::Collect(Lane* aLanes, size_t aCount, Tick& aTick)
{
    aTick = Tick();
    for (size_t k = 0; k < aCount; k++) {
        const OhmReceiver& r = *aLanes[k].receiver;
        if (r.iStopped || r.iSizes.empty()) {
            continue;
        }
        ohgpu_ohm_rx_stream s;
        memset(&s, 0, sizeof(s));
        s.first_datagram = (uint32_t)aTick.datagrams.size();
        s.n_datagrams = (uint32_t)r.iSizes.size();
        s.dst_offset = aTick.dstBytes;
        s.state_in = r.iState;
        for (size_t i = 0; i < r.iSizes.size(); i++) {
            const ohgpu_ohm_rx_datagram g = {aTick.srcBytes + r.iOffsets[i], r.iSizes[i], 0};    // (a multiple of 16 each: the ABI asks for 4)
            aTick.datagrams.push_back(g);
            s.dst_capacity += r.iSizes[i] > 58u ? r.iSizes[i] - 58u : 0u;                       // what the table alone says the stream may carry
        }
        aTick.srcBase.push_back(aTick.srcBytes);
        aTick.srcBytes += MsgFactory::ArenaShare(r.iPending.size());
        aTick.dstBytes += MsgFactory::ArenaShare(s.dst_capacity);
        aTick.streams.push_back(s);
        aTick.laneOf.push_back(k);
    }
}

void OhmReceiver::FillSource(const Lane* aLanes, const Tick& aTick, TByte* aSrc)
{
    for (size_t i = 0; i < aTick.streams.size(); i++) {
        const OhmReceiver& r = *aLanes[aTick.laneOf[i]].receiver;
        memcpy(aSrc + aTick.srcBase[i], r.iPending.data(), r.iPending.size());
    }
}

static TBool Carried(const ohgpu_ohm_rx_record& aRec)
{
    // what CodecController and MsgAudioPcm can carry: whole bytes a subsample, the pipeline's channel counts, a rate it knows
    const TUint depth = aRec.bit_depth, channels = aRec.channels;
    if ((depth != 8 && depth != 16 && depth != 24 && depth != 32) || channels == 0 || channels > OHGPU_MAX_CHANNELS) {
        return false;
    }
    return Jiffies::IsValidSampleRate(aRec.sample_rate);
}

void OhmReceiver::Deliver(Lane* aLanes, const Tick& aTick, const ohgpu_ohm_rx_stream_result* aResults, const ohgpu_ohm_rx_record* aRecords, const TByte* aDst)
{
    for (size_t i = 0; i < aTick.streams.size(); i++) {
        Lane& lane = aLanes[aTick.laneOf[i]];
        OhmReceiver& r = *lane.receiver;
        const ohgpu_ohm_rx_stream& s = aTick.streams[i];
        const ohgpu_ohm_rx_stream_result& res = aResults[i];
        const ohgpu_ohm_rx_record* recs = aRecords + s.first_datagram;
        // the records by their place in the output order / in the replay
        std::vector<TUint> out(res.n_output), keep(res.n_pending);
        for (TUint k = 0; k < s.n_datagrams; k++) {
            if (recs[k].disposition == OHGPU_OHM_RX_OUTPUT) {
                ASSERT(recs[k].order < res.n_output);
                out[recs[k].order] = k;
            } else if (recs[k].disposition == OHGPU_OHM_RX_PENDING) {
                ASSERT(recs[k].order < res.n_pending);
                keep[recs[k].order] = k;
            }
        }
        TUint stop = res.stop_reason;
        const ohgpu_ohm_rx_record* format = nullptr;       // the record the run's format comes from
        uint64_t runStart = 0, runBytes = 0;
        auto flushRun = [&]() {
            if (format != nullptr && runBytes != 0) {
                ASSERT(runBytes <= 0xffffffffull);
                lane.trackOffset += lane.controller->OutputAudioPcm(Brn(aDst + runStart, (TUint)runBytes), format->channels, format->sample_rate, format->bit_depth,
                                                                    AudioDataEndian::Big, lane.trackOffset);
                r.iBytesOutput += runBytes;
            }
            runBytes = 0;
        };
        TBool announced = r.iState.stream_msg_due == 0;     // a stream announced in an earlier tick goes on in its format
        ohgpu_ohm_rx_record carried;
        if (announced) {
            memset(&carried, 0, sizeof(carried));
            carried.bit_depth = r.iState.bit_depth; carried.channels = r.iState.channels; carried.sample_rate = r.iState.sample_rate;
            format = &carried;
        }
        for (TUint n = 0; n < res.n_output && stop != kStopUnsupported; n++) {
            const ohgpu_ohm_rx_record& rec = recs[out[n]];
            if (rec.events != 0) {
                flushRun();
            }
            if (rec.events & OHGPU_OHM_RX_EVENT_NEW_STREAM) {
                const TUint frameBytes = (TUint)rec.channels * rec.bit_depth / 8;
                if (!Carried(rec) || rec.audio_bytes % frameBytes != 0) {
                    stop = kStopUnsupported;
                    break;
                }
                // ProtocolOhBase.cpp:477-488 and CodecPcm's StreamInitialise: the wire's format, the track's length and where it starts
                const TUint64 perSample = Jiffies::PerSample(rec.sample_rate);
                lane.controller->OutputDecodedStream(rec.bit_rate, rec.bit_depth, rec.sample_rate, rec.channels, Brn(rec.codec, rec.codec_bytes),
                                                     rec.samples_total * perSample, rec.sample_start, (rec.flags & OHGPU_OHM_FLAG_LOSSLESS) != 0);
                lane.trackOffset = rec.sample_start * perSample;
                format = &rec;
            }
            if ((rec.events & OHGPU_OHM_RX_EVENT_DELAY) && r.iObserver != nullptr && Jiffies::IsValidSampleRate(rec.sample_rate)) {
                r.iObserver->NotifyDelay((TUint)Jiffies::FromSongcastTime(rec.media_latency, rec.sample_rate));
            }
            const TUint frameBytes = format == nullptr ? 0u : (TUint)format->channels * format->bit_depth / 8;
            if (frameBytes == 0 || rec.audio_bytes % frameBytes != 0) {
                stop = kStopUnsupported;                    // (audio that is no whole number of sample frames)
                break;
            }
            if (runBytes == 0) {
                runStart = rec.dst_offset;
            }
            ASSERT(rec.dst_offset == runStart + runBytes);  // the gather lays a stream's output back to back
            runBytes += rec.audio_bytes;
            r.iFramesOutput++;
            if (rec.events & OHGPU_OHM_RX_EVENT_HALT) {
                flushRun();
                if (r.iObserver != nullptr) r.iObserver->NotifyHalt();
            }
        }
        flushRun();
        r.iState = res.state_out;
        if (stop != OHGPU_OHM_RX_STOP_NONE) {
            // the reference leaves its receive loop here: what is queued goes, and nothing is taken until the caller restarts
            r.Drop();
            r.iStopped = true;
            r.iStopReason = stop;
            r.iState.running = 0;
            r.iState.stream_msg_due = 1;
            if (r.iObserver != nullptr) r.iObserver->NotifyStopped(stop);
            continue;
        }
        r.Requeue(keep);
        if (res.n_resend != 0 && r.iResendSink != nullptr) {
            // RequestResend (:93-110): OhmHeader of type resend, OhmHeaderResend's count, the frame numbers
            TByte gram[8 + 4 + 4 * OHGPU_OHM_RX_MAX_RESEND];
            const TUint total = 8 + 4 + 4 * res.n_resend;
            memcpy(gram, "Ohm ", 4);
            gram[4] = 1; gram[5] = 7; gram[6] = (TByte)(total >> 8); gram[7] = (TByte)total;
            auto put = [&](TUint at, uint32_t v) { gram[at] = (TByte)(v >> 24); gram[at + 1] = (TByte)(v >> 16); gram[at + 2] = (TByte)(v >> 8); gram[at + 3] = (TByte)v; };
            put(8, res.n_resend);
            for (TUint k = 0; k < res.n_resend; k++) put(12 + 4 * k, res.resend[k]);
            r.iResendSink->RequestResend(Brn(gram, total));
        }
    }
}

void OhmReceiver::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    Tick tick;
    Collect(aLanes, aCount, tick);
    if (tick.streams.empty()) {
        return;
    }
    TByte* src = nullptr;
    TByte* dst = nullptr;
    aFactory.ReserveArena((size_t)tick.srcBytes, (size_t)std::max<TUint64>(tick.dstBytes, 16), src, dst);
    FillSource(aLanes, tick, src);
    std::vector<ohgpu_ohm_rx_stream_result> results(tick.streams.size());
    std::vector<ohgpu_ohm_rx_record> records(tick.datagrams.size());
    const int err = ohgpu_ohm_rx_process_host(aFactory.Gpu(), tick.streams.data(), tick.streams.size(), tick.datagrams.data(), tick.datagrams.size(),
                                              src, tick.srcBytes, dst, tick.dstBytes, results.data(), records.data());
    ASSERT(err == OHGPU_OK);
    Deliver(aLanes, tick, results.data(), records.data(), dst);
}

} // namespace Av
} // namespace OpenHome
