// RaopReceiver.cpp -- see RaopReceiver.h.
#include "RaopReceiver.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Media {

RaopReceiver::RaopReceiver(IRaopResendSink* aResendSink, IRaopReceiverObserver* aObserver, TUint aMaxFrames)
    : iResendSink(aResendSink), iObserver(aObserver), iMaxFrames(aMaxFrames), iWaiting(0), iConfigured(false), iAnnounced(false), iCorrupt(false), iRepairing(false),
      iNextRequestMs(0), iPackets(0)
{
    ASSERT(aMaxFrames >= 1 && aMaxFrames <= OHGPU_RAOP_RX_MAX_FRAMES);
    memset(&iState, 0, sizeof(iState));
    memset(&iConfig, 0, sizeof(iConfig));
    memset(iKey, 0, sizeof(iKey));
    memset(iIv, 0, sizeof(iIv));
}

RaopReceiver::~RaopReceiver()
{
    for (TByte& b : iKey) *(volatile TByte*)&b = 0;     // the session key does not outlive the session
}

void RaopReceiver::Clear()
{
    iPending.clear();
    iOffsets.clear();
    iSizes.clear();
    iPorts.clear();
    iWaiting = 0;
    iRepairing = false;
}

void RaopReceiver::SetSession(const Brx& aFmtp, const Brx& aKey, const Brx& aIv)
{
    ASSERT(aKey.Bytes() == sizeof(iKey));
    ASSERT(aIv.Bytes() == sizeof(iIv));
    Clear();
    memset(&iState, 0, sizeof(iState));                 // ProtocolRaop::Reset
    iConfigured = false;
    AlacCheckConfig(ohgpu_raop_fmtp_parse((const char*)aFmtp.Ptr(), aFmtp.Bytes(), &iConfig) == OHGPU_OK, iConfig, iCorrupt);
    memcpy(iKey, aKey.Ptr(), sizeof(iKey));
    memcpy(iIv, aIv.Ptr(), sizeof(iIv));
    iConfigured = true;
    iAnnounced = false;
    iCorrupt = false;
}

void RaopReceiver::Push(const Brx& aDatagram, TUint aPort)
{
    ASSERT(iConfigured);
    const size_t at = (iPending.size() + kDatagramAlign - 1) / kDatagramAlign * kDatagramAlign;
    iPending.resize(at, 0);
    iPending.insert(iPending.end(), aDatagram.Ptr(), aDatagram.Ptr() + aDatagram.Bytes());
    iOffsets.push_back((TUint)at);
    iSizes.push_back(aDatagram.Bytes());
    iPorts.push_back((TByte)aPort);
}

void RaopReceiver::SendFlush(TUint aSeq, TUint aTime)
{
    iState.flush_seq = aSeq;
    iState.flush_time = aTime;
}

void RaopReceiver::DropAudio()
{
    // RepairReset: the waiting frames -- the first iWaiting datagrams of the queue -- go, what came since stays
    std::vector<TByte> pending;
    std::vector<TUint> offsets, sizes;
    std::vector<TByte> ports;
    for (size_t k = iWaiting; k < iSizes.size(); k++) {
        const size_t at = (pending.size() + kDatagramAlign - 1) / kDatagramAlign * kDatagramAlign;
        pending.resize(at, 0);
        pending.insert(pending.end(), iPending.begin() + iOffsets[k], iPending.begin() + iOffsets[k] + iSizes[k]);
        offsets.push_back((TUint)at);
        sizes.push_back(iSizes[k]);
        ports.push_back(iPorts[k]);
    }
    iPending.swap(pending);
    iOffsets.swap(offsets);
    iSizes.swap(sizes);
    iPorts.swap(ports);
    iWaiting = 0;
    iRepairing = false;
    iState.running = 0;
}

void RaopReceiver::WriteResendRequest(TUint aSeqStart, TUint aCount, TByte aOut[kResendRequestBytes])
{
    aOut[0] = 0x80;                                     // version 2, no padding, no extension, no csrc
    aOut[1] = 0x80 | 0x55;                              // marker, EResendRequest
    aOut[2] = 0;
    aOut[3] = 1;                                        // sequence number 1
    aOut[4] = (TByte)(aSeqStart >> 8);
    aOut[5] = (TByte)aSeqStart;
    aOut[6] = (TByte)(aCount >> 8);
    aOut[7] = (TByte)aCount;
}

void RaopReceiver::Collect(TUint64 aSrcBase, ohgpu_raop_rx_stream& aStream, std::vector<ohgpu_raop_rx_datagram>& aDatagrams) const
{
    memset(&aStream, 0, sizeof(aStream));
    aStream.first_datagram = (uint32_t)aDatagrams.size();
    aStream.n_datagrams = (uint32_t)iSizes.size();
    aStream.max_frames = iMaxFrames;
    aStream.state_in = iState;
    for (size_t k = 0; k < iSizes.size(); k++) {
        ohgpu_raop_rx_datagram g;
        memset(&g, 0, sizeof(g));
        g.src_offset = aSrcBase + iOffsets[k];
        g.bytes = iSizes[k];
        g.port = iPorts[k];
        aDatagrams.push_back(g);
    }
}

void RaopReceiver::Apply(TUint64 aNowMs, const ohgpu_raop_rx_stream_result& aResult, const ohgpu_raop_rx_record* aRecords)
{
    // events, in arrival order; the waiting datagrams back into the queue by their place in the replay
    std::vector<size_t> keep(aResult.n_pending);
    for (size_t k = 0; k < iSizes.size(); k++) {
        const ohgpu_raop_rx_record& r = aRecords[k];
        if (iObserver != nullptr && (r.events & OHGPU_RAOP_RX_EVENT_NEW_STREAM)) iObserver->NotifyNewStream();
        if (iObserver != nullptr && (r.events & OHGPU_RAOP_RX_EVENT_DELAY)) iObserver->NotifyDelay(aResult.state_out.latency);
        if (r.disposition == OHGPU_RAOP_RX_PENDING) {
            ASSERT(r.order < keep.size());
            keep[r.order] = k;
        }
    }
    std::vector<TByte> pending;
    std::vector<TUint> offsets, sizes;
    std::vector<TByte> ports;
    for (size_t k : keep) {
        const size_t at = (pending.size() + kDatagramAlign - 1) / kDatagramAlign * kDatagramAlign;
        pending.resize(at, 0);
        pending.insert(pending.end(), iPending.begin() + iOffsets[k], iPending.begin() + iOffsets[k] + iSizes[k]);
        offsets.push_back((TUint)at);
        sizes.push_back(iSizes[k]);
        ports.push_back(iPorts[k]);
    }
    iPending.swap(pending);
    iOffsets.swap(offsets);
    iSizes.swap(sizes);
    iPorts.swap(ports);
    iWaiting = aResult.n_pending;
    iState = aResult.state_out;
    iPackets += aResult.n_output;
    if (aResult.stop_reason != OHGPU_RAOP_RX_STOP_NONE) {
        // the reference closes its servers and drains: what was not reached is gone with them
        iRepairing = false;
        if (iObserver != nullptr) iObserver->NotifyDiscontinuity(aResult.stop_reason);
        return;
    }
    if (aResult.n_pending == 0) {
        iRepairing = false;
        return;
    }
    if (!iRepairing) {                                  // RepairBegin: the timer is set
        iRepairing = true;
        iNextRequestMs = aNowMs + kInitialRepairTimeoutMs;
    }
    if (aNowMs >= iNextRequestMs) {                     // TimerRepairExpired
        if (iResendSink != nullptr)
            for (uint32_t k = 0; k < aResult.n_ranges; k++) iResendSink->RequestResend(aResult.ranges[k].start, (aResult.ranges[k].end - aResult.ranges[k].start) + 1);
        iNextRequestMs = aNowMs + kSubsequentRepairTimeoutMs;
    }
}

void RaopReceiver::Tick(TUint64 aNowMs, MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_raop_rx_stream> streams;
    std::vector<ohgpu_raop_stream_desc> descs;
    std::vector<ohgpu_raop_rx_datagram> datagrams;
    std::vector<size_t> laneOf;
    std::vector<TUint64> base;
    TUint64 srcTotal = 0, dstTotal = 0;
    for (size_t k = 0; k < aCount; k++) {
        RaopReceiver& r = *aLanes[k].receiver;
        if (!r.iConfigured || r.iCorrupt || r.iSizes.empty()) {
            continue;
        }
        ohgpu_raop_rx_stream s;
        r.Collect(srcTotal, s, datagrams);
        ohgpu_raop_stream_desc d;
        memset(&d, 0, sizeof(d));
        d.alac.config = r.iConfig;
        d.alac.dst_offset = dstTotal;
        d.alac.flags = OHGPU_ALAC_OUT_PACKED_LE;
        memcpy(d.aes_key, r.iKey, sizeof(r.iKey));
        memcpy(d.aes_iv, r.iIv, sizeof(r.iIv));
        base.push_back(srcTotal);
        srcTotal += MsgFactory::ArenaShare(r.iPending.size());
        dstTotal += MsgFactory::ArenaShare((TUint64)s.n_datagrams * r.iConfig.frame_length * r.iConfig.channels * (r.iConfig.bit_depth / 8));
        streams.push_back(s);
        descs.push_back(d);
        laneOf.push_back(k);
    }
    if (streams.empty()) {
        return;
    }
    TByte* src = nullptr;
    TByte* dst = nullptr;
    aFactory.ReserveArena((size_t)srcTotal, (size_t)dstTotal, src, dst);
    for (size_t i = 0; i < streams.size(); i++) {
        const RaopReceiver& r = *aLanes[laneOf[i]].receiver;
        memcpy(src + base[i], r.iPending.data(), r.iPending.size());
    }
    std::vector<ohgpu_raop_rx_stream_result> results(streams.size());
    std::vector<ohgpu_raop_rx_record> records(datagrams.size());
    std::vector<ohgpu_alac_stream_result> decoded(streams.size());
    std::vector<ohgpu_alac_packet_result> each(datagrams.size());
    const int err = ohgpu_raop_rx_alac_process_host(aFactory.Gpu(), streams.data(), descs.data(), streams.size(), datagrams.data(), datagrams.size(), src, srcTotal, dst,
                                                    dstTotal, results.data(), records.data(), nullptr, decoded.data(), each.data());
    for (ohgpu_raop_stream_desc& d : descs) for (uint8_t& b : d.aes_key) *(volatile uint8_t*)&b = 0;
    ASSERT(err == OHGPU_OK);
    const ohgpu_alac_stream_result* firstBad = nullptr;
    for (size_t i = 0; i < streams.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        RaopReceiver& r = *lane.receiver;
        r.Apply(aNowMs, results[i], records.data() + streams[i].first_datagram);
        // the packets that came out are the first n_output rows of the stream's share of the tables
        ohgpu_alac_stream_desc out = descs[i].alac;
        out.first_packet = streams[i].first_datagram;
        out.n_packets = results[i].n_output;
        const TBool ok = AlacDeliver(*lane.controller, lane.trackOffset, r.iAnnounced, r.iConfig.sample_rate, 0, out, decoded[i], each.data(), dst);
        if (!ok) {
            r.iCorrupt = true;
            if (firstBad == nullptr) firstBad = &decoded[i];
        }
    }
    AlacThrowFirstBad(firstBad);
}

} // namespace Media
} // namespace OpenHome
