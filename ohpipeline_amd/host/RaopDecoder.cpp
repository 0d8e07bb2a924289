// RaopDecoder.cpp -- see RaopDecoder.h.
#include "RaopDecoder.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Media {

RaopBatchDecoder::RaopBatchDecoder()
    : iPendingBytes(0), iLastSeq(0), iLastTimestamp(0), iLastSsrc(0), iConfigured(false), iAnnounced(false), iCorrupt(false), iSamples(0), iPackets(0)
{
    memset(&iConfig, 0, sizeof(iConfig));
    memset(iKey, 0, sizeof(iKey));
    memset(iIv, 0, sizeof(iIv));
}

RaopBatchDecoder::~RaopBatchDecoder()
{
    for (TByte& b : iKey) *(volatile TByte*)&b = 0;     // the session key does not outlive the session
}

void RaopBatchDecoder::Drop()
{
    iPending.clear();
    iOffsets.clear();
    iSizes.clear();
    iPendingBytes = 0;
}

void RaopBatchDecoder::SetSession(const Brx& aFmtp, const Brx& aKey, const Brx& aIv)
{
    ASSERT(aKey.Bytes() == kKeyBytes);
    ASSERT(aIv.Bytes() == kKeyBytes);
    Drop();
    iConfigured = false;
    AlacCheckConfig(ohgpu_raop_fmtp_parse((const char*)aFmtp.Ptr(), aFmtp.Bytes(), &iConfig) == OHGPU_OK, iConfig, iCorrupt);
    memcpy(iKey, aKey.Ptr(), kKeyBytes);
    memcpy(iIv, aIv.Ptr(), kKeyBytes);
    iConfigured = true;
    iAnnounced = false;
    iCorrupt = false;
}

void RaopBatchDecoder::PushDatagram(const Brx& aRtp)
{
    ASSERT(iConfigured);
    const TUint bytes = aRtp.Bytes();
    if (bytes > kMaxDatagramBytes || bytes < kRtpHeaderBytes || bytes - kRtpHeaderBytes < kAudioHeaderBytes) {
        THROW(InvalidRaopPacket);                                     // ProtocolRaop.cpp:169-176, 222-229
    }
    const TByte* p = aRtp.Ptr();
    iLastSeq = ((TUint)p[2] << 8) | p[3];
    iLastTimestamp = ((TUint)p[4] << 24) | ((TUint)p[5] << 16) | ((TUint)p[6] << 8) | p[7];
    iLastSsrc = ((TUint)p[8] << 24) | ((TUint)p[9] << 16) | ((TUint)p[10] << 8) | p[11];
    const TUint header = kRtpHeaderBytes + kAudioHeaderBytes;
    const size_t at = (iPending.size() + kPayloadAlign - 1) / kPayloadAlign * kPayloadAlign;
    iPending.resize(at, 0);
    iPending.insert(iPending.end(), p + header, p + bytes);
    iOffsets.push_back((TUint)at);
    iSizes.push_back(bytes - header);
    iPendingBytes += bytes - header;
}

void RaopBatchDecoder::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_raop_stream_desc> descs;
    std::vector<ohgpu_alac_packet> packets;
    std::vector<size_t> laneOf;
    std::vector<TUint64> base;
    TUint64 srcTotal = 0, dstTotal = 0;
    for (size_t k = 0; k < aCount; k++) {
        RaopBatchDecoder& d = *aLanes[k].decoder;
        if (!d.iConfigured || d.iCorrupt || d.iSizes.empty()) {
            continue;
        }
        ohgpu_raop_stream_desc s;
        memset(&s, 0, sizeof(s));
        s.alac.config = d.iConfig;
        s.alac.first_packet = (uint32_t)packets.size();
        s.alac.n_packets = (uint32_t)d.iSizes.size();
        s.alac.dst_offset = dstTotal;
        s.alac.flags = OHGPU_ALAC_OUT_PACKED_LE;
        memcpy(s.aes_key, d.iKey, kKeyBytes);
        memcpy(s.aes_iv, d.iIv, kKeyBytes);
        for (size_t i = 0; i < d.iSizes.size(); i++) {
            ohgpu_alac_packet p = {srcTotal + d.iOffsets[i], d.iSizes[i], 0};       // (a multiple of 16 each: the ABI asks for 4)
            packets.push_back(p);
        }
        base.push_back(srcTotal);
        srcTotal += MsgFactory::ArenaShare(d.iPending.size());
        dstTotal += MsgFactory::ArenaShare((TUint64)s.alac.n_packets * d.iConfig.frame_length * d.iConfig.channels * (d.iConfig.bit_depth / 8));
        descs.push_back(s);
        laneOf.push_back(k);
    }
    if (descs.empty()) {
        return;
    }
    TByte* src = nullptr;
    TByte* dst = nullptr;
    aFactory.ReserveArena((size_t)srcTotal, (size_t)dstTotal, src, dst);
    for (size_t i = 0; i < descs.size(); i++) {
        const RaopBatchDecoder& d = *aLanes[laneOf[i]].decoder;
        memcpy(src + base[i], d.iPending.data(), d.iPending.size());
    }
    std::vector<ohgpu_alac_stream_result> results(descs.size());
    std::vector<ohgpu_alac_packet_result> each(packets.size());
    const int err = ohgpu_raop_process_host(aFactory.Gpu(), descs.data(), descs.size(), packets.data(), packets.size(), src, srcTotal, dst, dstTotal,
                                            results.data(), each.data());
    for (ohgpu_raop_stream_desc& s : descs) for (uint8_t& b : s.aes_key) *(volatile uint8_t*)&b = 0;
    ASSERT(err == OHGPU_OK);
    const ohgpu_alac_stream_result* firstBad = nullptr;
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        RaopBatchDecoder& d = *lane.decoder;
        // CodecRaopApple.cpp:109-117: the fmtp's sample rate and no track length are what is announced
        const TBool ok = AlacDeliver(*lane.controller, lane.trackOffset, d.iAnnounced, d.iConfig.sample_rate, 0, descs[i].alac, results[i], each.data(), dst);
        d.iSamples += results[i].samples;
        d.iPackets += results[i].packets_ok;
        d.Drop();
        if (!ok) {
            d.iCorrupt = true;
            if (firstBad == nullptr) firstBad = &results[i];
        }
    }
    AlacThrowFirstBad(firstBad);
}

} // namespace Media
} // namespace OpenHome
