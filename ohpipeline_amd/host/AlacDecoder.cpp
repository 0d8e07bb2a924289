// AlacDecoder.cpp -- see AlacDecoder.h.
#include "AlacDecoder.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Media {

AlacBatchDecoder::AlacBatchDecoder()
    : iRate(0), iLengthJiffies(0), iConfigured(false), iAnnounced(false), iCorrupt(false), iNextPacket(0), iSamples(0)
{
    memset(&iConfig, 0, sizeof(iConfig));
}

void AlacBatchDecoder::SetConfig(const Brx& aCookie, TUint aTimescale, TUint64 aDuration)
{
    if (ohgpu_alac_config_parse(aCookie.Ptr(), aCookie.Bytes(), &iConfig) != OHGPU_OK || aTimescale == 0) {
        iCorrupt = true;
        THROW(CodecStreamCorrupt);
    }
    if (iConfig.frame_length == 0 || iConfig.frame_length > kFrameLengthMost || iConfig.channels == 0 || iConfig.channels > kChannelsMost) {
        iCorrupt = true;
        THROW(CodecStreamCorrupt);                                    // AlacApple.cpp:147-157, AlacAppleBase.cpp:69-76
    }
    if (iConfig.bit_depth != 16 && iConfig.bit_depth != 20 && iConfig.bit_depth != 24 && iConfig.bit_depth != 32) {
        iCorrupt = true;
        THROW(CodecStreamFeatureUnsupported);
    }
    iRate = aTimescale;                                         // AlacApple.cpp:177: the container's, not the configuration's
    iLengthJiffies = aDuration * Jiffies::kPerSecond / aTimescale;
    iConfigured = true;
}

void AlacBatchDecoder::PushPacket(const Brx& aPacket)
{
    ASSERT(iConfigured);
    iPending.insert(iPending.end(), aPacket.Ptr(), aPacket.Ptr() + aPacket.Bytes());
    iSizes.push_back(aPacket.Bytes());
}

void AlacBatchDecoder::SeekToPacket(TUint64 aIndex)
{
    iPending.clear();
    iSizes.clear();
    iNextPacket = aIndex;
}

void AlacBatchDecoder::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_alac_stream_desc> descs;
    std::vector<ohgpu_alac_packet> packets;
    std::vector<size_t> laneOf;
    TUint64 srcTotal = 0, dstTotal = 0;
    for (size_t k = 0; k < aCount; k++) {
        AlacBatchDecoder& d = *aLanes[k].decoder;
        if (!d.iConfigured || d.iCorrupt || d.iSizes.empty()) {
            continue;
        }
        ohgpu_alac_stream_desc s;
        memset(&s, 0, sizeof(s));
        s.config = d.iConfig;
        s.first_packet = (uint32_t)packets.size();
        s.n_packets = (uint32_t)d.iSizes.size();
        s.dst_offset = dstTotal;
        s.flags = OHGPU_ALAC_OUT_PACKED_LE;
        TUint64 at = srcTotal;
        for (TUint bytes : d.iSizes) {
            ohgpu_alac_packet p = {at, bytes, 0};
            packets.push_back(p);
            at += bytes;
        }
        srcTotal += (d.iPending.size() + 15u) & ~(TUint64)15u;
        dstTotal += ((TUint64)s.n_packets * d.iConfig.frame_length * d.iConfig.channels * (d.iConfig.bit_depth / 8) + 15u) & ~(TUint64)15u;
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
        const AlacBatchDecoder& d = *aLanes[laneOf[i]].decoder;
        memcpy(src + packets[descs[i].first_packet].src_offset, d.iPending.data(), d.iPending.size());
    }
    std::vector<ohgpu_alac_stream_result> results(descs.size());
    std::vector<ohgpu_alac_packet_result> each(packets.size());
    const int err = ohgpu_alac_process_host(aFactory.Gpu(), descs.data(), descs.size(), packets.data(), packets.size(), src, srcTotal, dst, dstTotal,
                                            results.data(), each.data());
    ASSERT(err == OHGPU_OK);
    static const TByte kName[] = {'A', 'L', 'A', 'C'};
    size_t firstBad = descs.size();
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        AlacBatchDecoder& d = *lane.decoder;
        const ohgpu_alac_config& c = d.iConfig;
        const TUint sampleBytes = (c.bit_depth / 8u) * c.channels;
        if (!d.iAnnounced) {
            // AlacApple.cpp:175-185: the PCM's bit rate (the stream is lossless), the container's rate and length
            lane.controller->OutputDecodedStream(d.iRate * sampleBytes * 8, c.bit_depth, d.iRate, c.channels, Brn(kName, sizeof(kName)),
                                                 d.iLengthJiffies, 0, true);
            d.iAnnounced = true;
        }
        for (uint32_t k = 0; k < results[i].packets_ok; k++) {
            // AlacAppleBase.cpp:94-111: a packet leaves in pieces of kMaxPieceBytes, the count restarting with every packet
            const TByte* audio = dst + descs[i].dst_offset + (size_t)k * c.frame_length * sampleBytes;
            const TUint bytes = each[descs[i].first_packet + k].samples * sampleBytes;
            for (TUint done = 0; done < bytes; ) {
                const TUint n = std::min(kMaxPieceBytes, bytes - done);
                lane.trackOffset += lane.controller->OutputAudioPcm(Brn(audio + done, n), c.channels, d.iRate, c.bit_depth, AudioDataEndian::Little,
                                                                    lane.trackOffset);
                done += n;
            }
        }
        d.iSamples += results[i].samples;
        d.iNextPacket += results[i].packets_ok;
        d.iPending.clear();
        d.iSizes.clear();
        if (results[i].packets_ok != descs[i].n_packets) {
            d.iCorrupt = true;
            if (firstBad == descs.size()) firstBad = i;
        }
    }
    if (firstBad != descs.size()) {
        if (results[firstBad].first_bad_status == OHGPU_ALAC_UNSUPPORTED) THROW(CodecStreamFeatureUnsupported);
        THROW(CodecStreamCorrupt);                                    // AlacAppleBase.cpp:85-88
    }
}

} // namespace Media
} // namespace OpenHome
