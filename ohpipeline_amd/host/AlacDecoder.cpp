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

void AlacCheckConfig(TBool aParsed, const ohgpu_alac_config& aConfig, TBool& aCorrupt)
{
    const TBool was = aCorrupt;
    aCorrupt = true;                                                  // (while a check can throw)
    if (!aParsed) THROW(CodecStreamCorrupt);                          // AlacApple.cpp:147-157; CodecRaopApple.cpp:80-83, 211-213
    if (aConfig.frame_length == 0 || aConfig.frame_length > AlacBatchDecoder::kFrameLengthMost || aConfig.channels == 0
        || aConfig.channels > AlacBatchDecoder::kChannelsMost) THROW(CodecStreamCorrupt);   // AlacAppleBase.cpp:69-76; CodecRaopApple.cpp:85-94
    if (aConfig.bit_depth != 16 && aConfig.bit_depth != 20 && aConfig.bit_depth != 24 && aConfig.bit_depth != 32) THROW(CodecStreamFeatureUnsupported);
    aCorrupt = was;
}

void AlacBatchDecoder::SetConfig(const Brx& aCookie, TUint aTimescale, TUint64 aDuration)
{
    AlacCheckConfig(ohgpu_alac_config_parse(aCookie.Ptr(), aCookie.Bytes(), &iConfig) == OHGPU_OK && aTimescale != 0, iConfig, iCorrupt);
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

TBool AlacDeliver(CodecController& aController, TUint64& aTrackOffset, TBool& aAnnounced, TUint aRate, TUint64 aLengthJiffies,
                  const ohgpu_alac_stream_desc& aDesc, const ohgpu_alac_stream_result& aResult, const ohgpu_alac_packet_result* aEach, const TByte* aDst)
{
    static const TByte kName[] = {'A', 'L', 'A', 'C'};
    const ohgpu_alac_config& c = aDesc.config;
    const TUint sampleBytes = (c.bit_depth / 8u) * c.channels;
    if (!aAnnounced) {
        // AlacApple.cpp:175-185, CodecRaopApple.cpp:109-117: the PCM's bit rate (the stream is lossless)
        aController.OutputDecodedStream(aRate * sampleBytes * 8, c.bit_depth, aRate, c.channels, Brn(kName, sizeof(kName)), aLengthJiffies, 0, true);
        aAnnounced = true;
    }
    for (uint32_t k = 0; k < aResult.packets_ok; k++) {
        // AlacAppleBase.cpp:94-111: a packet leaves in pieces of kMaxPieceBytes, the count restarting with every packet
        const TByte* audio = aDst + aDesc.dst_offset + (size_t)k * c.frame_length * sampleBytes;
        const TUint bytes = aEach[aDesc.first_packet + k].samples * sampleBytes;
        for (TUint done = 0; done < bytes; ) {
            const TUint n = std::min(AlacBatchDecoder::kMaxPieceBytes, bytes - done);
            aTrackOffset += aController.OutputAudioPcm(Brn(audio + done, n), c.channels, aRate, c.bit_depth, AudioDataEndian::Little, aTrackOffset);
            done += n;
        }
    }
    return aResult.packets_ok == aDesc.n_packets;
}

void AlacThrowFirstBad(const ohgpu_alac_stream_result* aFirstBad)
{
    if (aFirstBad != nullptr && aFirstBad->first_bad_status == OHGPU_ALAC_UNSUPPORTED) THROW(CodecStreamFeatureUnsupported);
    if (aFirstBad != nullptr) THROW(CodecStreamCorrupt);              // AlacAppleBase.cpp:85-88
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
        srcTotal += MsgFactory::ArenaShare(d.iPending.size());
        dstTotal += MsgFactory::ArenaShare((TUint64)s.n_packets * d.iConfig.frame_length * d.iConfig.channels * (d.iConfig.bit_depth / 8));
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
    const ohgpu_alac_stream_result* firstBad = nullptr;
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        AlacBatchDecoder& d = *lane.decoder;
        // AlacApple.cpp:175-185: the container's rate and length are what is announced
        const TBool ok = AlacDeliver(*lane.controller, lane.trackOffset, d.iAnnounced, d.iRate, d.iLengthJiffies, descs[i], results[i], each.data(), dst);
        d.iSamples += results[i].samples;
        d.iNextPacket += results[i].packets_ok;
        d.iPending.clear();
        d.iSizes.clear();
        if (!ok) {
            d.iCorrupt = true;
            if (firstBad == nullptr) firstBad = &results[i];
        }
    }
    AlacThrowFirstBad(firstBad);
}

} // namespace Media
} // namespace OpenHome
