// VorbisDecoder.cpp -- see VorbisDecoder.h.
#include "VorbisDecoder.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Media {

TBool VorbisRecognise(const Brx& aBytes)
{
    const TByte* p = aBytes.Ptr();
    if (aBytes.Bytes() < 28 || memcmp(p, "OggS", 4) != 0) return false;
    const TUint body = 27u + p[26];
    return aBytes.Bytes() >= body + 7u && p[body] == 1 && memcmp(p + body + 1, "vorbis", 6) == 0;
}

OggVorbisBatchDecoder::OggVorbisBatchDecoder()
    : iHeadKnown(false), iAnnounced(false), iCorrupt(false), iFinished(false), iSamples(0), iConsumed(0), iSerial(0), iNextSeq(0), iResumeSegment(0)
{
    memset(&iInfo, 0, sizeof(iInfo));
}

void OggVorbisBatchDecoder::Push(const Brx& aBytes)
{
    iPending.insert(iPending.end(), aBytes.Ptr(), aBytes.Ptr() + aBytes.Bytes());
    if (!iHeadKnown && !iPending.empty()) {
        ReadHead();
    }
}

void OggVorbisBatchDecoder::ReadHead()
{
    // what can be told from the first bytes is told at once; the rest waits until the library finds the head whole
    const size_t have = iPending.size();
    const size_t body = have >= 27 ? 27u + iPending[26] : 0;
    if (memcmp(iPending.data(), "OggS", std::min<size_t>(have, 4)) != 0 || (have >= 27 && have >= body + 7 && !VorbisRecognise(Brn(iPending.data(), (TUint)(body + 7))))) {
        iCorrupt = true;
        THROW(CodecStreamCorrupt);
    }
    if (have < 27 || have < body + 7) {
        return;
    }
    uint64_t page = 0;
    uint32_t serial = 0, segment = 0, seq = 0;
    int err = ohgpu_vorbis_head(iPending.data(), have, nullptr, 0, &iInfo, &serial, &page, &segment, &seq);
    if (err == OHGPU_ERR_UNSUPPORTED) {
        iCorrupt = true;
        THROW(CodecStreamFeatureUnsupported);
    }
    if (err != OHGPU_OK) {
        return;                                                       // (not all of it yet)
    }
    iImage.resize(iInfo.image_bytes);
    err = ohgpu_vorbis_head(iPending.data(), have, iImage.data(), iImage.size(), &iInfo, &serial, &page, &segment, &seq);
    ASSERT(err == OHGPU_OK);
    iPending.erase(iPending.begin(), iPending.begin() + (size_t)page);
    iConsumed = page;
    iSerial = serial; iNextSeq = seq; iResumeSegment = segment;
    iHeadKnown = true;
}

TBool OggVorbisBatchDecoder::Collect(TUint64 aSrcBase, TUint64 aMidBase, TUint64 aDstBase, TUint aPacketFirst, TUint64 aImageOffset, ohgpu_ogg_stream_desc& aOgg,
                                     ohgpu_vorbis_stream_desc& aVorbis) const
{
    if (!iHeadKnown || iCorrupt || iFinished || iPending.empty()) {
        return false;
    }
    memset(&aOgg, 0, sizeof(aOgg));
    aOgg.src_offset = aSrcBase;
    aOgg.src_bytes = (uint32_t)iPending.size();
    aOgg.dst_offset = aMidBase;
    aOgg.dst_capacity = aOgg.src_bytes;
    aOgg.serial = iSerial;
    aOgg.expect_seq = iNextSeq;
    aOgg.first_page_segment = iResumeSegment;
    aOgg.packet_first = aPacketFirst;
    aOgg.packet_capacity = kMaxPacketsPerTick;
    memset(&aVorbis, 0, sizeof(aVorbis));
    aVorbis.image_offset = aImageOffset;
    aVorbis.image_bytes = (uint32_t)iImage.size();
    aVorbis.dst_offset = aDstBase;
    aVorbis.max_samples = (TUint64)kMaxPacketsPerTick * (iInfo.blocksize_long / 2u);      // (a packet delivers half a long block at most)
    return true;
}

TBool OggVorbisBatchDecoder::Apply(const ohgpu_ogg_stream_desc& aOgg, const ohgpu_ogg_stream_result& aDemuxed, const ohgpu_ogg_packet* aRecords,
                                   const ohgpu_vorbis_stream_result& aDecoded, const TByte* aPcm, CodecController& aController, TUint64& aTrackOffset)
{
    static const TByte kName[] = {'V', 'O', 'R', 'B', 'I', 'S'};
    const TUint channels = iInfo.channels, sampleBytes = 2u * channels;
    if (!iAnnounced) {
        aController.OutputDecodedStream(0, 16, iInfo.sample_rate, channels, Brn(kName, sizeof(kName)), 0, 0, false);
        iAnnounced = true;
    }
    const uint32_t recorded = std::min(aDemuxed.packets, aOgg.packet_capacity);
    // every recorded packet was decoded; the last of them is the next tick's first
    TUint64 samples = aDecoded.samples;
    const TBool all = recorded == aDemuxed.packets;                  // (else the page layer went on past the records: its end state is not ours)
    if (all && aDemuxed.eos_seen && aDemuxed.last_granule >= 0) {
        // the stream ends in this tick: its length is the last page's granule position
        const TUint64 total = (TUint64)aDemuxed.last_granule;
        samples = std::min<TUint64>(samples, total > iSamples ? total - iSamples : 0);
        iFinished = true;
    }
    // CodecVorbis's pieces: whole samples within DecodedAudio::kMaxBytes
    const TUint perPiece = DecodedAudio::kMaxBytes / sampleBytes;
    for (TUint64 done = 0; done < samples; ) {
        const TUint n = (TUint)std::min<TUint64>(perPiece, samples - done);
        aTrackOffset += aController.OutputAudioPcm(Brn(aPcm + (size_t)done * sampleBytes, n * sampleBytes), channels, iInfo.sample_rate, 16, AudioDataEndian::Big, aTrackOffset);
        done += n;
    }
    iSamples += samples;
    if (iFinished) {
        iPending.clear();
    } else if (recorded > 1) {
        const ohgpu_ogg_packet& last = aRecords[recorded - 1];
        iPending.erase(iPending.begin(), iPending.begin() + (size_t)last.page_offset);
        iConsumed += last.page_offset;
        iNextSeq = last.page_seq;
        iResumeSegment = last.segment;
    }
    if (aDemuxed.status != OHGPU_OGG_OK) {
        iCorrupt = true;
        return false;
    }
    return true;
}

void OggVorbisBatchDecoder::Tick(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_ogg_stream_desc> pages;
    std::vector<ohgpu_vorbis_stream_desc> descs;
    std::vector<size_t> laneOf;
    std::vector<TByte> images;
    TUint64 srcTotal = 0, midTotal = 0, dstTotal = 0;
    TUint packetsTotal = 0;
    for (size_t k = 0; k < aCount; k++) {
        const OggVorbisBatchDecoder& d = *aLanes[k].decoder;
        ohgpu_ogg_stream_desc p;
        ohgpu_vorbis_stream_desc s;
        if (!d.Collect(srcTotal, midTotal, dstTotal, packetsTotal, images.size(), p, s)) {
            continue;
        }
        images.insert(images.end(), d.iImage.begin(), d.iImage.end());
        srcTotal += MsgFactory::ArenaShare(p.src_bytes);
        midTotal += MsgFactory::ArenaShare(p.src_bytes);
        dstTotal += MsgFactory::ArenaShare(s.max_samples * 2u * d.iInfo.channels);
        packetsTotal += p.packet_capacity;
        pages.push_back(p);
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
        const OggVorbisBatchDecoder& d = *aLanes[laneOf[i]].decoder;
        memcpy(src + pages[i].src_offset, d.iPending.data(), d.iPending.size());
    }
    std::vector<ohgpu_ogg_stream_result> demuxed(descs.size());
    std::vector<ohgpu_ogg_packet> packets(packetsTotal);
    std::vector<ohgpu_vorbis_stream_result> results(descs.size());
    const int err = ohgpu_ogg_vorbis_process_host(aFactory.Gpu(), pages.data(), descs.data(), descs.size(), packets.size(), images.data(), images.size(), src, srcTotal,
                                                  midTotal, dst, dstTotal, demuxed.data(), packets.data(), results.data(), nullptr);
    ASSERT(err == OHGPU_OK);
    size_t firstBad = descs.size();
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        if (!lane.decoder->Apply(pages[i], demuxed[i], packets.data() + pages[i].packet_first, results[i], dst + descs[i].dst_offset, *lane.controller, lane.trackOffset) &&
            firstBad == descs.size()) {
            firstBad = i;
        }
    }
    if (firstBad != descs.size()) {
        THROW(CodecStreamCorrupt);
    }
}

} // namespace Media
} // namespace OpenHome
