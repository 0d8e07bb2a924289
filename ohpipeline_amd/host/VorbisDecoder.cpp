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

// Packet `aIndex` of the logical stream whose first page lies at aData: its lacing values joined over that serial's pages.  False when
// the bytes end before the packet does.
static TBool NthPacket(const TByte* aData, size_t aBytes, TUint aIndex, std::vector<TByte>& aOut)
{
    aOut.clear();
    if (aBytes < 27) return false;
    const TByte* const serial = aData + 14;
    TUint done = 0;
    for (size_t at = 0; at + 27 <= aBytes && memcmp(aData + at, "OggS", 4) == 0; ) {
        const TUint segments = aData[at + 26];
        if (at + 27 + segments > aBytes) return false;
        size_t body = at + 27 + segments;
        const TBool mine = memcmp(aData + at + 14, serial, 4) == 0;
        for (TUint s = 0; s < segments; s++) {
            const TUint v = aData[at + 27 + s];
            if (body + v > aBytes) return false;
            if (mine) {
                if (done == aIndex) aOut.insert(aOut.end(), aData + body, aData + body + v);
                if (v < 255) {
                    if (done == aIndex) return true;
                    done++;
                }
            }
            body += v;
        }
        at = body;
    }
    return false;
}

OggVorbisBatchDecoder::OggVorbisBatchDecoder()
    : iHeadKnown(false), iAnnounced(false), iCorrupt(false), iFinished(false), iSamples(0), iConsumed(0), iSerial(0), iNextSeq(0), iResumeSegment(0),
      iObserver(nullptr), iCommentPending(false), iResent(false), iG0Known(false), iAnnouncedChannels(0), iAnnouncedRate(0), iLinkDecoded(0), iG0(0)
{
    memset(&iInfo, 0, sizeof(iInfo));
}

void OggVorbisBatchDecoder::Push(const Brx& aBytes)
{
    iPending.insert(iPending.end(), aBytes.Ptr(), aBytes.Ptr() + aBytes.Bytes());
    if (iFinished && !iCorrupt && !iPending.empty()) {                // bytes behind a link's last page: a further link
        iFinished = false;
        WaitForHeadAt(0);
    }
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
    const int err = ParseHeadAt(0, page);
    if (err == OHGPU_ERR_UNSUPPORTED) {
        iCorrupt = true;
        THROW(CodecStreamFeatureUnsupported);
    }
    if (err != OHGPU_OK) {
        return;                                                       // (not all of it yet)
    }
    iPending.erase(iPending.begin(), iPending.begin() + (size_t)page);
    iConsumed += page;
    iHeadKnown = true;
}

// The head of the link whose first page lies at aOffset of the queue: info, image, serial, comment packet, and where its audio begins
// (aAudioPage from aOffset; the page number and segment for a queue cut there).  The library's code when the head is not whole or not taken.
int OggVorbisBatchDecoder::ParseHeadAt(size_t aOffset, uint64_t& aAudioPage)
{
    const TByte* const bytes = iPending.data() + aOffset;
    const size_t have = iPending.size() - aOffset;
    ohgpu_vorbis_info info;
    uint32_t serial = 0, segment = 0, seq = 0;
    int err = ohgpu_vorbis_head(bytes, have, nullptr, 0, &info, &serial, &aAudioPage, &segment, &seq);
    if (err != OHGPU_OK) {
        return err;
    }
    iInfo = info;
    iImage.resize(iInfo.image_bytes);
    err = ohgpu_vorbis_head(bytes, have, iImage.data(), iImage.size(), &iInfo, &serial, &aAudioPage, &segment, &seq);
    ASSERT(err == OHGPU_OK);
    iCommentPending = NthPacket(bytes, have, 1, iComment);
    iSerial = serial; iNextSeq = seq; iResumeSegment = segment;
    iResent = false; iG0Known = false; iLinkDecoded = 0; iG0 = 0;
    return OHGPU_OK;
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

TBool OggVorbisBatchDecoder::CollectLinks(TUint64 aSrcBase, TUint64 aMidBase, TUint64 aDstBase, TUint aPacketFirst, TUint64 aImageOffset, ohgpu_ogg_stream_desc& aOgg,
                                          ohgpu_vorbis_stream_desc& aVorbis, TUint64& aRegionBytes) const
{
    if (!Collect(aSrcBase, aMidBase, aDstBase, aPacketFirst, aImageOffset, aOgg, aVorbis)) {
        return false;
    }
    aRegionBytes = std::max<TUint64>(2u * aVorbis.max_samples * 2u * iInfo.channels, kMinRegionBytes);
    return true;
}

// The queue from aQueueOffset on begins with a link's first page: everything in front of it goes, and the head is read when it is whole.
void OggVorbisBatchDecoder::WaitForHeadAt(size_t aQueueOffset)
{
    iPending.erase(iPending.begin(), iPending.begin() + aQueueOffset);
    iConsumed += aQueueOffset;
    iHeadKnown = false;
    if (!iPending.empty()) {
        ReadHead();
    }
}

// In front of a link's first PCM: the decoded-stream message if this is the first link or channels or rate changed, then the comment.
void OggVorbisBatchDecoder::BeginLink(CodecController& aController)
{
    static const TByte kName[] = {'V', 'O', 'R', 'B', 'I', 'S'};
    if (!iAnnounced || iAnnouncedChannels != iInfo.channels || iAnnouncedRate != iInfo.sample_rate) {
        aController.OutputDecodedStream(0, 16, iInfo.sample_rate, iInfo.channels, Brn(kName, sizeof(kName)), 0, 0, false);
        iAnnounced = true; iAnnouncedChannels = iInfo.channels; iAnnouncedRate = iInfo.sample_rate;
    }
    if (iCommentPending) {
        if (iObserver) iObserver->NotifyVorbisComment(Brn(iComment.data(), (TUint)iComment.size()));
        iCommentPending = false;
        iComment.clear();
    }
}

// CodecVorbis's pieces: whole samples within DecodedAudio::kMaxBytes
void OggVorbisBatchDecoder::Output(const TByte* aPcm, TUint64 aSamples, CodecController& aController, TUint64& aTrackOffset)
{
    const TUint sampleBytes = 2u * iInfo.channels, perPiece = DecodedAudio::kMaxBytes / sampleBytes;
    for (TUint64 done = 0; done < aSamples; ) {
        const TUint n = (TUint)std::min<TUint64>(perPiece, aSamples - done);
        aTrackOffset += aController.OutputAudioPcm(Brn(aPcm + (size_t)done * sampleBytes, n * sampleBytes), iInfo.channels, iInfo.sample_rate, 16, AudioDataEndian::Big, aTrackOffset);
        done += n;
    }
    iSamples += aSamples;
}

TBool OggVorbisBatchDecoder::ApplyLinks(const ohgpu_ogg_stream_desc& aOgg, const ohgpu_vorbis_stream_desc& aVorbis, TUint64 aRegionBytes, const ohgpu_ogg_stream_result& aDemuxed,
                                        const ohgpu_ogg_packet* aRecords, const ohgpu_vorbis_packet_result* aPacketResults, const ohgpu_vorbis_link* aLinks, size_t aLinkCount,
                                        const TByte* aDst, CodecController& aController, TUint64& aTrackOffset)
{
    const uint32_t recorded = std::min(aDemuxed.packets, aOgg.packet_capacity);
    const TBool all = recorded == aDemuxed.packets;
    TBool waiting = false;                                            // the queue was cut at a link's first page: nothing behind it is this tick's
    for (size_t j = 0; j < aLinkCount && !waiting; j++) {
        const ohgpu_vorbis_link& row = aLinks[j];
        if (j > 0) {
            // a link begins: its head from our own queue, or the wait for it
            const uint32_t frame = row.channels * 2u;
            const TBool room = row.head == OHGPU_OK && row.dst_offset + (TUint64)row.n_packets * (row.blocksize_long / 2u) * frame <= aVorbis.dst_offset + aRegionBytes;
            if (row.head < 0) {
                iCorrupt = true;
                return false;
            }
            if (row.head == OHGPU_VORBIS_LINK_HEAD_OPEN || !room) {
                WaitForHeadAt((size_t)row.page_offset);
                waiting = true;
                break;
            }
            uint64_t audio = 0;
            const int err = ParseHeadAt((size_t)row.page_offset, audio);     // (in place: the tick's records count from the queue's first byte)
            ASSERT(err == OHGPU_OK && iInfo.channels == row.channels && iSerial == row.serial);
        }
        if (row.n_packets == 0) continue;
        BeginLink(aController);
        const uint32_t k0 = row.first_packet - aOgg.packet_first, k1 = k0 + row.n_packets;
        // the link's samples of this tick, packet by packet: where g0 becomes known, and the start trim there
        TUint64 tick = 0, holeAt = 0, hole = 0;
        TInt64 lastGranule = -1;
        for (uint32_t k = k0; k < k1; k++) {
            const ohgpu_vorbis_packet_result& pr = aPacketResults[k];
            const TBool again = j == 0 && k == k0 && iResent;          // the last tick's last packet, sent again to prime: its granule has been seen
            if (pr.status == OHGPU_VORBIS_OK && aRecords[k].granule != -1 && !again) {
                if (!iG0Known) {
                    iG0Known = true;
                    iG0 = aRecords[k].granule - (TInt64)(iLinkDecoded + tick + pr.samples);
                    if (iG0 < 0) { holeAt = tick; hole = std::min<TUint64>((TUint64)(-iG0), pr.samples); }
                }
                lastGranule = aRecords[k].granule;
            }
            tick += pr.samples;
        }
        ASSERT(tick == row.samples);
        const TBool ended = (aRecords[k1 - 1].flags & OHGPU_OGG_PACKET_EOS) != 0 && (j + 1 < aLinkCount || all);
        TUint64 keep = tick;
        if (ended && iG0Known && lastGranule >= 0) {                  // the link's length is its last page's granule position, from g0
            const TInt64 total = lastGranule - iG0;
            keep = total > (TInt64)iLinkDecoded ? std::min<TUint64>(tick, (TUint64)total - iLinkDecoded) : 0;
        }
        const TByte* pcm = aDst + row.dst_offset;
        const TUint frame = 2u * iInfo.channels;
        const TUint64 a = std::min(holeAt, keep), b = std::min(holeAt + hole, keep);
        Output(pcm, a, aController, aTrackOffset);
        Output(pcm + (size_t)b * frame, keep - b, aController, aTrackOffset);
        iLinkDecoded += tick;
        if (ended && j + 1 == aLinkCount) {
            iFinished = true;
        }
    }
    if (!waiting) {
        if (iFinished) {
            // what the page layer left unread is a further link's beginning (or nothing)
            const size_t used = std::min<size_t>((size_t)aDemuxed.bytes_consumed, iPending.size());
            if (used < iPending.size()) { iFinished = false; WaitForHeadAt(used); }
            else { iPending.clear(); iConsumed += used; }
        } else if (recorded > 1 || aLinkCount > 1) {
            const ohgpu_ogg_packet& last = aRecords[recorded - 1];
            iPending.erase(iPending.begin(), iPending.begin() + (size_t)last.page_offset);
            iConsumed += last.page_offset;
            iNextSeq = last.page_seq;
            iResumeSegment = last.segment;
            iResent = true;
        }
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
    std::vector<uint64_t> regions;
    std::vector<TByte> images;
    TUint64 srcTotal = 0, midTotal = 0, dstTotal = 0;
    TUint packetsTotal = 0;
    for (size_t k = 0; k < aCount; k++) {
        const OggVorbisBatchDecoder& d = *aLanes[k].decoder;
        ohgpu_ogg_stream_desc p;
        ohgpu_vorbis_stream_desc s;
        TUint64 region = 0;
        if (!d.CollectLinks(srcTotal, midTotal, dstTotal, packetsTotal, images.size(), p, s, region)) {
            continue;
        }
        regions.push_back(region);
        images.insert(images.end(), d.iImage.begin(), d.iImage.end());
        srcTotal += MsgFactory::ArenaShare(p.src_bytes);
        midTotal += MsgFactory::ArenaShare(p.src_bytes);
        dstTotal += MsgFactory::ArenaShare(region);
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
    std::vector<ohgpu_vorbis_packet_result> decoded(packetsTotal);
    std::vector<ohgpu_vorbis_link> links(descs.size() + packetsTotal);   // (a link is seen by a packet record: no more than these)
    size_t nLinks = 0;
    const int err = ohgpu_ogg_vorbis_links_process_host(aFactory.Gpu(), pages.data(), descs.data(), regions.data(), descs.size(), packets.size(), images.data(), images.size(),
                                                        src, srcTotal, midTotal, dst, dstTotal, demuxed.data(), packets.data(), links.data(), links.size(), &nLinks, decoded.data());
    ASSERT(err == OHGPU_OK && nLinks <= links.size());
    size_t firstBad = descs.size();
    for (size_t i = 0, row = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        size_t rows = 0;
        while (row + rows < nLinks && links[row + rows].stream == i) rows++;
        if (!lane.decoder->ApplyLinks(pages[i], descs[i], regions[i], demuxed[i], packets.data() + pages[i].packet_first, decoded.data() + pages[i].packet_first,
                                      links.data() + row, rows, dst, *lane.controller, lane.trackOffset) &&
            firstBad == descs.size()) {
            firstBad = i;
        }
        row += rows;
    }
    if (firstBad != descs.size()) {
        THROW(CodecStreamCorrupt);
    }
}

} // namespace Media
} // namespace OpenHome
