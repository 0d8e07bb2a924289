// OggFlacDecoder.cpp -- see OggFlacDecoder.h.
#include "OggFlacDecoder.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Media {

FlacStreamKind FlacRecognise(const Brx& aBytes)
{
    const TByte* p = aBytes.Ptr();
    if (aBytes.Bytes() < 4) return FlacStreamKind::None;
    if (memcmp(p, "fLaC", 4) == 0) return FlacStreamKind::Native;
    if (memcmp(p, "OggS", 4) == 0 && aBytes.Bytes() >= 42 && memcmp(p + 37, "fLaC", 4) == 0) return FlacStreamKind::Ogg;
    return FlacStreamKind::None;
}

OggFlacBatchDecoder::OggFlacBatchDecoder()
    : iInfoKnown(false), iAnnounced(false), iCorrupt(false), iNextSample(0), iSerial(0), iNextSeq(0), iResumeSegment(0)
{
    memset(&iInfo, 0, sizeof(iInfo));
}

void OggFlacBatchDecoder::Push(const Brx& aFileBytes)
{
    iPending.insert(iPending.end(), aFileBytes.Ptr(), aFileBytes.Ptr() + aFileBytes.Bytes());
    if (!iInfoKnown) {
        ReadHead();
    }
}

void OggFlacBatchDecoder::ReadHead()
{
    // what can be told from the first bytes is told at once; the rest waits until the library finds the head whole
    const size_t have = iPending.size();
    if (memcmp(iPending.data(), "OggS", std::min<size_t>(have, 4)) != 0 ||
        (have >= 42 && FlacRecognise(Brn(iPending.data(), 42)) != FlacStreamKind::Ogg)) {
        iCorrupt = true;
        THROW(CodecStreamCorrupt);
    }
    if (have < 42) {
        return;
    }
    uint64_t page = 0;
    uint32_t serial = 0, segment = 0, seq = 0;
    const int err = ohgpu_ogg_flac_head(iPending.data(), have, &iInfo, &serial, &page, &segment, &seq);
    if (err == OHGPU_ERR_UNSUPPORTED) {
        THROW(CodecStreamFeatureUnsupported);                         // (a metadata block that shares its packet with audio)
    }
    if (err != OHGPU_OK) {
        return;                                                       // (not all of it yet)
    }
    if (iInfo.bits != 8 && iInfo.bits != 16 && iInfo.bits != 24) {
        THROW(CodecStreamFeatureUnsupported);                         // Flac.cpp:404-406
    }
    iPending.erase(iPending.begin(), iPending.begin() + (size_t)page);
    iSerial = serial; iNextSeq = seq; iResumeSegment = segment;
    iInfoKnown = true;
}

void OggFlacBatchDecoder::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    std::vector<ohgpu_ogg_stream_desc> pages;
    std::vector<ohgpu_flac_stream_desc> descs;
    std::vector<size_t> laneOf;
    TUint64 srcTotal = 0, midTotal = 0, dstTotal = 0, framesMax = 0, packetsTotal = 0;
    for (size_t k = 0; k < aCount; k++) {
        OggFlacBatchDecoder& d = *aLanes[k].decoder;
        if (!d.iInfoKnown || d.iCorrupt || d.iPending.empty()) {
            continue;
        }
        const ohgpu_flac_streaminfo_t& info = d.iInfo;
        // a packet is a frame, and no frame is shorter than its header, a byte per subframe and the CRC-16
        const TUint64 frames = d.iPending.size() / std::max<TUint64>(info.min_framesize, 7u + info.channels) + 1;
        TUint64 samples = std::min<TUint64>(frames * info.max_blocksize, FlacBatchDecoder::kMaxSamplesPerTick);
        if (info.total_samples != 0) {
            samples = std::min<TUint64>(samples, info.total_samples - std::min<TUint64>(info.total_samples, d.iNextSample));
        }
        ohgpu_ogg_stream_desc p;
        memset(&p, 0, sizeof(p));
        p.src_offset = srcTotal;
        p.src_bytes = (uint32_t)d.iPending.size();
        p.dst_offset = midTotal;
        p.dst_capacity = p.src_bytes;
        p.serial = d.iSerial;
        p.expect_seq = d.iNextSeq;
        p.first_page_segment = d.iResumeSegment;
        p.packet_first = (uint32_t)packetsTotal;
        p.packet_capacity = (uint32_t)frames + 16u;
        p.flags = OHGPU_OGG_FLAC_MAPPING;
        ohgpu_flac_stream_desc s;
        memset(&s, 0, sizeof(s));
        s.src_offset = midTotal;
        s.dst_offset = dstTotal;
        s.first_sample = d.iNextSample;
        s.max_samples = (uint32_t)std::max<TUint64>(samples, info.max_blocksize);
        s.sample_rate = info.sample_rate;
        s.blocksize = info.min_blocksize == info.max_blocksize ? info.max_blocksize : 0;
        s.max_blocksize = info.max_blocksize;
        s.channels = info.channels;
        s.bits = info.bits;
        s.flags = OHGPU_FLAC_FLAG_AT_FRAME | OHGPU_FLAC_OUT_PACKED_BE;
        srcTotal += MsgFactory::ArenaShare(p.src_bytes);
        midTotal += MsgFactory::ArenaShare(p.src_bytes);
        dstTotal += MsgFactory::ArenaShare((TUint64)s.max_samples * info.channels * (info.bits / 8));
        packetsTotal += p.packet_capacity;
        framesMax += frames;
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
        const OggFlacBatchDecoder& d = *aLanes[laneOf[i]].decoder;
        memcpy(src + pages[i].src_offset, d.iPending.data(), d.iPending.size());
    }
    std::vector<ohgpu_ogg_stream_result> demuxed(descs.size());
    std::vector<ohgpu_ogg_packet> packets((size_t)packetsTotal);
    std::vector<ohgpu_flac_stream_result> results(descs.size());
    std::vector<ohgpu_flac_frame> frames((size_t)framesMax);
    size_t nFrames = 0;
    const int err = ohgpu_ogg_flac_process_host(aFactory.Gpu(), pages.data(), descs.data(), descs.size(), packets.size(), src, srcTotal, midTotal, dst, dstTotal,
                                                demuxed.data(), packets.data(), results.data(), frames.data(), frames.size(), &nFrames);
    ASSERT(err == OHGPU_OK && nFrames <= frames.size());
    static const TByte kName[] = {'F', 'L', 'A', 'C'};
    size_t at = 0, firstBad = descs.size();
    bool firstBadUnsupported = false;
    for (size_t i = 0; i < descs.size(); i++) {
        Lane& lane = aLanes[laneOf[i]];
        OggFlacBatchDecoder& d = *lane.decoder;
        const ohgpu_flac_streaminfo_t& info = d.iInfo;
        const TUint sampleBytes = (info.bits / 8u) * info.channels;
        if (!d.iAnnounced) {
            // Flac.cpp:427-441: bit rate = rate x depth x channels, lossless
            lane.controller->OutputDecodedStream(info.sample_rate * info.bits * info.channels, info.bits, info.sample_rate, info.channels,
                                                 Brn(kName, sizeof(kName)), info.total_samples * Jiffies::kPerSecond / info.sample_rate, 0, true);
            d.iAnnounced = true;
        }
        for (; at < nFrames && frames[at].stream == i; at++) {
            // Flac.cpp:379-417: a frame leaves in pieces of whole samples within kMaxPieceBytes, the count restarting with every frame
            const TByte* audio = dst + descs[i].dst_offset + (frames[at].first_sample - descs[i].first_sample) * sampleBytes;
            const TUint perPiece = FlacBatchDecoder::PieceSamples(info.channels, info.bits);
            for (TUint done = 0; done < frames[at].blocksize; ) {
                const TUint n = std::min(perPiece, frames[at].blocksize - done);
                lane.trackOffset += lane.controller->OutputAudioPcm(Brn(audio + (size_t)done * sampleBytes, n * sampleBytes), info.channels, info.sample_rate,
                                                                    info.bits, AudioDataEndian::Big, lane.trackOffset);
                done += n;
            }
        }
        d.iNextSample += results[i].samples;
        bool bad = demuxed[i].status != OHGPU_OGG_OK || results[i].status == OHGPU_FLAC_CORRUPT || results[i].status == OHGPU_FLAC_UNSUPPORTED;
        if (!bad && results[i].bytes_consumed == demuxed[i].bytes_delivered) {
            // every delivered packet was decoded: go on where the page layer says
            d.iPending.erase(d.iPending.begin(), d.iPending.begin() + (size_t)demuxed[i].bytes_consumed);
            d.iNextSeq = demuxed[i].next_seq;
            d.iResumeSegment = demuxed[i].resume_segment;
        } else if (!bad) {
            // the FLAC layer stopped short (OHGPU_FLAC_OVERFLOW: this tick's arena is full): the packet table maps its bytes_consumed
            // back to a page and a segment
            const ohgpu_ogg_packet* first = packets.data() + pages[i].packet_first;
            const uint32_t recorded = std::min(demuxed[i].packets, pages[i].packet_capacity);
            const ohgpu_ogg_packet* hit = nullptr;
            for (uint32_t k = 0; k < recorded && !hit; k++) {
                if (first[k].run_pos == results[i].bytes_consumed && first[k].bytes != 0) hit = first + k;
            }
            if (hit) {
                d.iPending.erase(d.iPending.begin(), d.iPending.begin() + (size_t)hit->page_offset);
                d.iNextSeq = hit->page_seq;
                d.iResumeSegment = hit->segment;
            } else {
                bad = true;                                           // (no packet begins there: these are no FLAC frames in packets)
            }
        }
        if (bad) {
            d.iCorrupt = true;
            if (firstBad == descs.size()) {
                firstBad = i;
                firstBadUnsupported = demuxed[i].status == OHGPU_OGG_OK && results[i].status == OHGPU_FLAC_UNSUPPORTED;
            }
        }
    }
    if (firstBad != descs.size()) {
        if (firstBadUnsupported) THROW(CodecStreamFeatureUnsupported);
        THROW(CodecStreamCorrupt);                                    // Flac.cpp:249-251, :421-425
    }
}

} // namespace Media
} // namespace OpenHome
