// Mpeg4AlacDecoder.cpp -- see Mpeg4AlacDecoder.h.
#include "Mpeg4AlacDecoder.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Media {

TBool Mpeg4Recognise(const Brx& aBytes)
{
    return aBytes.Bytes() >= 8 && memcmp(aBytes.Ptr() + 4, "ftyp", 4) == 0;
}

Mpeg4AlacBatchDecoder::Mpeg4AlacBatchDecoder()
    : iPeekAt(0), iExtent(0), iMoovEnd(0), iNext(0), iBoxes(0), iMoovSeen(false), iMdatSeen(false), iStuck(false), iHeadWhole(false), iHeadRead(false), iBad(false)
{
    memset(&iResult, 0, sizeof(iResult));
}

static TUint64 Be(const TByte* p, TUint n)
{
    TUint64 v = 0;
    for (TUint k = 0; k < n; k++) v = (v << 8) | p[k];
    return v;
}

void Mpeg4AlacBatchDecoder::Push(const Brx& aFileBytes)
{
    iFile.insert(iFile.end(), aFileBytes.Ptr(), aFileBytes.Ptr() + aFileBytes.Bytes());
    if (iFile.size() >= 8 && !Mpeg4Recognise(Brn(iFile.data(), 8))) {
        iBad = true;
        THROW(CodecStreamCorrupt);
    }
    if (!iHeadWhole && !iBad) Peek();
}

void Mpeg4AlacBatchDecoder::Peek()
{
    // top-level headers only: the size, the fourcc, the 64-bit size where one is announced.  What is wrong with them is the device's
    // to say: a size no walk accepts, or "to the end of the stream", ends the peek where it stands.
    while (!iStuck && iFile.size() >= iPeekAt && iFile.size() - iPeekAt >= 8) {
        const TByte* h = iFile.data() + iPeekAt;
        TUint64 size = Be(h, 4), header = 8;
        if (size == 1) {
            if (iFile.size() - iPeekAt < 16) break;
            size = Be(h + 8, 8);
            header = 16;
        }
        iBoxes++;
        if (memcmp(h + 4, "mdat", 4) == 0) iMdatSeen = true;
        if (size < header || size > 0x7fffffffull || iPeekAt + size > 0x7fffffffull) {
            if (!iMoovSeen && memcmp(h + 4, "moov", 4) == 0) { iMoovSeen = true; iMoovEnd = iPeekAt + 8; }
            iStuck = true;
            break;
        }
        if (!iMoovSeen && memcmp(h + 4, "moov", 4) == 0) { iMoovSeen = true; iMoovEnd = iPeekAt + size; }
        iPeekAt += size;
        iExtent = iPeekAt;
    }
    // whole: `moov` has arrived, and so has the header of `mdat` -- in front of it, or behind it, where it tells how far the audio reaches
    iHeadWhole = iMoovSeen && (iMdatSeen || iStuck) && iFile.size() >= iMoovEnd;
}

TBool Mpeg4AlacBatchDecoder::TrySeek(TUint64 aFrame, TUint64& aFirstFrame)
{
    if (!iHeadRead || iBad) return false;
    uint64_t index = 0, first = 0;
    if (ohgpu_mp4_seek(iSamples.data(), iSamples.size(), aFrame, &index, &first) != OHGPU_OK) return false;
    iNext = index;
    iAlac.SeekToPacket(index);
    aFirstFrame = first;
    return true;
}

void Mpeg4AlacBatchDecoder::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    // 1. the heads that became whole this tick, in one call
    std::vector<ohgpu_mp4_stream_desc> descs;
    std::vector<size_t> laneOf;
    std::vector<TByte> src;
    TUint64 rows = 0;
    for (size_t k = 0; k < aCount; k++) {
        Mpeg4AlacBatchDecoder& d = *aLanes[k].decoder;
        if (!d.iHeadWhole || d.iHeadRead || d.iBad) continue;
        ohgpu_mp4_stream_desc s;
        memset(&s, 0, sizeof(s));
        const TUint64 bytes = std::max<TUint64>(d.iExtent, d.iFile.size());
        s.src_offset = src.size();
        s.src_bytes = (uint32_t)bytes;
        s.packet_first = (uint32_t)rows;
        s.packet_capacity = (uint32_t)(d.iMoovEnd / 4u + 16u);            // (a sample costs stsz four bytes; a uniform stsz of more is refused below)
        src.resize(src.size() + (size_t)bytes, 0);
        memcpy(src.data() + s.src_offset, d.iFile.data(), d.iFile.size());
        src.resize((src.size() + 15u) & ~(size_t)15u, 0);
        rows += s.packet_capacity;
        descs.push_back(s);
        laneOf.push_back(k);
    }
    int firstBad = 0;                                                     // 1: corrupt, 2: unsupported
    if (!descs.empty()) {
        std::vector<ohgpu_mp4_stream_result> results(descs.size());
        std::vector<ohgpu_alac_packet> packets((size_t)rows);
        std::vector<ohgpu_mp4_sample> samples((size_t)rows);
        const int err = ohgpu_mp4_process_host(aFactory.Gpu(), descs.data(), descs.size(), packets.size(), src.data(), src.size(), results.data(), packets.data(),
                                               samples.data());
        ASSERT(err == OHGPU_OK);
        for (size_t i = 0; i < descs.size(); i++) {
            Mpeg4AlacBatchDecoder& d = *aLanes[laneOf[i]].decoder;
            const ohgpu_mp4_stream_result& r = results[i];
            d.iResult = r;
            d.iHeadRead = true;
            int bad = 0;
            if (r.status == OHGPU_MP4_UNSUPPORTED || r.status == OHGPU_MP4_NOT_ALAC || (r.status == OHGPU_MP4_OK && r.samples > descs[i].packet_capacity)) bad = 2;
            else if (r.status != OHGPU_MP4_OK) bad = 1;
            if (!bad) {
                const ohgpu_alac_config& c = r.config;
                TByte cookie[24];
                const uint32_t words[3] = {c.max_frame_bytes, c.avg_bit_rate, c.sample_rate};
                for (int b = 0; b < 4; b++) cookie[b] = (TByte)(c.frame_length >> (24 - 8 * b));
                cookie[4] = c.compatible_version; cookie[5] = c.bit_depth; cookie[6] = c.pb; cookie[7] = c.mb; cookie[8] = c.kb; cookie[9] = c.channels;
                cookie[10] = (TByte)(c.max_run >> 8); cookie[11] = (TByte)c.max_run;
                for (int w = 0; w < 3; w++) for (int b = 0; b < 4; b++) cookie[12 + 4 * w + b] = (TByte)(words[w] >> (24 - 8 * b));
                try {
                    d.iAlac.SetConfig(Brn(cookie, sizeof(cookie)), r.timescale, r.duration);      // AlacApple.cpp:160-185
                } catch (CodecStreamFeatureUnsupported&) { bad = 2; } catch (CodecStreamCorrupt&) { bad = 1; }
            }
            if (bad) {
                d.iBad = true;
                if (!firstBad) firstBad = bad;
                continue;
            }
            const ohgpu_alac_packet* p = packets.data() + descs[i].packet_first;
            d.iPackets.assign(p, p + r.samples);
            for (ohgpu_alac_packet& q : d.iPackets) q.src_offset -= descs[i].src_offset;
            d.iSamples.assign(samples.data() + descs[i].packet_first, samples.data() + descs[i].packet_first + r.samples);
        }
    }
    // 2. the packets that have arrived whole, then one decode for all lanes
    std::vector<AlacBatchDecoder::Lane> lanes;
    for (size_t k = 0; k < aCount; k++) {
        Mpeg4AlacBatchDecoder& d = *aLanes[k].decoder;
        if (d.iHeadRead && !d.iBad) {
            while (d.iNext < d.iPackets.size()) {
                const ohgpu_alac_packet& p = d.iPackets[(size_t)d.iNext];
                if (p.src_offset + p.bytes > d.iFile.size()) break;
                d.iAlac.PushPacket(Brn(d.iFile.data() + p.src_offset, p.bytes));     // (a refused sample is a packet of no bytes: CORRUPT there)
                d.iNext++;
            }
        }
        AlacBatchDecoder::Lane l = {&d.iAlac, aLanes[k].controller, aLanes[k].trackOffset};
        lanes.push_back(l);
    }
    int decodeBad = 0;
    try {
        AlacBatchDecoder::Flush(aFactory, lanes.data(), lanes.size());
    } catch (CodecStreamFeatureUnsupported&) { decodeBad = 2; } catch (CodecStreamCorrupt&) { decodeBad = 1; }
    for (size_t k = 0; k < aCount; k++) {
        aLanes[k].trackOffset = lanes[k].trackOffset;
        if (aLanes[k].decoder->iAlac.Corrupt()) aLanes[k].decoder->iBad = true;
    }
    if (!firstBad) firstBad = decodeBad;
    if (firstBad == 2) THROW(CodecStreamFeatureUnsupported);
    if (firstBad == 1) THROW(CodecStreamCorrupt);
}

} // namespace Media
} // namespace OpenHome
