// Mpeg4CencDecoder.cpp -- see Mpeg4CencDecoder.h.
#include "Mpeg4CencDecoder.h"

#include <algorithm>
#include <cstring>

namespace OpenHome {
namespace Media {

static const uint32_t kFlacCode = 0x664c6143u, kAlacCode = 0x616c6163u;    // 'fLaC', 'alac'

static Mpeg4CencKind KindOfHead(const ohgpu_cenc_stream_result& aHead)
{
    switch (aHead.mp4f.status) {
    case OHGPU_MP4F_OK: return aHead.mp4f.codec == kFlacCode ? Mpeg4CencKind::Flac : aHead.mp4f.codec == kAlacCode ? Mpeg4CencKind::Alac : Mpeg4CencKind::Other;
    case OHGPU_MP4F_NOT_MP4: return Mpeg4CencKind::None;
    case OHGPU_MP4F_TRUNCATED: return Mpeg4CencKind::NeedMore;
    case OHGPU_MP4F_NOT_FRAGMENTED: return Mpeg4CencKind::Plain;
    default: return Mpeg4CencKind::Other;
    }
}

Mpeg4CencKind Mpeg4CencRecognise(const Brx& aBytes, TBool aAllSchemes)
{
    if (aBytes.Bytes() >= 8 && memcmp(aBytes.Ptr() + 4, "ftyp", 4) != 0) return Mpeg4CencKind::None;
    if (aAllSchemes) {
        ohgpu_cbcs_stream_result wide;
        if (ohgpu_cbcs_head(aBytes.Ptr(), aBytes.Bytes(), &wide) != OHGPU_OK) return Mpeg4CencKind::None;
        return KindOfHead(wide.cenc);
    }
    ohgpu_cenc_stream_result head;
    if (ohgpu_cenc_head(aBytes.Ptr(), aBytes.Bytes(), &head) != OHGPU_OK) return Mpeg4CencKind::None;
    return KindOfHead(head);
}

Mpeg4CencBatchDecoder::Mpeg4CencBatchDecoder(ICencKeyProvider& aKeys, TBool aAllSchemes)
    : iKeys(aKeys), iAllSchemes(aAllSchemes), iHaveKey(false), iPeekAt(0), iWhole(0), iMoovEnd(0), iServed(0), iNextRow(0), iNextSample(0), iStuck(false), iHeadRead(false), iBad(false), iAnnounced(false), iConfigured(false),
      iKind(Mpeg4CencKind::NeedMore)
{
    memset(&iHead, 0, sizeof(iHead));
    memset(&iWideHead, 0, sizeof(iWideHead));
    memset(iKey, 0, sizeof(iKey));
}

static TUint64 Be(const TByte* p, TUint n)
{
    TUint64 v = 0;
    for (TUint k = 0; k < n; k++) v = (v << 8) | p[k];
    return v;
}

void Mpeg4CencBatchDecoder::Push(const Brx& aBytes)
{
    iFile.insert(iFile.end(), aBytes.Ptr(), aBytes.Ptr() + aBytes.Bytes());
    if (iFile.size() >= 8 && memcmp(iFile.data() + 4, "ftyp", 4) != 0) {
        iBad = true;
        THROW(CodecStreamCorrupt);
    }
    if (!iBad) Peek();
}

void Mpeg4CencBatchDecoder::Peek()
{
    // top-level headers only.  A size no walk accepts, or "to the end of the stream", ends the peek where it stands: what is wrong with
    // it is the device's to say, once the bytes up to it have been served.
    while (!iStuck && iFile.size() - iPeekAt >= 8) {
        const TByte* h = iFile.data() + iPeekAt;
        TUint64 size = Be(h, 4), header = 8;
        if (size == 1) {
            if (iFile.size() - iPeekAt < 16) break;
            size = Be(h + 8, 8);
            header = 16;
        }
        if (size < header || size > 0x7fffffffull || iPeekAt + size > 0x7fffffffull) {
            iStuck = true;
            iWhole = iFile.size();
            break;
        }
        if (iFile.size() - iPeekAt < size) break;                         // (this box has not arrived whole)
        if (!iMoovEnd && memcmp(h + 4, "moov", 4) == 0) iMoovEnd = iPeekAt + size;
        iPeekAt += size;
        iWhole = iPeekAt;
    }
    if (iStuck) iWhole = iFile.size();
    if (!iHeadRead && (iMoovEnd || iStuck)) {
        const int err = iAllSchemes ? ohgpu_cbcs_head(iFile.data(), (size_t)iWhole, &iWideHead) : ohgpu_cenc_head(iFile.data(), (size_t)iWhole, &iHead);
        ASSERT(err == OHGPU_OK);
        if (iAllSchemes) iHead = iWideHead.cenc;
        iHeadRead = true;
        iKind = KindOfHead(iHead);
        if (iHead.mp4f.status == OHGPU_MP4F_OK && iHead.is_protected) {   // the key is asked for once, by the kid the head gives
            Bwx key(iKey, sizeof(iKey));
            iHaveKey = iKeys.Key(Brn(iHead.kid, sizeof(iHead.kid)), key) && key.Bytes() == sizeof(iKey);
            if (!iHaveKey) memset(iKey, 0, sizeof(iKey));
        }
    }
}

TBool Mpeg4CencBatchDecoder::TrySeek(TUint64 aFrame, TUint64& aFirstFrame)
{
    if (iBad || iSamples.empty()) return false;
    uint64_t index = 0, first = 0;
    if (ohgpu_mp4_seek(iSamples.data(), iSamples.size(), aFrame, &index, &first) != OHGPU_OK) return false;
    iNextRow = index;
    iNextSample = first;
    iServed = 0;                                                          // (the next Flush serves the lane whatever has arrived since)
    if (iKind == Mpeg4CencKind::Alac) iAlac.SeekToPacket(index);
    aFirstFrame = first;
    return true;
}

// 0: served; 1: corrupt; 2: unsupported
int Mpeg4CencBatchDecoder::Judge(const ohgpu_cenc_stream_result& aResult, TUint aCapacity)
{
    const ohgpu_mp4f_stream_result& r = aResult.mp4f;
    if (r.status == OHGPU_CENC_NO_KEY) return 2;
    if (r.status == OHGPU_MP4F_UNSUPPORTED || r.status == OHGPU_MP4F_NOT_CODEC || r.status == OHGPU_MP4F_NOT_FRAGMENTED) return 2;
    if (r.status != OHGPU_MP4F_OK) return 1;
    return r.samples > aCapacity ? 2 : 0;
}

void Mpeg4CencBatchDecoder::Describe(ohgpu_cenc_stream_desc& s, TUint64 aSrcOffset, TUint64 aRow, TUint64 aRun) const
{
    memset(&s, 0, sizeof(s));
    s.src_offset = aSrcOffset;
    s.src_bytes = (uint32_t)iWhole;
    s.codecs = OHGPU_MP4F_CODEC_ALAC | OHGPU_MP4F_CODEC_FLAC;
    s.packet_first = (uint32_t)aRow;
    s.packet_capacity = (uint32_t)std::min<TUint64>(iWhole / 4u + 64u, 1u << 22);       // (an entry with a size costs its trun four bytes)
    s.run_first = (uint32_t)aRun;
    s.run_capacity = (uint32_t)(iWhole / 16u + 4u);                                      // (a trun is 16 bytes at the least)
    s.gather_first_row = (uint32_t)iNextRow;
    s.flags = OHGPU_MP4F_GATHER;
    if (iHeadRead) memcpy(s.kid, iHead.kid, sizeof(s.kid));
    if (iHaveKey) { s.key_flags = OHGPU_CENC_HAVE_KEY; memcpy(s.key, iKey, sizeof(s.key)); }
}

void Mpeg4CencBatchDecoder::Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount)
{
    int firstBad = 0;                                                     // 1: corrupt, 2: unsupported
    auto refuse = [&](Mpeg4CencBatchDecoder& d, int bad) { d.iBad = true; if (!firstBad) firstBad = bad; };
    // the second family's descriptors and results around the first's (ohgpu_cbcs_stream_desc begins with ohgpu_cenc_stream_desc, the result
    // with the result): a lane's share of the subsample table is sized from its bytes, of which an entry costs six
    auto widen = [](const std::vector<ohgpu_cenc_stream_desc>& aDescs, size_t* aSubsamples) {
        std::vector<ohgpu_cbcs_stream_desc> wide(aDescs.size());
        size_t rows = 0;
        for (size_t i = 0; i < aDescs.size(); i++) {
            memset(&wide[i], 0, sizeof(wide[i]));
            memcpy(&wide[i], &aDescs[i], sizeof(aDescs[i]));
            wide[i].subsample_first = (uint32_t)rows;
            wide[i].subsample_capacity = aDescs[i].src_bytes / 6u;
            rows += wide[i].subsample_capacity;
        }
        *aSubsamples = rows;
        return wide;
    };
    for (int family = 0; family < 2; family++) {                         // 0: ohgpu_cenc_*; 1: ohgpu_cbcs_* (the lanes made with aAllSchemes)
        std::vector<size_t> flacLanes, alacLanes;
        for (size_t k = 0; k < aCount; k++) {
            Mpeg4CencBatchDecoder& d = *aLanes[k].decoder;
            if (!d.iHeadRead || d.iBad || (d.iAllSchemes ? 1 : 0) != family) continue;
            if (d.iKind != Mpeg4CencKind::Flac && d.iKind != Mpeg4CencKind::Alac) {
                const int bad = d.Judge(d.iHead, ~0u);
                refuse(d, bad ? bad : 2);
                continue;
            }
            if (d.iWhole <= d.iServed) continue;                             // nothing whole has arrived since the lane was served
            (d.iKind == Mpeg4CencKind::Flac ? flacLanes : alacLanes).push_back(k);
        }

        // ---- fLaC: demultiplex, gather and decode in one call
        if (!flacLanes.empty()) {
            const size_t n = flacLanes.size();
            std::vector<ohgpu_cenc_stream_desc> descs(n);
            std::vector<ohgpu_flac_stream_desc> flac(n);
            TUint64 srcTotal = 0, midTotal = 0, dstTotal = 0, rows = 0, runs = 0, framesMax = 0;
            for (size_t i = 0; i < n; i++) {
                const Mpeg4CencBatchDecoder& d = *aLanes[flacLanes[i]].decoder;
                const ohgpu_flac_streaminfo_t& info = d.iHead.mp4f.flac;
                d.Describe(descs[i], srcTotal, rows, runs);
                descs[i].dst_offset = midTotal;
                descs[i].dst_capacity = descs[i].src_bytes;
                const TUint64 frames = d.iWhole / std::max<TUint64>(info.min_framesize, 7u + info.channels) + 1;
                TUint64 samples = std::min<TUint64>(frames * std::max<TUint64>(info.max_blocksize, 16u), FlacBatchDecoder::kMaxSamplesPerTick);
                if (info.total_samples != 0) samples = std::min<TUint64>(samples, info.total_samples - std::min<TUint64>(info.total_samples, d.iNextSample));
                ohgpu_flac_stream_desc& s = flac[i];
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
                srcTotal += MsgFactory::ArenaShare(descs[i].src_bytes);
                midTotal += MsgFactory::ArenaShare(descs[i].src_bytes);
                dstTotal += MsgFactory::ArenaShare((TUint64)s.max_samples * info.channels * (info.bits / 8));
                rows += descs[i].packet_capacity;
                runs += descs[i].run_capacity;
                framesMax += descs[i].packet_capacity;
            }
            TByte* src = nullptr;
            TByte* dst = nullptr;
            aFactory.ReserveArena((size_t)srcTotal, (size_t)dstTotal, src, dst);
            for (size_t i = 0; i < n; i++) memcpy(src + descs[i].src_offset, aLanes[flacLanes[i]].decoder->iFile.data(), descs[i].src_bytes);
            std::vector<ohgpu_cenc_stream_result> demuxed(n);
            std::vector<ohgpu_alac_packet> packets((size_t)rows);
            std::vector<ohgpu_mp4_sample> samples((size_t)rows);
            std::vector<ohgpu_flac_stream_result> results(n);
            std::vector<ohgpu_flac_frame> frames((size_t)framesMax);
            size_t nFrames = 0;
            int err;
            if (family == 0) {
                err = ohgpu_cenc_flac_process_host(aFactory.Gpu(), descs.data(), flac.data(), n, packets.size(), (size_t)runs, src, srcTotal, midTotal, dst, dstTotal,
                                                   demuxed.data(), nullptr, packets.data(), samples.data(), results.data(), frames.data(), frames.size(), &nFrames);
            } else {
                size_t subsamples = 0;
                const std::vector<ohgpu_cbcs_stream_desc> wide = widen(descs, &subsamples);
                std::vector<ohgpu_cbcs_stream_result> wideResults(n);
                err = ohgpu_cbcs_flac_process_host(aFactory.Gpu(), wide.data(), flac.data(), n, packets.size(), (size_t)runs, subsamples, src, srcTotal, midTotal, dst, dstTotal,
                                                   wideResults.data(), nullptr, packets.data(), samples.data(), results.data(), frames.data(), frames.size(), &nFrames);
                for (size_t i = 0; i < n; i++) demuxed[i] = wideResults[i].cenc;
            }
            ASSERT(err == OHGPU_OK && nFrames <= frames.size());
            static const TByte kName[] = {'F', 'L', 'A', 'C'};
            size_t at = 0;
            for (size_t i = 0; i < n; i++) {
                Lane& lane = aLanes[flacLanes[i]];
                Mpeg4CencBatchDecoder& d = *lane.decoder;
                const ohgpu_flac_streaminfo_t& info = d.iHead.mp4f.flac;
                const TUint sampleBytes = (info.bits / 8u) * info.channels;
                int bad = d.Judge(demuxed[i], descs[i].packet_capacity);
                if (!bad && !d.iAnnounced) {
                    // Flac.cpp:427-441: bit rate = rate x depth x channels, lossless
                    lane.controller->OutputDecodedStream(info.sample_rate * info.bits * info.channels, info.bits, info.sample_rate, info.channels, Brn(kName, sizeof(kName)),
                                                         info.total_samples * Jiffies::kPerSecond / info.sample_rate, 0, true);
                    d.iAnnounced = true;
                }
                for (; at < nFrames && frames[at].stream == i; at++) {
                    // Flac.cpp:379-417: a frame leaves in pieces of whole samples within kMaxPieceBytes, the count restarting with every frame
                    const TByte* audio = dst + flac[i].dst_offset + (frames[at].first_sample - flac[i].first_sample) * sampleBytes;
                    const TUint perPiece = FlacBatchDecoder::PieceSamples(info.channels, info.bits);
                    for (TUint done = 0; done < frames[at].blocksize; ) {
                        const TUint m = std::min(perPiece, frames[at].blocksize - done);
                        lane.trackOffset += lane.controller->OutputAudioPcm(Brn(audio + (size_t)done * sampleBytes, m * sampleBytes), info.channels, info.sample_rate, info.bits,
                                                                            AudioDataEndian::Big, lane.trackOffset);
                        done += m;
                    }
                }
                if (bad) { refuse(d, bad); continue; }
                if (results[i].status == OHGPU_FLAC_CORRUPT) bad = 1;
                if (results[i].status == OHGPU_FLAC_UNSUPPORTED) bad = 2;
                // the rows whose bytes the FLAC phases consumed: a frame is a sample, so bytes_consumed ends a row
                const ohgpu_alac_packet* mine = packets.data() + descs[i].packet_first;
                TUint64 row = d.iNextRow, bytes = 0;
                while (row < demuxed[i].mp4f.samples_available && bytes < results[i].bytes_consumed) bytes += mine[row++].bytes;
                if (!bad && bytes != results[i].bytes_consumed) bad = 1;     // (these are no FLAC frames in samples)
                const ohgpu_mp4_sample* rowsOf = samples.data() + descs[i].packet_first;
                d.iSamples.assign(rowsOf, rowsOf + std::min<TUint64>(demuxed[i].mp4f.samples, descs[i].packet_capacity));
                d.iNextRow = row;
                d.iNextSample += results[i].samples;
                if (row == demuxed[i].mp4f.samples_available) d.iServed = descs[i].src_bytes;      // (else this tick's arena was full: the next one goes on)
                if (bad) refuse(d, bad);
            }
        }

        // ---- alac: demultiplex, then the packets that are new to the lane's packet decoder
        if (!alacLanes.empty()) {
            const size_t n = alacLanes.size();
            std::vector<ohgpu_cenc_stream_desc> descs(n);
            std::vector<TByte> src;
            TUint64 rows = 0, runs = 0, dstTotal = 0;
            for (size_t i = 0; i < n; i++) {
                const Mpeg4CencBatchDecoder& d = *aLanes[alacLanes[i]].decoder;
                d.Describe(descs[i], src.size(), rows, runs);
                descs[i].dst_offset = dstTotal;                                   // the clear packets come home here
                descs[i].dst_capacity = descs[i].src_bytes;
                dstTotal += (descs[i].src_bytes + 15u) & ~15u;
                src.insert(src.end(), d.iFile.begin(), d.iFile.begin() + (size_t)d.iWhole);
                src.resize((src.size() + 15u) & ~(size_t)15u, 0);
                rows += descs[i].packet_capacity;
                runs += descs[i].run_capacity;
            }
            std::vector<ohgpu_cenc_stream_result> demuxed(n);
            std::vector<ohgpu_alac_packet> packets((size_t)rows);
            std::vector<ohgpu_mp4_sample> samples((size_t)rows);
            std::vector<TByte> clear((size_t)dstTotal);
            int err;
            if (family == 0) {
                err = ohgpu_cenc_process_host(aFactory.Gpu(), descs.data(), n, packets.size(), (size_t)runs, src.data(), src.size(), clear.data(), clear.size(), demuxed.data(),
                                              nullptr, packets.data(), samples.data());
            } else {
                size_t subsamples = 0;
                const std::vector<ohgpu_cbcs_stream_desc> wide = widen(descs, &subsamples);
                std::vector<ohgpu_cbcs_stream_result> wideResults(n);
                err = ohgpu_cbcs_process_host(aFactory.Gpu(), wide.data(), n, packets.size(), (size_t)runs, subsamples, src.data(), src.size(), clear.data(), clear.size(),
                                              wideResults.data(), nullptr, packets.data(), samples.data());
                for (size_t i = 0; i < n; i++) demuxed[i] = wideResults[i].cenc;
            }
            ASSERT(err == OHGPU_OK);
            for (size_t i = 0; i < n; i++) {
                Mpeg4CencBatchDecoder& d = *aLanes[alacLanes[i]].decoder;
                const ohgpu_mp4f_stream_result& r = demuxed[i].mp4f;
                int bad = d.Judge(demuxed[i], descs[i].packet_capacity);
                if (!bad && !d.iConfigured) {
                    const ohgpu_alac_config& c = r.config;
                    TByte cookie[24];
                    const uint32_t words[3] = {c.max_frame_bytes, c.avg_bit_rate, c.sample_rate};
                    for (int b = 0; b < 4; b++) cookie[b] = (TByte)(c.frame_length >> (24 - 8 * b));
                    cookie[4] = c.compatible_version; cookie[5] = c.bit_depth; cookie[6] = c.pb; cookie[7] = c.mb; cookie[8] = c.kb; cookie[9] = c.channels;
                    cookie[10] = (TByte)(c.max_run >> 8); cookie[11] = (TByte)c.max_run;
                    for (int w = 0; w < 3; w++) for (int b = 0; b < 4; b++) cookie[12 + 4 * w + b] = (TByte)(words[w] >> (24 - 8 * b));
                    try {
                        d.iAlac.SetConfig(Brn(cookie, sizeof(cookie)), r.timescale, r.duration);      // AlacApple.cpp:160-185
                        d.iConfigured = true;
                    } catch (CodecStreamFeatureUnsupported&) { bad = 2; } catch (CodecStreamCorrupt&) { bad = 1; }
                }
                if (bad) { refuse(d, bad); continue; }
                const ohgpu_alac_packet* mine = packets.data() + descs[i].packet_first;
                // (rows [iNextRow, samples_available) were gathered: each row names its clear bytes in the destination buffer; a tick whose
                // gather found no room or nothing new leaves the rows empty and the lane where it stands)
                for (; r.bytes_gathered && d.iNextRow < r.samples_available; d.iNextRow++) {
                    const ohgpu_alac_packet& p = mine[(size_t)d.iNextRow];
                    d.iAlac.PushPacket(Brn(clear.data() + p.src_offset, p.bytes));
                }
                const ohgpu_mp4_sample* rowsOf = samples.data() + descs[i].packet_first;
                d.iSamples.assign(rowsOf, rowsOf + std::min<TUint64>(r.samples, descs[i].packet_capacity));
                d.iServed = descs[i].src_bytes;
            }
        }
    }
    // one decode for every alac lane, whether it was served this tick or not
    std::vector<AlacBatchDecoder::Lane> lanes;
    std::vector<size_t> laneOf;
    for (size_t k = 0; k < aCount; k++) {
        Mpeg4CencBatchDecoder& d = *aLanes[k].decoder;
        if (d.iKind != Mpeg4CencKind::Alac || !d.iConfigured) continue;
        AlacBatchDecoder::Lane l = {&d.iAlac, aLanes[k].controller, aLanes[k].trackOffset};
        lanes.push_back(l);
        laneOf.push_back(k);
    }
    int decodeBad = 0;
    if (!lanes.empty()) {
        try {
            AlacBatchDecoder::Flush(aFactory, lanes.data(), lanes.size());
        } catch (CodecStreamFeatureUnsupported&) { decodeBad = 2; } catch (CodecStreamCorrupt&) { decodeBad = 1; }
        for (size_t i = 0; i < lanes.size(); i++) {
            aLanes[laneOf[i]].trackOffset = lanes[i].trackOffset;
            if (aLanes[laneOf[i]].decoder->iAlac.Corrupt()) aLanes[laneOf[i]].decoder->iBad = true;
        }
    }
    if (!firstBad) firstBad = decodeBad;
    if (firstBad == 2) THROW(CodecStreamFeatureUnsupported);
    if (firstBad == 1) THROW(CodecStreamCorrupt);
}

} // namespace Media
} // namespace OpenHome
