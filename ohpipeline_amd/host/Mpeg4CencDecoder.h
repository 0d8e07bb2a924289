// Mpeg4CencDecoder.h -- the codec side of PROTECTED fragmented MPEG-4 (DASH / CMAF segments under Common Encryption, scheme `cenc`) with a
// fLaC or an alac track: stream bytes in, MsgAudioPcm out, the fragments read and decrypted on the device in front of
// the FLAC phases (5.10) or host/AlacDecoder.h's packet decoder (5.12).  A clear fragmented stream is served the same way.
//
// Stands where the reference's container decrypts a sample at a time (file:line relative to the reference tree):
//   Mpeg4BoxSchm / Tenc / Senc         OpenHome/Media/Codec/Mpeg4.cpp:2243-2550     the protection boxes
//   Mpeg4BoxMdat::Process              OpenHome/Media/Codec/Mpeg4.cpp:3327-3440     IMpegDRMProvider::Decrypt(KID, data, IV, out) a sample
//   IMpegDRMProvider                   OpenHome/Media/Codec/Mpeg4.h:1084-1092       here ICencKeyProvider: it gives the key, the device decrypts
// Shape of this implementation: host/Mpeg4FragmentDecoder.h's, whose text on the byte queue, the peek and the ticks holds here.  What
// differs: the head is ohgpu_cenc_head's (no key needed); once it is read and says the track is protected, the provider is asked for the
// key ONCE, by the head's kid -- a provider that has none leaves the lane to answer OHGPU_CENC_NO_KEY at its first Flush --; Flush()
// makes ONE ohgpu_cenc_flac_process_host for the fLaC lanes of a tick and ONE ohgpu_cenc_process_host for the alac lanes, whose clear
// packets come home in the destination buffer and go to the lane's AlacBatchDecoder, then ONE AlacBatchDecoder::Flush.  NO_KEY and
// UNSUPPORTED throw CodecStreamFeatureUnsupported, other bad statuses CodecStreamCorrupt, once every lane has been served.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "AlacDecoder.h"
#include "FlacDecoder.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

/** Where IMpegDRMProvider stands: the key that belongs to a key identifier (16 bytes each).  False: there is none. */
class ICencKeyProvider {
public:
    virtual TBool Key(const Brx& aKid, Bwx& aKey16) = 0;
    virtual ~ICencKeyProvider() {}
};

enum class Mpeg4CencKind { None, NeedMore, Flac, Alac, Plain, Other };
/** What the first bytes of a stream are: None (no "ftyp" at bytes 4..8), NeedMore (`moov` has not arrived whole), Flac / Alac (a
 *  fragmented stream with such a track: this element's), Plain (a file with sample tables: host/Mpeg4AlacDecoder.h's), Other (an MPEG-4
 *  stream this element refuses). */
Mpeg4CencKind Mpeg4CencRecognise(const Brx& aBytes, TBool aAllSchemes = false);

class Mpeg4CencBatchDecoder {
public:
    explicit Mpeg4CencBatchDecoder(ICencKeyProvider& aKeys, TBool aAllSchemes = false);
    /** Stream bytes as they come, from the first byte on.  Throws CodecStreamCorrupt at the eighth byte when they are no MPEG-4 stream. */
    void Push(const Brx& aBytes);
    TBool HeadRead() const { return iHeadRead; }            // `moov` has arrived whole and was read (on the host)
    Mpeg4CencKind Kind() const { return iKind; }        // NeedMore until then
    const ohgpu_cenc_stream_result& Head() const { ASSERT(iHeadRead); return iHead; }
    TUint64 BytesPushed() const { return iFile.size(); }
    TUint64 WholeExtent() const { return iWhole; }          // how far the top-level boxes that have arrived whole reach
    TUint64 NextRow() const { return iNextRow; }            // the first sample that was not delivered yet
    TUint64 RowsKnown() const { return iSamples.size(); }   // the samples of the fragments read so far
    TBool Corrupt() const { return iBad; }
    TBool Protected() const { return iHeadRead && iHead.is_protected != 0; }
    TBool HaveKey() const { return iHaveKey; }                // the provider gave the key the head's kid names
    TBool AllSchemes() const { return iAllSchemes; }          // served by ohgpu_cbcs_*
    const ohgpu_cbcs_stream_result& WideHead() const { ASSERT(iHeadRead && iAllSchemes); return iWideHead; }
    AlacBatchDecoder& Alac() { return iAlac; }
    /** The sample that holds audio frame aFrame becomes the next one delivered; aFirstFrame is that sample's first frame.  False
     *  (nothing changes) before a Flush has read a fragment or when the frame lies behind the fragments read so far. */
    TBool TrySeek(TUint64 aFrame, TUint64& aFirstFrame);

    struct Lane {
        Mpeg4CencBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** One tick for all lanes.  A lane whose stream is refused (NO_KEY, UNSUPPORTED, NOT_CODEC, NOT_FRAGMENTED: CodecStreamFeatureUnsupported;
     *  any other status but OK: CodecStreamCorrupt) or whose samples do not decode delivers what precedes; the first such lane's
     *  exception is thrown once every lane has been served. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
private:
    void Peek();
    int Judge(const ohgpu_cenc_stream_result& aResult, TUint aCapacity);
    void Describe(ohgpu_cenc_stream_desc& aDesc, TUint64 aSrcOffset, TUint64 aRow, TUint64 aRun) const;
private:
    ICencKeyProvider& iKeys;
    TBool iAllSchemes;
    ohgpu_cbcs_stream_result iWideHead;
    TBool iHaveKey;
    TByte iKey[16];
    std::vector<TByte> iFile;
    TUint64 iPeekAt, iWhole, iMoovEnd, iServed, iNextRow, iNextSample;
    TBool iStuck, iHeadRead, iBad, iAnnounced, iConfigured;
    Mpeg4CencKind iKind;
    ohgpu_cenc_stream_result iHead;
    std::vector<ohgpu_mp4_sample> iSamples;
    AlacBatchDecoder iAlac;
};

} // namespace Media
} // namespace OpenHome
