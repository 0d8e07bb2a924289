// DsdPacker.h -- the codec side of DSD: file bytes in, messages in the pipeline's DSD format out.
//
// Stands in for what the reference's three DSD codecs do per byte on the codec thread before they call
// ICodecController::OutputAudioDsd (file:line relative to the reference tree):
//   CodecDsdDsf::Process / TransferToOutputBuffer   OpenHome/Media/Codec/DsdDsf.cpp:169-247   (plane pairs, bits reversed)
//   CodecDsdDff::TransferToOutputBuffer             OpenHome/Media/Codec/DsdDff.cpp:305-369   (L R L R)
//   CodecDsdRaw + DsdFiller                         OpenHome/Media/Codec/DsdRaw.cpp:119-134, DsdFiller.cpp:52-99   (L L R R)
// Shape of this implementation: a packer is a byte queue with a rule for how much of it is convertible; nothing is converted when
// bytes arrive.  Flush() takes every lane of a tick, lays the convertible bytes of all of them into one arena and makes ONE device
// call (ohgpu_dsd_process_host); each lane's run then leaves through CodecController::OutputAudioDsd as messages of at most
// DecodedAudio::kMaxBytes.  What a packer keeps back: less than a plane pair (DSF), less than a sample block's worth of input
// (DFF, Raw) -- until Drain(), after which the rest goes out, a DSF / DFF tail completed with 0x69 by the device and a Raw tail
// completed on the host, where only the audio positions are filled (DsdFiller.cpp:52-65).
#pragma once

#include <vector>

#include "DecodedAudioAggregator.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

class DsdPacker {
public:
    enum class EKind { Dsf, Dff, Raw };
    static const TUint kDsfPlaneBytes = 4096;
    static const TUint kDsfPairChunks = 2048;            // a pair of planes holds this many chunks' worth
public:
    DsdPacker(EKind aKind, TUint aSampleBlockWords, TUint aPadBytesPerChunk);
    /** File bytes as they come (DSF: the sample data, from the first plane pair on). */
    void Push(const Brx& aFileBytes);
    /** DSF only: the stream's length in chunks (the header's sample count / 16): chunks of the last pair beyond it are padding. */
    void SetStreamChunks(TUint64 aChunks);
    /** End of stream: the next Flush converts everything that is left. */
    void Drain();
    /** Chunks the next Flush would convert. */
    TUint ConvertibleChunks() const;
    TUint ChunksPerBlock() const { return iChunksPerBlock; }
    TUint SampleBlockWords() const { return iSampleBlockWords; }
    TUint PadBytesPerChunk() const { return iPadBytesPerChunk; }

    /** One stream of a tick: its packer, where its messages go and the stream's position (advanced by what was output). */
    struct Lane {
        DsdPacker* packer;
        CodecController* controller;
        TUint channels, sampleRate;
        TUint64 trackOffset;
    };
    /** Converts what every lane has pending in one device call and hands each lane's run to its controller. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
private:
    TUint SourceBytes(TUint aChunks) const;              // of iPending, consumed by a conversion of aChunks
private:
    const EKind iKind;
    const TUint iSampleBlockWords, iPadBytesPerChunk, iChunksPerBlock;
    std::vector<TByte> iPending;
    TUint64 iStreamChunks = UINT64_MAX, iChunksOut = 0;
    TBool iDraining = false;
};

} // namespace Media
} // namespace OpenHome
