// FlacDecoder.h -- the codec side of FLAC: file bytes in, MsgAudioPcm out, the frames decoded on the device.
//
// Stands in for CodecFlac and the libFLAC under it (file:line relative to the reference tree):
//   CodecFlac::CallbackMetadata   OpenHome/Media/Codec/Flac.cpp:427-443   STREAMINFO -> OutputDecodedStream
//   CodecFlac::CallbackWrite      OpenHome/Media/Codec/Flac.cpp:355-419   a frame's planes -> big-endian pieces -> OutputAudioPcm
//   CodecFlac::CallbackError      OpenHome/Media/Codec/Flac.cpp:421-425   -> CodecStreamCorrupt
// Shape of this implementation (host/DsdPacker.h's): a decoder is a byte queue; nothing is decoded when bytes arrive.  The first
// bytes are the metadata, read on the host once all of it is there (ohgpu_flac_streaminfo).  Flush() takes every lane of a tick,
// lays the queued audio bytes of all of them into one arena and makes ONE device call (ohgpu_flac_process_host, packed big-endian
// output); the frames that call found leave through CodecController::OutputAudioPcm in CallbackWrite's pieces, and what a lane's
// last whole frame left over stays queued for the next tick.  Seeking, Ogg FLAC and the container layer are not here.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "DecodedAudioAggregator.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

class FlacBatchDecoder {
public:
    static const TUint kMaxPieceBytes = DecodedAudio::kMaxBytes;    // sizeof(CodecFlac::iBuf), Flac.cpp:51
    static const TUint kMaxSamplesPerTick = 1u << 20;                // a tick's output arena per lane is bounded by this many samples
public:
    FlacBatchDecoder();
    /** File bytes as they come, from "fLaC" on.  Throws CodecStreamCorrupt when they do not start a FLAC stream. */
    void Push(const Brx& aFileBytes);
    TBool StreamInfoKnown() const { return iInfoKnown; }
    const ohgpu_flac_streaminfo_t& StreamInfo() const { ASSERT(iInfoKnown); return iInfo; }
    /** Audio bytes queued (behind the metadata) that no Flush has consumed yet. */
    TUint PendingBytes() const { return iInfoKnown ? (TUint)iPending.size() : 0; }
    TUint64 SamplesDecoded() const { return iNextSample; }
    TBool Corrupt() const { return iCorrupt; }
    /** How CallbackWrite cuts a frame of aSamples (Flac.cpp:379-383): samples per piece, whole samples within kMaxPieceBytes. */
    static TUint PieceSamples(TUint aChannels, TUint aBitDepth) { return kMaxPieceBytes / ((aBitDepth / 8) * aChannels); }

    /** One stream of a tick: its decoder, where its messages go and the stream's position (advanced by what was output). */
    struct Lane {
        FlacBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** Decodes what every lane has queued in one device call and hands each lane's frames to its controller.  A lane whose bytes
     *  are no FLAC frames delivers what precedes the break; once every lane has been served the first such lane's
     *  CodecStreamCorrupt (a 12- or 20-bit frame: CodecStreamFeatureUnsupported) is thrown. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
private:
    void ReadMetadata();
private:
    std::vector<TByte> iPending;        // until the metadata is whole: the file from its start; then: unconsumed audio bytes
    ohgpu_flac_streaminfo_t iInfo;
    TBool iInfoKnown, iAnnounced, iCorrupt;
    TUint64 iNextSample;                // the first sample of the next frame
};

} // namespace Media
} // namespace OpenHome
