// DsdFileDecoder.h -- the codec side of DSD files: the bytes of a DSF or DFF file in, MsgAudioDsd out, the chunks read and the audio
// packed into the pipeline's DSD format on the device.
//
// Stands in for (file:line relative to the reference tree):
//   CodecDsdDsf::Recognise / CodecDsdDff::Recognise       OpenHome/Media/Codec/DsdDsf.cpp, DsdDff.cpp   the first four / sixteen bytes
//   CodecDsdDsf::StreamInitialise, ::Process              OpenHome/Media/Codec/DsdDsf.cpp               `DSD `, `fmt `, `data`, the plane pairs
//   CodecDsdDff::StreamInitialise, ::Process              OpenHome/Media/Codec/DsdDff.cpp               `FRM8`, `PROP`, `DSD `
//   CodecDsdDsf::TrySeek / CodecDsdDff::TrySeek                                                         a sample -> a block boundary
// Shape of this implementation: host/PcmFileDecoder.h's.  A decoder is a byte queue.  The walk over the bytes at hand runs on the host
// first (ohgpu_dsd_file_head: the core the device runs): a lane whose chunks have not all arrived waits, one that is no DSD file is
// dropped as not recognised, neither goes to the device.  Flush() then takes every other lane of a tick: ONE
// ohgpu_dsd_file_process_host over their bytes, from the chunk each lane stands at.  A lane's first OK result announces its stream;
// the sample blocks that came home leave through CodecController::OutputAudioDsd, as host/DsdPacker.h's do.  While the stream runs a
// lane's run is whole sample blocks; the 0x69 fill of a last partial block comes with the stream's last chunk alone.  The whole file
// at hand goes to the device at every tick (the walk wants the chunks where they lie): DESIGN.md 8.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "DecodedAudioAggregator.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

/** The rules of the two Recognise functions over the first bytes of a stream: four bytes decide DSF, sixteen DFF. */
TBool DsfRecognise(const Brx& aBytes);
TBool DffRecognise(const Brx& aBytes);

class DsdFileBatchDecoder {
public:
    /** (aSampleBlockWords, aPadBytesPerChunk): the pipeline's DSD format, validated as ohgpu_dsd_desc's. */
    DsdFileBatchDecoder(TUint aSampleBlockWords, TUint aPadBytesPerChunk);
    /** File bytes as they come, from the file's first byte on. */
    void Push(const Brx& aFileBytes);
    /** No more bytes will come: a TRUNCATED file is reported at the next tick. */
    void End() { iEnded = true; }
    TUint64 BytesPushed() const { return iFile.size(); }
    TBool Announced() const { return iAnnounced; }          // the stream's first OK result has been seen
    TBool Dropped() const { return iDropped; }              // a status other than OK was reported: the lane is served no more
    TBool Recognised() const { return !(iDropped && iResult.status == OHGPU_DSD_FILE_NOT_DSD); }
    TUint64 NextChunk() const { return iNextChunk; }
    const ohgpu_dsd_file_stream_result& Result() const { ASSERT(iAnnounced || iDropped); return iResult; }
    /** The walk over the bytes at hand, on the host: what the device will say of them for chunk 0 and unlimited room. */
    ohgpu_dsd_file_stream_result Head() const;

    struct Lane {
        DsdFileBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** One tick for all lanes.  A lane whose file is refused is dropped -- NOT_DSD: not recognised, nothing thrown; UNSUPPORTED:
     *  CodecStreamFeatureUnsupported; INVALID, or TRUNCATED once End() was called: CodecStreamCorrupt --; the first such lane's
     *  exception is thrown once every lane has been served. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
    /** The lane goes on at the block boundary at or in front of aSample (ohgpu_dsd_file_seek): its track offset becomes, for DSF, the
     *  rounded sample x Jiffies::PerSample(rate) and, for DFF, the rounded sample x Jiffies::kPerSecond / rate, and a new
     *  MsgDecodedStream says so.  False (nothing changes) before the stream has been announced or beyond the track's length. */
    static TBool TrySeek(Lane& aLane, TUint64 aSample);
private:
    void Announce(CodecController& aController, TUint64 aSampleStart);
private:
    std::vector<TByte> iFile;
    const TUint iSampleBlockWords, iPadBytesPerChunk, iChunksPerBlock;
    TUint64 iNextChunk;
    TBool iEnded, iAnnounced, iDropped;
    ohgpu_dsd_file_stream_result iResult;
};

} // namespace Media
} // namespace OpenHome
