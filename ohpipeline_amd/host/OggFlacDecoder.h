// OggFlacDecoder.h -- the codec side of Ogg FLAC: file bytes in, MsgAudioPcm out, pages and frames both handled on the device
// (DESIGN.md 5.15 in front of 5.10).
//
// Stands in for what CodecFlac does with the second kind of stream it recognises (file:line relative to the reference tree):
//   CodecFlac::Recognise          OpenHome/Media/Codec/Flac.cpp:155-178   "fLaC" at 0, or "OggS" at 0 and "fLaC" at 37 of 42 bytes
//   CodecFlac::StreamInitialise   OpenHome/Media/Codec/Flac.cpp:201-213   libFLAC initialised for Ogg: its Ogg layer and the page library
//   CodecFlac::Process            OpenHome/Media/Codec/Flac.cpp:249-251   any Ogg-level error -> CodecStreamCorrupt
// Shape of this implementation: host/FlacDecoder.h's.  A decoder is a byte queue.  The first bytes are the head -- the pages that hold
// the mapping header and the metadata -- read on the host once all of it is there (ohgpu_ogg_flac_head), which also says on which
// page, at which segment and with which page number the audio begins.  Flush() takes every lane of a tick and makes ONE device call
// (ohgpu_ogg_flac_process_host: demux into a device-only arena, decode from there, packed big-endian output); the frames leave through
// CodecController::OutputAudioPcm in CallbackWrite's pieces.  The queue keeps the bytes from the page on which the first undelivered
// packet began, with that page's number and the packet's segment, for the next tick.  FlacBatchDecoder is unchanged beside it.
#pragma once

#include <vector>

#include "../../include/ohgpu.h"
#include "DecodedAudioAggregator.h"
#include "FlacDecoder.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

enum class FlacStreamKind { None, Native, Ogg };
/** CodecFlac::Recognise's rule over the first bytes of a stream (it reads 42). */
FlacStreamKind FlacRecognise(const Brx& aBytes);

class OggFlacBatchDecoder {
public:
    OggFlacBatchDecoder();
    /** File bytes as they come, from "OggS" on.  Throws CodecStreamCorrupt when they do not start an Ogg FLAC stream. */
    void Push(const Brx& aFileBytes);
    TBool StreamInfoKnown() const { return iInfoKnown; }
    const ohgpu_flac_streaminfo_t& StreamInfo() const { ASSERT(iInfoKnown); return iInfo; }
    /** Bytes queued from the resume page on that no Flush has consumed yet. */
    TUint PendingBytes() const { return iInfoKnown ? (TUint)iPending.size() : 0; }
    TUint64 SamplesDecoded() const { return iNextSample; }
    TBool Corrupt() const { return iCorrupt; }
    TUint Serial() const { return iSerial; }
    TUint NextPageNumber() const { return iNextSeq; }
    TUint ResumeSegment() const { return iResumeSegment; }

    struct Lane {
        OggFlacBatchDecoder* decoder;
        CodecController* controller;
        TUint64 trackOffset;
    };
    /** Demuxes and decodes what every lane has queued in one device call and hands each lane's frames to its controller.  A lane that
     *  stops on either layer (lost sync, a hole, a foreign mapping header; bytes that are no FLAC frames) delivers what precedes the
     *  break; once every lane has been served the first such lane's CodecStreamCorrupt (a 12- or 20-bit frame:
     *  CodecStreamFeatureUnsupported) is thrown. */
    static void Flush(MsgFactory& aFactory, Lane* aLanes, size_t aCount);
private:
    void ReadHead();
private:
    std::vector<TByte> iPending;        // until the head is whole: the file from its start; then: the bytes from the resume page on
    ohgpu_flac_streaminfo_t iInfo;
    TBool iInfoKnown, iAnnounced, iCorrupt;
    TUint64 iNextSample;                // the first sample of the next frame
    TUint iSerial, iNextSeq, iResumeSegment;
};

} // namespace Media
} // namespace OpenHome
