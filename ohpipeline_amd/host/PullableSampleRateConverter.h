// PullableSampleRateConverter.h -- the stand-in for a pulled DAC clock when one device serves many streams against one output
// clock.  The reference keeps a stream in step with its source by pulling the DAC (IPullableClock, ClockPuller.h:17-34:
// RaatOutput::SetRemoteTime works out the multiplier, Av/Raat/Output.cpp:405-435; AnimatorBasic pulls more or fewer jiffies a tick,
// AnimatorBasic.cpp:120-127, 257-270).  Here there is no DAC per stream: this element IS the stream's pullable clock.  It converts
// every PCM stream (48 -> 48 kHz included: that is the common drift case) with the pulled resampler and, like
// SampleRateConverter, never touches a PCM byte -- it hands downstream MsgAudioPcm messages whose audio is virtual ("outputs from
// input position pos, step apart"), which downstream elements split and ramp as usual and the driver's PlayableBatch reads in one
// device call per filter.  A multiplier above nominal consumes input faster, as in AnimatorBasic.
#pragma once

#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "ClockPuller.h"
#include "Msg.h"

namespace OpenHome {
namespace Media {

/** Moves an input position (frame, fraction of 2^-32) on by aCount outputs of aStep (Q32.32): the split identity of DESIGN.md 4b. */
inline void PullAdvance(TUint64& aFrame, TUint& aFrac, TUint64 aStep, TUint64 aCount)
{
    const TUint64 u = (TUint64)aFrac + aCount * aStep;
    aFrame += u >> 32;
    aFrac = (TUint)(u & 0xffffffffu);
}

/** Input history of one pulled stream (shared by the output messages that refer to it) and the stream's filter: a ring of aHistoryMs
 *  of input, never less than a filter length and two maximal messages, as SampleRateConverterStream keeps for the fixed ratio.  A
 *  reader copies the window of input a message reads (ohgpu_src_pull_window); Append runs on the element's puller thread, the copy
 *  on the driver's: both take iLock. */
class PullableSampleRateConverterStream {
public:
    PullableSampleRateConverterStream(const PullFilter& aFilter, TUint aRateIn, TUint aChannels, TUint aBitDepth, AudioDataEndian aEndian,
                                      TUint aHistoryMs = 2000);
    void Append(const TByte* aData, TUint aBytes);
    TUint64 InputFrames() const;
    /** Copies input frames [aFirst, aFirst + aFrames) to aDst; ASSERTs that the ring still holds them. */
    void CopyFrames(TUint64 aFirst, TUint aFrames, TByte* aDst) const;
    const PullFilter& Filter() const { return iFilter; }
    TUint FrameBytes() const { return iFrameBytes; }
    TUint SourceBitDepth() const { return iBitDepth; }
    AudioDataEndian SourceEndian() const { return iEndian; }
private:
    const PullFilter& iFilter;
    const TUint iBitDepth, iFrameBytes;
    const AudioDataEndian iEndian;
    mutable std::mutex iLock;
    std::vector<TByte> iRing;                            // frame f lives at (f % iCapacity) * iFrameBytes
    TUint64 iCapacity;                                   // frames
    TUint64 iFrames;                                     // appended so far: the ring holds [max(0, iFrames - iCapacity), iFrames)
};

class PullableSampleRateConverter : public PipelineElement, public IPipelineElementUpstream, public IPullableClock {
    static const TUint kSupportedMsgTypes;
public:
    static const TUint kPhasesLog2 = 8;
    /** As SampleRateConverter, plus aMaxPull: the largest pull the filter is designed for (1e-3 = 1000 ppm; crystals drift by a few
     *  hundred ppm at most).  Every PCM stream the pipeline accepts is converted, each with the design StreamDesign picks for its
     *  rate: aTapsPerPhase = 0 (the default) lets it choose 32 or 64 taps per phase, aPassHz is the widest pass band it may use. */
    PullableSampleRateConverter(MsgFactory& aFactory, IPipelineElementUpstream& aUpstreamElement, TUint aOutputRate,
                                TUint aTapsPerPhase = 0, double aBeta = 8.0, double aPassHz = 20000.0, double aMaxPull = 0.001);
    /** The design a stream of aRateIn gets ("Per stream"): the pass edge is at most aPassHz and at most
     *  aPassHz * min(rate_in, rate_out) / 44100 (the band 20 kHz is of 44.1 kHz, kept below the narrower Nyquist), and narrowed
     *  further where the band between the pass and stop edges, at both extreme pulls, is narrower than the T taps hold -80 dB
     *  across at beta = 8 (0.1655 cycles per input frame for T = 32, 0.09 for T = 64).  With aTapsPerPhase = 0, T = 32 where it
     *  keeps the whole pass band, T = 64 otherwise.  Measured from 8 to 384 kHz into 44.1 and 48 kHz: -80.6 dB or better. */
    static void StreamDesign(TUint aRateIn, TUint aRateOut, TUint aTapsPerPhase, double aPassHz, double aMaxPull, TUint& aTaps,
                             double& aPassEdgeHz);
public: // from IPipelineElementUpstream
    Msg* Pull() override;
public: // from IPullableClock: any thread; takes effect at the next message this element emits; clamped to +-MaxPull()
    void PullClock(TUint aMultiplier) override;
    TUint MaxPull() const override { return iMaxPull; }
public:
    /** The multiplier in force (after clamping). */
    TUint Multiplier() const { return iMultiplier.load(); }
private: // IMsgProcessor
    Msg* ProcessMsg(MsgDecodedStream* aMsg) override;
    Msg* ProcessMsg(MsgAudioPcm* aMsg) override;
    Msg* ProcessMsg(MsgSilence* aMsg) override;
    Msg* ProcessMsg(MsgHalt* aMsg) override;
private:
    MsgFactory& iFactory;
    IPipelineElementUpstream& iUpstreamElement;
    const TUint iOutputRate, iTapsPerPhase;
    const double iBeta, iPassHz, iMaxPullRatio;
    const TUint iMaxPull;
    std::atomic<TUint> iMultiplier;
    DecodedStreamInfo iInfo;
    std::shared_ptr<PullableSampleRateConverterStream> iStream;
    TUint64 iPosFrame;                                    // the next output's input position
    TUint iPosFrac;
    TUint64 iTrackOffset;                                 // jiffies, at the output rate
};

} // namespace Media
} // namespace OpenHome
