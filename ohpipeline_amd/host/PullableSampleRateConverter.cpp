// PullableSampleRateConverter.cpp -- see PullableSampleRateConverter.h.
#include "PullableSampleRateConverter.h"

#include <algorithm>
#include <cstring>

#include "../../include/ohgpu.h"

namespace OpenHome {
namespace Media {

// ---------------------------------------------------------------- PullableSampleRateConverterStream
PullableSampleRateConverterStream::PullableSampleRateConverterStream(const PullFilter& aFilter, TUint aRateIn, TUint aChannels,
                                                                     TUint aBitDepth, AudioDataEndian aEndian, TUint aHistoryMs)
    : iFilter(aFilter)
    , iBitDepth(aBitDepth), iFrameBytes(aChannels * (aBitDepth / 8))
    , iEndian(aEndian)
    , iCapacity(0), iFrames(0)
{
    iCapacity = (TUint64)aRateIn * aHistoryMs / 1000;
    const TUint64 least = (TUint64)iFilter.T + 2 * (DecodedAudio::kMaxBytes / iFrameBytes + 1);
    if (iCapacity < least) iCapacity = least;
    iRing.resize((size_t)(iCapacity * iFrameBytes));
}

void PullableSampleRateConverterStream::Append(const TByte* aData, TUint aBytes)
{
    ASSERT(aBytes % iFrameBytes == 0);
    const TUint64 frames = aBytes / iFrameBytes;
    ASSERT(frames <= iCapacity);
    std::lock_guard<std::mutex> hold(iLock);
    const TUint64 at = iFrames % iCapacity;
    const TUint64 head = std::min(frames, iCapacity - at);            // up to the ring's end, the rest from its start
    memcpy(&iRing[(size_t)(at * iFrameBytes)], aData, (size_t)(head * iFrameBytes));
    if (frames > head) memcpy(&iRing[0], aData + head * iFrameBytes, (size_t)((frames - head) * iFrameBytes));
    iFrames += frames;
}

TUint64 PullableSampleRateConverterStream::InputFrames() const
{
    std::lock_guard<std::mutex> hold(iLock);
    return iFrames;
}

void PullableSampleRateConverterStream::CopyFrames(TUint64 aFirst, TUint aFrames, TByte* aDst) const
{
    std::lock_guard<std::mutex> hold(iLock);
    ASSERT(aFirst + aFrames <= iFrames);                               // the output exists only once its input has arrived
    ASSERT(aFirst + iCapacity >= iFrames);                             // ... and the ring must not have gone round over it
    const TUint64 at = aFirst % iCapacity;
    const TUint64 head = std::min<TUint64>(aFrames, iCapacity - at);
    memcpy(aDst, &iRing[(size_t)(at * iFrameBytes)], (size_t)(head * iFrameBytes));
    if (aFrames > head) memcpy(aDst + head * iFrameBytes, &iRing[0], (size_t)((aFrames - head) * iFrameBytes));
}

// ---------------------------------------------------------------- PullableSampleRateConverter
const TUint PullableSampleRateConverter::kSupportedMsgTypes =
    eMode | eTrack | eDrain | eDelay | eEncodedStream | eMetatext | eStreamInterrupted | eHalt | eFlush | eWait |
    eDecodedStream | eAudioPcm | eSilence | eQuit;

PullableSampleRateConverter::PullableSampleRateConverter(MsgFactory& aFactory, IPipelineElementUpstream& aUpstreamElement,
                                                         TUint aOutputRate, TUint aTapsPerPhase, double aBeta, double aPassHz,
                                                         double aMaxPull)
    : PipelineElement(kSupportedMsgTypes)
    , iFactory(aFactory)
    , iUpstreamElement(aUpstreamElement)
    , iOutputRate(aOutputRate), iTapsPerPhase(aTapsPerPhase)
    , iBeta(aBeta), iPassHz(aPassHz), iMaxPullRatio(aMaxPull)
    , iMaxPull((TUint)(aMaxPull * (double)kNominalFreq + 0.5))
    , iMultiplier(kNominalFreq)
    , iPosFrame(0), iPosFrac(0)
    , iTrackOffset(0)
{
    (void)Jiffies::PerSample(aOutputRate);       // throws SampleRateInvalid for a rate the pipeline cannot express
    ASSERT(aMaxPull >= 0.0 && aMaxPull < 0.5);
}

void PullableSampleRateConverter::StreamDesign(TUint aRateIn, TUint aRateOut, TUint aTapsPerPhase, double aPassHz, double aMaxPull,
                                               TUint& aTaps, double& aPassEdgeHz)
{
    // the widest pass edge f (Hz) whose band up to the stop edge, f_stop = rate_out - f (rate_in - f from 2x upsampling on),
    // spans `transition` cycles per input frame at both extreme pulls: (A - f) / (r (1 + p)) - f / (r (1 - p)) = transition
    const double r = (double)aRateIn, a = (aRateOut >= 2 * aRateIn) ? r : (double)aRateOut;
    auto widest = [&](double aTransition) { return (a / (1.0 + aMaxPull) - aTransition * r) / (1.0 / (1.0 + aMaxPull) + 1.0 / (1.0 - aMaxPull)); };
    const double cap = std::min(aPassHz, aPassHz * (double)std::min(aRateIn, aRateOut) / 44100.0);
    aTaps = aTapsPerPhase != 0 ? aTapsPerPhase : (widest(0.1655) >= cap ? 32u : 64u);
    aPassEdgeHz = std::min(cap, widest(aTaps == 32 ? 0.1655 : 0.09));
}

void PullableSampleRateConverter::PullClock(TUint aMultiplier)
{
    const TUint lo = kNominalFreq - iMaxPull, hi = kNominalFreq + iMaxPull;
    iMultiplier.store(aMultiplier < lo ? lo : (aMultiplier > hi ? hi : aMultiplier));
}

Msg* PullableSampleRateConverter::Pull()
{
    Msg* msg;
    do {                                          // input that does not complete an output frame yields nothing yet
        msg = iUpstreamElement.Pull();
        msg = msg->Process(*this);
    } while (msg == nullptr);
    return msg;
}

Msg* PullableSampleRateConverter::ProcessMsg(MsgDecodedStream* aMsg)
{
    iInfo = aMsg->StreamInfo();
    iStream.reset();
    iPosFrame = 0;
    iPosFrac = 0;
    iTrackOffset = 0;
    if (iInfo.Format() != AudioFormat::Pcm || iInfo.SampleRate() == 0) {
        return aMsg;                              // nothing to convert
    }
    DecodedStreamInfo out = iInfo;
    out.iSampleRate = iOutputRate;
    out.iBitDepth = 24;                           // the converter works, and delivers, in the S24 domain
    out.iBitRate = iOutputRate * 24 * iInfo.NumChannels();
    aMsg->RemoveRef();
    return iFactory.CreateMsgDecodedStream(out);
}

Msg* PullableSampleRateConverter::ProcessMsg(MsgAudioPcm* aMsg)
{
    if (iInfo.SampleRate() == 0 || iInfo.Format() != AudioFormat::Pcm) {
        return aMsg;
    }
    ASSERT(aMsg->iAudioData != nullptr);                              // input must be real audio
    ASSERT(!aMsg->Ramp().IsEnabled());                                // ramps are set downstream of the converter
    const TUint jps = Jiffies::PerSample(aMsg->SampleRate());
    const TUint frameBytes = aMsg->NumChannels() * (aMsg->BitDepth() / 8);
    if (iStream == nullptr) {
        TUint taps = 0;
        double passHz = 0.0;
        StreamDesign(aMsg->SampleRate(), iOutputRate, iTapsPerPhase, iPassHz, iMaxPullRatio, taps, passHz);
        const PullFilter& f = iFactory.SharedPullFilter(aMsg->SampleRate(), iOutputRate, taps, kPhasesLog2, iBeta, passHz, iMaxPullRatio);
        iStream = std::make_shared<PullableSampleRateConverterStream>(f, aMsg->SampleRate(), aMsg->NumChannels(), aMsg->BitDepth(),
                                                                      aMsg->iAudioData->Endian());
    }
    const TUint firstFrame = aMsg->iOffset / jps;
    const TUint frames = aMsg->iSize / jps;
    iStream->Append(aMsg->iAudioData->Ptr(firstFrame * frameBytes), frames * frameBytes);
    const TUint rateIn = aMsg->SampleRate();
    aMsg->RemoveRef();
    // the step the clock asks for now, for every output of this message
    uint64_t step = 0;
    const int err = ohgpu_src_pull_step(rateIn, iOutputRate, iMultiplier.load(), &step);
    ASSERT(err == OHGPU_OK);
    // how many outputs the input that has arrived makes: output k exists once its newest input frame pos + k * step has arrived
    const TUint64 have = iStream->InputFrames();
    if (have <= iPosFrame) {
        return nullptr;
    }
    const TUint64 room = ((have - 1 - iPosFrame) << 32) + (0xffffffffull - iPosFrac);
    const TUint64 n = room / step + 1;
    ASSERT(n < (1u << 20));                                           // (one input message makes at most a few thousand)
    const TUint jpsOut = Jiffies::PerSample(iOutputRate);
    MsgAudioPcm* out = new MsgAudioPcm(iFactory, nullptr, iOutputRate, 24, iInfo.NumChannels(), iTrackOffset);
    out->iPulled = iStream;
    out->iPullPosFrame = iPosFrame;
    out->iPullPosFrac = iPosFrac;
    out->iPullStep = step;
    out->iSize = (TUint)n * jpsOut;
    PullAdvance(iPosFrame, iPosFrac, step, n);
    iTrackOffset += n * jpsOut;
    return out;
}

Msg* PullableSampleRateConverter::ProcessMsg(MsgSilence* aMsg)
{
    if (iInfo.SampleRate() == 0 || iInfo.Format() != AudioFormat::Pcm) {
        return aMsg;
    }
    TUint jiffies = aMsg->Jiffies();
    aMsg->RemoveRef();
    return iFactory.CreateMsgSilence(jiffies, iOutputRate, 24, iInfo.NumChannels());
}

Msg* PullableSampleRateConverter::ProcessMsg(MsgHalt* aMsg)
{
    return aMsg;
}

} // namespace Media
} // namespace OpenHome
