// ClockPuller.h -- the reference's pullable-clock interface (OpenHome/Media/ClockPuller.h:17-34), same name, same constant, same
// two calls, so that a receiver's clock controller (RaatOutput::SetRemoteTime, Av/Raat/Output.cpp:405-435) can drive this project's
// PullableSampleRateConverter as it drives an animator (AnimatorBasic.cpp:120-127, 257-270).
#pragma once

#include "OhTypes.h"

namespace OpenHome {
namespace Media {

class IPullableClock {
public:
    static const TUint kNominalFreq = 1u << 31;          // multiplier 1.0 in fix 1.31: no pull
public:
    virtual ~IPullableClock() {}
    /** Asks for the clock to run at aMultiplier times nominal (fix 1.31, so [0, 2)); kNominalFreq runs it at nominal. */
    virtual void PullClock(TUint aMultiplier) = 0;
    /** The largest departure from kNominalFreq this clock honours, in the same fix 1.31 units. */
    virtual TUint MaxPull() const = 0;
};

} // namespace Media
} // namespace OpenHome
