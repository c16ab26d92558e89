// busfx.hip — the bus reverbs' unit (busfx.hip.h): a stereo Freeverb per mix bus, a workgroup per bus, time-parallel within a block.
#include "launch.hpp"
#include "busfx.hip.h"

namespace srack {

void launch_bus_reverb(const BusFxArgs& a, uint32_t n_buses, hipStream_t st)
{
    hipLaunchKernelGGL(bus_reverb, dim3(n_buses), dim3(kBusFxThreads), 0, st, a);
}

}  // namespace srack
