// busshape.hip — the bus shapers' unit (busshape.hip.h): a wave per stretch of a bus, the libm's tables in LDS once per workgroup.
#include "launch.hpp"
#include "busshape.hip.h"

namespace srack {

void launch_bus_shaper(const BusShaperArgs& a, hipStream_t st)
{
    if (!a.n_units) return;
    const dim3 grid((a.n_units + kBusShpWaves - 1) / kBusShpWaves), block(kBusShpWaves * 64);
    if (a.used == 2)
        hipLaunchKernelGGL((bus_shaper<2>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((bus_shaper<1>), grid, block, 0, st, a);
}

}  // namespace srack
