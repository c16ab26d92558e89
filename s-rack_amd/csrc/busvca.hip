// busvca.hip — the bus VCAs' unit (busvca.hip.h): an ADSR per gated bus on a workgroup's first wave, the VCAs streamed by all eight.
#include "launch.hpp"
#include "busvca.hip.h"

namespace srack {

void launch_bus_vca(const BusVcaArgs& a, hipStream_t st)
{
    if (!a.n_buses || !a.n) return;
    const dim3 grid((a.n_buses + kBusVcaTile - 1) / kBusVcaTile), block(kBusVcaWaves * 64);
    if (a.used == 2)
        hipLaunchKernelGGL((bus_vca<2>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((bus_vca<1>), grid, block, 0, st, a);
}

}  // namespace srack
