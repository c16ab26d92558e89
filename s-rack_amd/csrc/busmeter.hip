// busmeter.hip — the bus meters' unit (busmeter.hip.h): a lane per (bus, channel) row, a wave per workgroup, two sets of statistics in registers.
#include "launch.hpp"
#include "busmeter.hip.h"

namespace srack {

template <int kUsed>
static void launch_bus_meter_used(const BusMeterArgs& a, dim3 grid, hipStream_t st)
{
    if (a.levels && a.totals)
        hipLaunchKernelGGL((bus_meter<kUsed, true, true>), grid, dim3(64), 0, st, a);
    else if (a.levels)
        hipLaunchKernelGGL((bus_meter<kUsed, true, false>), grid, dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((bus_meter<kUsed, false, true>), grid, dim3(64), 0, st, a);
}

void launch_bus_meter(const BusMeterArgs& a, hipStream_t st)
{
    if (!a.n || !a.n_buses || (!a.levels && !a.totals)) return;
    const dim3 grid((a.n_buses * a.used + 63u) / 64u);
    if (a.used == 2)
        launch_bus_meter_used<2>(a, grid, st);
    else
        launch_bus_meter_used<1>(a, grid, st);
}

}  // namespace srack
