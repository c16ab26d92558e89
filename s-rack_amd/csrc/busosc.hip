// busosc.hip — the bus oscillators' unit (busosc.hip.h): an oscillator and two Math operations per enabled bus, a wave per workgroup; the
// zeroing of the disabled buses' rows.
#include "launch.hpp"
#include "busosc.hip.h"

namespace srack {

void launch_bus_osc(const BusOscArgs& a, hipStream_t st)
{
    if (!a.n) return;
    if (a.n_on) {
        const dim3 grid((a.n_on + 63) / 64);
        if (a.cv && a.sync)
            hipLaunchKernelGGL((bus_osc<true, true>), grid, dim3(64), 0, st, a);
        else if (a.cv)
            hipLaunchKernelGGL((bus_osc<true, false>), grid, dim3(64), 0, st, a);
        else if (a.sync)
            hipLaunchKernelGGL((bus_osc<false, true>), grid, dim3(64), 0, st, a);
        else
            hipLaunchKernelGGL((bus_osc<false, false>), grid, dim3(64), 0, st, a);
    }
    if (a.n_off)
        hipLaunchKernelGGL(bus_osc_zero, dim3((uint32_t)(((uint64_t)a.n + kBusOscZeroThreads - 1) / kBusOscZeroThreads), a.n_off < 65535u ? a.n_off : 65535u),
                           dim3(kBusOscZeroThreads), 0, st, a);
}

}  // namespace srack
