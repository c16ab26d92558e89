// busvcf.hip — the bus filters' unit (busvcf.hip.h): a ladder per row, a wave per workgroup; the copy of the disabled buses' rows.
#include "launch.hpp"
#include "busvcf.hip.h"

namespace srack {

void launch_bus_filter(const BusVcfArgs& a, hipStream_t st)
{
    if (a.n_rows) {
        const dim3 grid((a.n_rows + 63) / 64);
        if (a.cv && a.used == 2)
            hipLaunchKernelGGL((bus_filter<true, 2>), grid, dim3(64), 0, st, a);
        else if (a.cv)
            hipLaunchKernelGGL((bus_filter<true, 1>), grid, dim3(64), 0, st, a);
        else if (a.used == 2)
            hipLaunchKernelGGL((bus_filter<false, 2>), grid, dim3(64), 0, st, a);
        else
            hipLaunchKernelGGL((bus_filter<false, 1>), grid, dim3(64), 0, st, a);
    }
    if (a.n_copy && a.out != a.rows)
        hipLaunchKernelGGL(bus_filter_copy, dim3((uint32_t)(((uint64_t)a.n + kBusVcfCopyThreads - 1) / kBusVcfCopyThreads), a.n_copy < 65535u ? a.n_copy : 65535u),
                           dim3(kBusVcfCopyThreads), 0, st, a);
}

}  // namespace srack
