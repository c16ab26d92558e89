// master.hip — the master section's unit (master.hip.h): run sums, the tree over them, the statistics of the result.
#include "launch.hpp"
#include "master.hip.h"

namespace srack {

void launch_master(const MasterArgs& a, hipStream_t st)
{
    const uint32_t n_runs = (a.n_buses + kMasterRun - 1) / kMasterRun;
    const uint32_t n_blocks = (n_runs + kMasterBlock - 1) / kMasterBlock;
    // four samples per lane where every row is 16-byte aligned: the rows' base, and a row length that keeps the alignment from row to row
    // (the scratch is the library's own allocation)
    const bool vec = a.n % 4 == 0 && ((uintptr_t)a.rows & 15u) == 0;
    if (vec) {
        const uint32_t per = kMasterThreads * 4;
        hipLaunchKernelGGL((master_runs<4, 8>), dim3((uint32_t)(((uint64_t)a.n + per - 1) / per), n_runs, a.used), dim3(kMasterThreads), 0, st, a);
    } else {
        hipLaunchKernelGGL((master_runs<1, 16>), dim3((uint32_t)(((uint64_t)a.n + kMasterThreads - 1) / kMasterThreads), n_runs, a.used), dim3(kMasterThreads), 0, st, a);
    }
    hipLaunchKernelGGL(master_tree, dim3((uint32_t)(((uint64_t)a.n + 63) / 64), 2), dim3(64 * n_blocks), 0, st, a);
    if (a.stats) hipLaunchKernelGGL(master_stats, dim3(1), dim3(128 * a.used), 0, st, a);
}

}  // namespace srack
