// sends.hip — the bus sends' unit (sends.hip.h): run sums per destination, the tree over the runs of a destination that has several.
#include "launch.hpp"
#include "sends.hip.h"

namespace srack {

void launch_sends(const SendArgs& a, hipStream_t st)
{
    // four samples per lane where every row is 16-byte aligned, read and written: both bases, and a row length that keeps the
    // alignment from row to row (the scratch is the library's own allocation)
    const bool vec = a.n % 4 == 0 && (((uintptr_t)a.rows | (uintptr_t)a.out) & 15u) == 0;
    const uint32_t gy = a.n_runs < kSendGridY ? a.n_runs : kSendGridY;
    const uint32_t gz = a.used * ((a.n_runs + kSendGridY - 1) / kSendGridY);
    if (vec) {
        const uint32_t per = kSendThreads * 4;
        hipLaunchKernelGGL((send_runs<4, 8>), dim3((uint32_t)(((uint64_t)a.n + per - 1) / per), gy, gz), dim3(kSendThreads), 0, st, a);
    } else {
        hipLaunchKernelGGL((send_runs<1, 16>), dim3((uint32_t)(((uint64_t)a.n + kSendThreads - 1) / kSendThreads), gy, gz), dim3(kSendThreads), 0, st, a);
    }
    if (a.n_multi) hipLaunchKernelGGL(send_tree, dim3((uint32_t)(((uint64_t)a.n + 63) / 64), a.n_multi, a.used), dim3(64 * a.max_blocks), 0, st, a);
}

}  // namespace srack
