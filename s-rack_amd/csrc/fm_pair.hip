// fm_pair.hip — the unit of the FM pairs that render one sample at a time (fm_pair.hip.h); their exact instantiations: fm_exact.hip.h.
#include "fm_exact.hip.h"
#include "fm_pair.hip.h"
#include "launch.hpp"

namespace srack {

void launch_fm_pair(Kernel kernel, bool exact, int out_mode, const KernelArgs& ka, const ChainRoles& roles, dim3 grid, hipStream_t st)
{
    if (kernel == Kernel::FmPairSplit) {
        hipLaunchKernelGGL((render_fm_pair_split<true, 0>), grid, dim3(128), 0, st, ka, roles);
        return;
    }
    auto launch = [&](auto E, auto O) {
        if (kernel == Kernel::FmPairRing)
            hipLaunchKernelGGL((render_fm_pair_ring<E, O>), grid, dim3(64), 0, st, ka, roles);
        else
            hipLaunchKernelGGL((render_fm_pair<E, O>), grid, dim3(64), 0, st, ka, roles);
    };
    if (exact)  // one instantiation, output mode decided at run time
        launch(std::true_type{}, std::integral_constant<int, 0>{});
    else
        with_out_mode(out_mode, [&](auto O) { launch(std::false_type{}, O); });
}

void launch_fm_pair_x(int out_mode, const KernelArgs& ka, const ChainRoles& roles, dim3 grid, hipStream_t st)
{
    with_out_mode(out_mode, [&](auto O) { hipLaunchKernelGGL((render_fm_pair_x<O>), grid, dim3(128), 0, st, ka, roles); });
}

}  // namespace srack
