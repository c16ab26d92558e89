// seq.hip — render_voice_chain_seq's unit (seq.hip.h).
#include "launch.hpp"
#include "seq.hip.h"

namespace srack {

void launch_seq(uint32_t osc_port, int out_mode, const KernelArgs& ka, const SeqRoles& r, dim3 grid, hipStream_t st)
{
    with_osc_port(osc_port, [&](auto A) {
        // (no instantiation for the mix alone: that request takes the one that decides at run time)
        with_out_mode(out_mode == 2 ? 0 : out_mode, [&](auto O) {
            if constexpr (O != 2) hipLaunchKernelGGL((render_voice_chain_seq<decltype(A)::value, O>), grid, dim3(64), 0, st, ka, r);
        });
    });
}

}  // namespace srack
