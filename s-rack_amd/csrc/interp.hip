// interp.hip — the tile interpreter's unit: its out-of-line tile_* functions sit beside all four kernels that call them — and beside
// the FM pairs' exact instantiations (fm_exact.hip.h), the other callers of the out-of-line exact oscillator.
#include <cstdio>

#define SRK_FM_EXACT_HERE  // (this unit instantiates them)
#include "flatten.hpp"
#include "fm_exact.hip.h"
#include "interp.hip.h"
#include "launch.hpp"

namespace srack {

void launch_interp(const FlatProgram& P, const KernelArgs& ka, hipStream_t st, bool debug_occ)
{
    const size_t lds = interp_lds_bytes(P.hdr);
    if (debug_occ) {  // tools/: what the runtime says about resident workgroups per CU for this LDS size
        int n = -1;
        hipError_t e = (P.render_flags & SRACK_RENDER_EXACT_OSC) ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_interp<true>, 64, lds)
                                                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, render_interp<false>, 64, lds);
        fprintf(stderr, "[srack] render_interp lds=%zu B/wave occupancy=%d workgroups/CU (%s) waves=%u\n", lds, n, hipGetErrorString(e), ka.n_waves);
    }
    if (P.render_flags & SRACK_RENDER_EXACT_OSC)
        hipLaunchKernelGGL(render_interp<true>, dim3(ka.n_waves), dim3(64), lds, st, ka);
    else
        hipLaunchKernelGGL(render_interp<false>, dim3(ka.n_waves), dim3(64), lds, st, ka);
}

void launch_interp_stages(bool exact, uint32_t n_stages, size_t lds, const KernelArgs* slots, hipStream_t st)
{
    if (exact)
        hipLaunchKernelGGL(render_interp_stages<true>, dim3(n_stages), dim3(64), lds, st, slots);
    else
        hipLaunchKernelGGL(render_interp_stages<false>, dim3(n_stages), dim3(64), lds, st, slots);
}

}  // namespace srack
