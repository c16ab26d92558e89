// fm_block.hip — the unit of the time-parallel FM pairs (fm_block.hip.h); render_fm_pair_block_x's instantiations: fm_exact.hip.h.
#include "fm_block.hip.h"
#include "fm_exact.hip.h"
#include "launch.hpp"

namespace srack {

// The FM pair with a delay of 256 ... 1024 samples in default mode: time-parallel, 32 voices per 512-thread workgroup, ring in LDS.
template <class K>
static hipError_t launch_blk(K kernel, size_t lds, const KernelArgs& ka, const ChainRoles& roles, hipStream_t st)
{
    // more than 64 KB of dynamic LDS has to be asked for — per device (the attribute belongs to the current device's copy of the
    // function) and from any thread: asked for before every launch, which costs nothing next to one
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(ka.n_waves), dim3(kBlkVoices * kBlkSlices), lds, st, ka, roles);
    return hipSuccess;
}

hipError_t launch_fm_block(bool x, int out_mode, const KernelArgs& ka, const ChainRoles& roles, hipStream_t st)
{
    const size_t B = (size_t)ka.prog.buffer_size;
    return with_out_mode(out_mode, [&](auto O) {
        if (x) return launch_blk(render_fm_pair_block_x<O>, fm_block_x_lds_bytes((uint32_t)B), ka, roles, st);
        return launch_blk(render_fm_pair_block<O>, sizeof(float) * B * kBlkVoices + sizeof(double) * 2 * kBlkSlices * kBlkVoices + 16, ka, roles, st);
    });
}

}  // namespace srack
