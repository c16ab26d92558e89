// jit.hpp — voice kernels specialised for one flattened program at run time: the generator (jit_gen.hpp), the compiler and the kernel
// cache (jit_cache.hpp), and the loaded kernel (jit.cpp).  The one header render.hip and capi.cpp include.
#pragma once
#include <cstdint>
#include <memory>
#include <string>

#include "jit_cache.hpp"
#include "jit_gen.hpp"
#include "kernel_args.hip.h"

namespace srack {

struct JitKernel {  // a loaded module: shared between the process-wide cache and every patch that renders with it
    void* module = nullptr;    // hipModule_t
    void* function = nullptr;  // hipFunction_t
    JitKernel() = default;
    JitKernel(const JitKernel&) = delete;
    JitKernel& operator=(const JitKernel&) = delete;
    ~JitKernel();              // hipModuleUnload, once the last owner lets go
};

struct JitFetchInfo {  // how one kernel was come by
    int how = 0;              // 0: this process had it (memory), 1: the disk cache, 2: compiled now
    double compile_ms = 0.0;  // hiprtc time when how == 2
    int waves = 0;            // the register budget the kernel was compiled under (waves per SIMD; 0: none asked for)
    int vgprs = 0;            // its VGPRs
    bool bank_lds = false;    // a banked sample player's waves are staged in LDS (part of the source: jit_gen.cpp, gen_sample)
};

// Generate + compile for the current device's architecture (gfx950 when the process has no device); nothing is loaded.
int jit_compile_only(const FlatPair& pair, int out_mode, bool with_ctl);
// Generate, fetch the code object (memory -> disk -> hiprtc; jit_cache.cpp "the kernel cache") and load it on the current device.
// want_waves: how many waves per SIMD the render has for this kernel (voices / 64 / 1024 SIMDs, at most 4).  A kernel whose registers
// allow fewer is compiled again under the budget for that many (then for half as many) and the tighter kernel is taken IF it does not
// spill (`how->waves`: the budget taken, 0: the compiler's own choice): more waves hide a recurrence's latency, scratch traffic does not.
int jit_get(const FlatPair& pair, int out_mode, bool with_ctl, std::shared_ptr<const JitKernel>* out, JitFetchInfo* how = nullptr, int want_waves = 1);
int jit_launch(const JitKernel& k, const KernelArgs& ka, uint32_t n_blocks, void* stream);

}  // namespace srack
