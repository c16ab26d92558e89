// jit.cpp — the loaded kernel of the general path's fast half: a generated source (jit_gen.cpp) is fetched as a code object
// (jit_cache.cpp), loaded as a module on the current device and launched.  The only part of the three that needs a device.
#include "jit.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace srack {

int jit_compile_only(const FlatPair& pair, int out_mode, bool with_ctl)
{
    std::string src;
    int rc = jit_source(pair, out_mode, with_ctl, src);
    if (rc != SRACK_OK) return rc;
    const Fetched f = fetch_code(device_arch(), src);
    if (f.rc != SRACK_OK) set_error(f.err);
    return f.rc;
}

JitKernel::~JitKernel()
{
    if (module) (void)hipModuleUnload((hipModule_t)module);
}

// A code object's kernel descriptor metadata (the AMDGPU msgpack note): the unsigned integer stored under `key`, or -1
static long metadata_uint(const std::vector<char>& code, const char* key)
{
    const size_t n = std::strlen(key);
    for (size_t i = 0; i + n + 1 < code.size(); i++) {
        if (std::memcmp(&code[i], key, n) != 0) continue;
        const unsigned char* p = (const unsigned char*)&code[i + n];
        const size_t left = code.size() - (i + n);
        if (*p <= 0x7f) return (long)*p;
        if (*p == 0xcc && left >= 2) return (long)p[1];
        if (*p == 0xcd && left >= 3) return (long)((p[1] << 8) | p[2]);
        if (*p == 0xce && left >= 5) return (long)(((unsigned long)p[1] << 24) | (p[2] << 16) | (p[3] << 8) | p[4]);
    }
    return -1;
}

int jit_get(const FlatPair& pair, int out_mode, bool with_ctl, std::shared_ptr<const JitKernel>* out, JitFetchInfo* how, int want_waves)
{
    out->reset();
    std::string src;
    int rc = jit_source(pair, out_mode, with_ctl, src, 0, want_waves);
    if (rc != SRACK_OK) return rc;
    // The register budget (see jit.hpp).  The compiler's own choice first: most kernels fit; one that does not is compiled under the
    // budget for want_waves, then for half as many, and the first of those that needs no scratch memory replaces it.
    int budget = 0, vgprs = 0;
    // OFF unless SRACK_JIT_BUDGET=1: on the survey's sixty random patches at 262 144 voices (tools/survey_ab.sh) no kernel that exceeds its
    // budget compiles under it without scratch — what they hold in registers is the exact flavour's f64 arithmetic of several oscillators, not
    // slack — so the rule only cost two more compilations per such kernel (median 127.8 against 128.1 ms per second of audio, with and without).
    if (want_waves > 1 && !getenv("SRACK_JIT_WAVES") && getenv("SRACK_JIT_BUDGET") && getenv("SRACK_JIT_BUDGET")[0] == '1') {
        const Fetched f0 = fetch_code(device_arch(), src);
        if (f0.rc != SRACK_OK) {
            set_error(f0.err);
            return f0.rc;
        }
        vgprs = (int)metadata_uint(f0.code->code, ".vgpr_count");
        for (int w = std::min(want_waves, 4); w >= 2 && vgprs > 0 && vgprs > 512 / w; w /= 2) {
            std::string tight;
            if (jit_source(pair, out_mode, with_ctl, tight, w, want_waves) != SRACK_OK) break;
            const Fetched fw = fetch_code(device_arch(), tight);
            if (fw.rc != SRACK_OK) break;
            if (metadata_uint(fw.code->code, ".private_segment_fixed_size") == 0) {
                src = tight;
                budget = w;
                vgprs = (int)metadata_uint(fw.code->code, ".vgpr_count");
                break;
            }
        }
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        set_error("specialise: no current device");
        return SRACK_ERR_DEVICE;
    }
    const std::string arch = device_arch();
    const std::string kkey = std::to_string(dev) + ":" + cache_key(arch, src);
    if (auto have = kernel_cache_find(kkey)) {
        *out = have;
        if (how) *how = JitFetchInfo{0, 0.0, budget, vgprs, src.find("_bank_lds[") != std::string::npos};
        return SRACK_OK;
    }
    const Fetched f = fetch_code(arch, src);
    if (f.rc != SRACK_OK) {
        set_error(f.err);
        return f.rc;
    }
    if (how) *how = JitFetchInfo{f.how, f.compile_ms, budget, vgprs, src.find("_bank_lds[") != std::string::npos};
    hipModule_t mod = nullptr;
    hipError_t e = hipModuleLoadData(&mod, f.code->code.data());
    if (e != hipSuccess) {
        set_error(std::string("hipModuleLoadData: ") + hipGetErrorString(e));
        return SRACK_ERR_DEVICE;
    }
    auto k = std::make_shared<JitKernel>();
    k->module = mod;  // (unloaded by ~JitKernel on every path from here)
    hipFunction_t fn = nullptr;
    e = hipModuleGetFunction(&fn, mod, "srk_voice");
    if (e != hipSuccess) {
        set_error(std::string("hipModuleGetFunction: ") + hipGetErrorString(e));
        return SRACK_ERR_DEVICE;
    }
    k->function = fn;
    *out = kernel_cache_keep(kkey, k);  // (another thread may have loaded it meanwhile: one module per kernel and device)
    return SRACK_OK;
}

int jit_launch(const JitKernel& k, const KernelArgs& ka, uint32_t n_blocks, void* stream)
{
    KernelArgs args = ka;
    size_t size = sizeof(args);
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    hipError_t e = hipModuleLaunchKernel((hipFunction_t)k.function, n_blocks, 1, 1, 64, 1, 1, 0, (hipStream_t)stream, nullptr, config);
    if (e != hipSuccess) {
        set_error(std::string("hipModuleLaunchKernel: ") + hipGetErrorString(e));
        return SRACK_ERR_DEVICE;
    }
    return SRACK_OK;
}

}  // namespace srack
