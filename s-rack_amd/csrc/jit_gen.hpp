// jit_gen.hpp — the kernel generator of the general path's fast half (jit_gen.cpp): a pure function from a flattened program and a few
// integers to the HIP source of its voice kernel.  Host code only — no HIP header, no device header: it builds with a plain C++17
// compiler next to graph.cpp, approx.cpp, flatten.cpp and srk.cpp (tests/cpp/jit_dump.cpp).  The text is the kernel cache's key
// (jit_cache.hpp); compiling and loading it is jit.hpp's.
#pragma once
#include <string>

#include "flatten.hpp"

namespace srack {

constexpr int kMixRowsHost = 32;  // = kMixRows of wave.hip.h: samples per tile of the specialised and the fused kernels

// Can the generator express this program?  (`why` names the first obstacle.)
bool jit_supported(const FlatProgram& P, std::string* why = nullptr);
// Can every unit of the control program be generated too (co-scheduled with the voice blocks)?
bool jit_ctl_supported(const FlatPair& pair, std::string* why = nullptr);
// The HIP source of the kernel for the pair's voice program with the given output mode (1 frames, 2 mix, 3 both, 4 neither);
// with_ctl: the control program's units ride along as blocks [0, block0) of every launch (KernelArgs::ctl_slots).
// waves: > 0 asks the compiler for a register budget that lets so many waves share a SIMD (amdgpu_waves_per_eu): see jit_get.
int jit_source(const FlatPair& pair, int out_mode, bool with_ctl, std::string& src, int waves = 0, int want_waves = 0);  // want_waves: waves per SIMD the render has for the kernel (what LDS it may spend)

}  // namespace srack
