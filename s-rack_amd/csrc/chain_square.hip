// chain_square.hip — the render_voice_chain and render_voice_chain_track kernels whose audio oscillator emits its square port (chain_unit.hip.h).
#include "chain_unit.hip.h"

namespace srack {
template void launch_chain<OSC_OUT_SQUARE>(uint32_t, bool, int, bool, const KernelArgs&, const ChainRoles&, const CtlWork&, dim3, hipStream_t);
}
