// launch.hpp — what render.hip and console.cpp call to launch the pre-built kernels.  Every kernel family is a translation unit of its own (its kernels
// in its own header, its launch functions in <family>.hip), so this header carries only what both sides of that seam need: the
// launch-side types, the dispatch helpers several families share, and the launch functions' declarations.  No kernel is visible here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "busfx_args.hpp"
#include "kernel_args.hip.h"
#include "launch_types.hpp"

namespace srack {

struct FlatProgram;  // flatten.hpp

// The hand-written kernel a program takes (render.hip, pick_kernel).
enum class Kernel { Interp, VoiceChain, VoiceChainTrack, SeqChain, FmPair, FmPairRing, FmPairSplit, FmPairBlock, FmPairBlockX, FmPairX };

// ---- kernel launches (template parameters from runtime port flags and output modes) ----------------
// f(std::integral_constant<int, O>) with the output mode as a compile-time constant: 3 frames + mix, 1 frames, 2 mix; 0 for anything else —
// the instantiation that decides at run time (a render that asks for neither only advances the voice state).  Every kernel family takes
// its output mode from here; one that has no instantiation of its own for a mode says so where it calls.
template <class Fn>
static auto with_out_mode(int out_mode, Fn&& f)
{
    switch (out_mode) {
    case 3: return f(std::integral_constant<int, 3>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 0>{});
    }
}

// ... and f(std::integral_constant<uint32_t, P>) for the one of three output ports a flag word names (anything else: the last)
template <uint32_t P0, uint32_t P1, uint32_t P2, class Fn>
static void with_port(uint32_t port, Fn&& f)
{
    if (port == P0)
        f(std::integral_constant<uint32_t, P0>{});
    else if (port == P1)
        f(std::integral_constant<uint32_t, P1>{});
    else
        f(std::integral_constant<uint32_t, P2>{});
}
template <class Fn>
static void with_osc_port(uint32_t port, Fn&& f)
{
    with_port<OSC_OUT_SAW, OSC_OUT_SQUARE, OSC_OUT_SINE>(port, f);
}

// ---- the chain family (fused.hip.h): render_voice_chain / render_voice_chain_track and the control block ----
// One translation unit per audio oscillator port: defined in chain_unit.hip.h, instantiated in chain_saw.hip, chain_square.hip and
// chain_sine.hip.  launch_fused (chain.hip) picks the unit.
template <uint32_t kOscAPort>
void launch_chain(uint32_t vcf_port, bool exact, int out_mode, bool track, const KernelArgs& ka, const ChainRoles& roles, const CtlWork& co, dim3 grid, hipStream_t st);
void launch_fused(uint32_t osc_port, uint32_t vcf_port, bool exact, int out_mode, bool track, const KernelArgs& ka, const ChainRoles& roles, const CtlWork& co,
                  dim3 grid, hipStream_t st);
void launch_ctl_gate_env(const CtlWork& w, hipStream_t st);  // render_ctl_gate_env on its own: one wave
#ifdef SRK_WAVE_CENSUS
// Tools-only build: every port's unit has its own srk_census_rec (fused.hip.h).  A launch of render_voice_chain_track copies *census_rec
// into its unit's on the launch's stream first (null: the launch is not recorded); the pointee must outlive that copy.
extern uint32_t* const* census_rec;
#endif

// ---- render_voice_chain_seq (seq.hip) ----
void launch_seq(uint32_t osc_port, int out_mode, const KernelArgs& ka, const SeqRoles& r, dim3 grid, hipStream_t st);

// ---- the z^-1 FM pairs (fm_pair.hip) and the time-parallel ones (fm_block.hip) ----
void launch_fm_pair(Kernel kernel, bool exact, int out_mode, const KernelArgs& ka, const ChainRoles& roles, dim3 grid, hipStream_t st);
void launch_fm_pair_x(int out_mode, const KernelArgs& ka, const ChainRoles& roles, dim3 grid, hipStream_t st);
// (the one launch that can fail before it starts: it asks for its LDS first)
hipError_t launch_fm_block(bool x, int out_mode, const KernelArgs& ka, const ChainRoles& roles, hipStream_t st);

// ---- the tile interpreter (interp.hip) ----
inline size_t interp_lds_bytes(const DevProgram& H)
{
    return ((size_t)H.n_rows + 2 + (size_t)H.n_tracks + (size_t)H.n_slots * H.tile) * 256;  // + zero, trash and track rows
}
// debug_occ: render.hip's SRACK_DEBUG_OCC knob (tools/) — what the runtime says about resident workgroups per CU for this LDS size
void launch_interp(const FlatProgram& P, const KernelArgs& ka, hipStream_t st, bool debug_occ);
// the control pipeline: one block per control unit, `slots` its argument blocks of this launch
void launch_interp_stages(bool exact, uint32_t n_stages, size_t lds, const KernelArgs* slots, hipStream_t st);

// ---- the bus reverbs (busfx.hip): a workgroup per bus of a.tab, n_buses of them ----
void launch_bus_reverb(const BusFxArgs& a, uint32_t n_buses, hipStream_t st);

// ---- the master section (master.hip): run sums into a.runs, the tree over them into a.master, a.stats when given ----
void launch_master(const MasterArgs& a, hipStream_t st);

// ---- the bus sends (sends.hip): every destination's run sums, into a.out or a.scratch, and the tree over the scratch rows into a.out ----
void launch_sends(const SendArgs& a, hipStream_t st);

// ---- the bus filters (busvcf.hip): a lane per row of a.tab, a wave per workgroup; the disabled buses' rows copied when a.out is not a.rows ----
void launch_bus_filter(const BusVcfArgs& a, hipStream_t st);

// ---- the bus VCAs (busvca.hip): a workgroup of eight waves per 64 buses of a.tab, the envelopes on its first wave ----
void launch_bus_vca(const BusVcaArgs& a, hipStream_t st);

// ---- the bus oscillators (busosc.hip): a lane per enabled bus of a.tab, a wave per workgroup; the disabled buses' rows of a.out zeroed ----
void launch_bus_osc(const BusOscArgs& a, hipStream_t st);

// ---- the bus shapers (busshape.hip): a wave per stretch of kBusShaperStretch samples of a bus, a.n_units of them, four to a workgroup ----
void launch_bus_shaper(const BusShaperArgs& a, hipStream_t st);

// ---- the bus meters (busmeter.hip): a lane per (bus, channel) row, a wave per workgroup; reads a.rows, continues a.levels and a.totals ----
void launch_bus_meter(const BusMeterArgs& a, hipStream_t st);

}  // namespace srack
