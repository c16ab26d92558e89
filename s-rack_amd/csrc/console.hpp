// console.hpp — the host side of the bus console (console.cpp): the eight stages behind the mixer — sends, reverbs, VCAs, shapers, filters,
// master section, meters, and the oscillators that write their control rows — as they hang off the handle.  None of them is part of the program or of DeviceState (that is replaced on every re-flatten,
// and a reverb's tail or a filter's state carries on across an edit of the patch); all are dropped with the mix table.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/srack_hip.h"
#include "program.hpp"

namespace srack {

struct PatchHandle;  // runtime.hpp

// The stream contract of a stage, stated once.  A stage's calls may come on different streams and its device
// memory is one: every call begins behind the call before it and leaves an event behind its kernels, and whoever frees or rewrites
// what those kernels read waits for that event on the host first.
struct StageSync {
    void* ev_done = nullptr;  // hipEvent_t recorded behind every call's kernels
    int begin(void* stream);  // the first call creates the event, every later one makes its stream wait for it
    int end(void* stream);    // the launches' error, if any, and the event behind them
    void wait();              // on the host, for the last call's kernels; nothing to wait for before the first call
    void destroy();
};

// A device allocation of a stage that only grows.
struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;
    // At least `want` bytes.  Allocated first and swapped in on success, the old one freed behind sync.wait(); a failure leaves the old
    // one in place, says "<who>: out of device memory for <what> (<want> bytes)" and returns SRACK_ERR_NOMEM.  The contents do not move.
    int grow(StageSync& sync, size_t want, const char* who, const char* what);
    void release();
};

// The state of a stage that keeps kFields values of T per bus, indexed by bus: T [kFields][n_buses] on the device between calls, every
// value as the C ABI hands it out, so nothing moves when the set of buses that own state changes.  A bus that owns none holds the fresh
// state there — what that is, field by field, the stage says with every call (`one`).  When the set changes, the state comes to the
// host, the buses that joined or left are made fresh (`pending`) and it goes up again before the next call's kernel.  Whatever reads or
// rewrites the device's copy waits on the host for the last call's kernels first (console.cpp).
template <class T, int kFields>
struct BusState {
    using Fresh = std::array<T, kFields>;
    // device side; nothing of it exists before the stage's first call
    DeviceBuf d_state;       // T [kFields][n_buses]
    bool fresh = true;       // every state is to be made fresh before the next call uses it (nothing ran yet, or a reset)
    std::vector<T> pending;  // [kFields][n_buses] the state to be uploaded before the next call; empty: none
    static std::vector<T> filled(const Fresh& one, size_t n);  // [kFields][n], every bus fresh
    bool all_fresh() const { return pending.empty() && (!d_state.p || fresh); }
    void reset();            // every state fresh, before the next call uses it
    int fetch(StageSync& sync, const Fresh& one, size_t n, std::vector<T>& out);  // the state as it stands: pending, or fresh, or the device's
    // owns(b) is about to become will_own(b): a bus for which it changes is made fresh; one that keeps its state keeps it
    template <class Owns, class WillOwn>
    int refresh(StageSync& sync, const Fresh& one, size_t n, Owns owns, WillOwn will_own);
    int alloc(StageSync& sync, size_t n, const char* who, const char* what);  // before a call: the device's copy exists (DeviceBuf::grow) ...
    int upload(StageSync& sync, const Fresh& one, size_t n);                  // ... and holds what is pending, or fresh states after a reset
    template <class Owns>
    int hand_out(StageSync& sync, const Fresh& one, size_t n_buses, Owns owns, T* state, uint32_t cap);  // host, [cap][kFields]; a bus that owns none reads fresh
};

// The bus reverbs (srack_buses_set_reverb / srack_buses_reverb): one Freeverb per mix bus.
struct BusFx {
    bool set = false;
    std::vector<double> params;     // [n_buses][SRACK_FREEVERB__NFIELDS], as the host gave them
    std::vector<uint8_t> enabled;   // [n_buses]
    uint32_t len[kFvLines] = {}, first[kFvLines] = {}, total = 0;  // the lines at the patch's sample rate (freeverb_params.hpp)
    uint32_t block = 0;             // samples the kernel takes at a time: min(256, shortest line)
    uint64_t counter = 0;           // samples processed since the last reset: every line's position is counter mod length
    // device side; nothing of it exists before the first srack_buses_reverb
    std::vector<double*> d_state;   // [n_buses] filter states + lines of an enabled bus; null: disabled, or not allocated yet
    std::vector<uint8_t> fresh;     // [n_buses] the state is to be zeroed before the next call uses it
    DeviceBuf d_tab;                // BusFxDev [n_buses]
    bool tab_dirty = true;
    StageSync sync;
    uint32_t last_enabled = 0, last_block = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

// The master section (srack_buses_set_master / srack_buses_master): a gain per bus and channel, the buses summed to one stereo pair.
struct Master {
    bool set = false;
    std::vector<float> gain;        // [n_buses][2] as the host gave them; empty: 1.0f everywhere
    // device side; nothing of it exists before the first srack_buses_master
    DeviceBuf d_gain;               // f32 [n_buses][2]
    bool gain_dirty = true;
    DeviceBuf d_runs;               // the run sums, f32 [n_runs][2][n_samples]: grown on demand
    StageSync sync;
    uint32_t last_buses = 0;        // srack_render_info, once a call has run
    bool ran = false;
};

// The bus sends (srack_buses_set_sends / srack_buses_send): aux sends from bus to bus, a gather-sum per destination bus.
struct Sends {
    bool set = false;
    std::vector<int32_t> src, dst;  // [n_sends] as the host gave them
    std::vector<float> gain;        // [n_sends][2]
    std::vector<float> through;     // [n_buses][2]
    // the plan, made when the sends are set (capi.cpp, sends_plan_make)
    std::vector<int32_t> n_terms;   // [n_buses] through term included
    std::vector<int32_t> order;     // [n_sends] send indices grouped by destination ascending, stable
    std::vector<uint32_t> term_src; // [n_buses + n_sends] the terms in that order, each destination's through term first
    std::vector<float> term_gain;   // [n_buses + n_sends][2]
    std::vector<uint32_t> runs;     // SendRun [n_runs] (launch_types.hpp), four words each
    std::vector<uint32_t> multi;    // SendMulti [n_multi], four words each
    uint32_t scratch_rows = 0;      // the runs of the destinations that have several
    uint32_t max_blocks = 0;
    // device side; nothing of it exists before the first srack_buses_send
    DeviceBuf d_tab;                // term_src | term_gain | runs | multi, each 16-byte aligned
    bool tab_dirty = true;
    DeviceBuf d_scratch;            // f32 [scratch_rows][2][n_samples]: grown on demand
    StageSync sync;
    uint32_t last_sends = 0, last_runs = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

// The bus filters (srack_buses_set_filter / srack_buses_filter): a Moog ladder per enabled bus and channel.
// The state of (enabled bus, channel) sits in slot 2 * (the bus's place among the enabled ones) + channel, on the device between calls
// as f32 [slots / 64][SRACK_BUS_FILTER_NSTATE][64] (busvcf.hip.h).  Whenever the enabled set changes the slots move: the state comes to
// the host, is laid out anew (`pending`) and goes up again before the next call's kernel.
struct BusVcf {
    bool set = false;
    std::vector<float> params;      // [n_buses][SRACK_BUS_FILTER_NPARAMS], as the host gave them
    std::vector<int32_t> port;      // [n_buses]
    std::vector<uint8_t> enabled;   // [n_buses]
    // device side; nothing of it exists before the first srack_buses_filter
    DeviceBuf d_state;              // f32 [slots / 64][10][64], slots a multiple of 64
    bool fresh = true;              // the state is to be zeroed before the next call uses it (nothing ran yet, or reset_filter)
    std::vector<float> pending;     // [slots][10] the state in the layout of `enabled`, to be uploaded before the next call; empty: none
    DeviceBuf d_tab;                // BusVcfRow [n_rows], then u32 [n_copy]: the rows of the disabled buses
    bool tab_dirty = true;          // parameters, ports or the enabled set changed ...
    uint32_t tab_row_channels = 0;  // ... or a call comes with another row_channels than the table was made for
    uint32_t n_rows = 0, n_copy = 0;
    StageSync sync;
    uint32_t last_enabled = 0, last_waves = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

// The bus VCAs (srack_buses_set_vca / srack_buses_vca): an ADSRModule and its VCAModules per mix bus.
// The state is a BusState of f32 [SRACK_BUS_VCA_NSTATE] per bus (busvca.hip.h) that the GATE buses own.
struct BusVca {
    bool set = false;
    std::vector<float> params;      // [n_buses][SRACK_BUS_VCA_NPARAMS], as the host gave them
    std::vector<int32_t> mode;      // [n_buses] SRACK_BUS_VCA_OFF / _CV / _GATE
    std::vector<uint8_t> negative;  // [n_buses]
    float rate = 0.0f;              // the f32 sample rate a fresh ADSRModule of this patch carries (Graph::adsr_sample_rate)
    BusState<float, SRACK_BUS_VCA_NSTATE> state;
    // device side; nothing of it exists before the first srack_buses_vca
    DeviceBuf d_tab;                // BusVcaBus [n_buses]
    bool tab_dirty = true;          // sliders, modes or flags changed
    StageSync sync;
    uint32_t last_on = 0, last_gated = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

// The bus oscillators (srack_buses_set_osc / srack_buses_osc): an OscillatorModule and two MathModules per enabled mix bus.
// The state is a BusState of f64 [SRACK_BUS_OSC_NSTATE] per bus (busosc.hip.h) that the enabled buses own; reset_osc with phases goes
// up as `pending`, too.
struct BusOsc {
    bool set = false;
    std::vector<float> params;      // [n_buses][SRACK_BUS_OSC_NPARAMS], as the host gave them
    std::vector<int32_t> port;      // [n_buses] SRACK_OSC_OUT_*
    std::vector<uint8_t> aa;        // [n_buses]
    std::vector<uint8_t> enabled;   // [n_buses]
    double rate = 0.0;              // f64(the patch's sample rate)
    BusState<double, SRACK_BUS_OSC_NSTATE> state;
    // device side; nothing of it exists before the first srack_buses_osc
    DeviceBuf d_tab;                // BusOscBus [n_on], then u32 [n_off]: the disabled buses
    bool tab_dirty = true;          // parameters, ports, flags or the enabled set changed
    uint32_t n_on = 0, n_off = 0;
    StageSync sync;
    uint32_t last_on = 0;           // srack_render_info, once a call has run
    bool last_cv = false, last_sync = false;
    bool ran = false;
};

// The bus shapers (srack_buses_set_shaper / srack_buses_shaper): a drive, a NonLinearModule and a make-up gain per mix bus and channel.
// No state: the setting, and on the device a table entry per bus with the list of the buses that are not OFF behind it (busshape.hip.h).
struct BusShaper {
    bool set = false;
    std::vector<float> params;      // [n_buses][SRACK_BUS_SHAPER_NPARAMS], as the host gave them
    std::vector<int32_t> mode;      // [n_buses] SRACK_BUS_SHAPER_OFF / _CONST / _CV
    // device side; nothing of it exists before the first srack_buses_shaper
    DeviceBuf d_tab;                // BusShaperBus [n_buses], then u32 [n_on]: the buses that are not OFF
    bool tab_dirty = true;          // constants or modes changed
    StageSync sync;
    uint32_t last_on = 0, last_cv = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

// The bus meters (srack_buses_meter): a read-only tap on the bus rows.  The records and totals are the caller's buffers and the stream
// position is the caller's count, so there is nothing to own: no setting, no device memory, no event — only what srack_render_info says.
struct BusMeter {
    uint32_t last_buses = 0, last_window = 0;  // srack_render_info, once a call has run; window 0: only totals were taken
    bool ran = false;
};

struct Console {
    BusFx busfx;
    Master master;
    Sends sends;
    BusVcf busvcf;
    BusVca busvca;
    BusShaper busshaper;
    BusMeter busmeter;
    BusOsc busosc;
};

void device_console_drop(PatchHandle& h);               // all eight stages: settings, device memory, events and notes
std::string device_console_note(const PatchHandle& h);  // the notes of the stages that have run: sends, busosc, busvcf, busvca, busshp, busfx, master, meter
// The bus reverbs: one call's work enqueued on `stream` (allocating and zeroing what is missing); state handling without a call.
int device_buses_reverb(PatchHandle& h, uint32_t n_samples, const float* d_bus_mix, float* d_bus_fx, void* stream);
void device_busfx_free_bus(PatchHandle& h, uint32_t bus);  // the bus's state, once no call uses it any more
// The master section: one call's work enqueued on `stream` (uploading the gains when they changed, growing the scratch).
int device_buses_master(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_master, double* d_master_stats, void* stream);
void device_master_gains_changed(PatchHandle& h);  // the host's gains were replaced: the next call uploads them
// The bus sends: one call's work enqueued on `stream` (uploading the tables when they changed, growing the scratch).
int device_buses_send(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_out, void* stream);
void device_sends_changed(PatchHandle& h);  // the host's list was replaced: the next call uploads the tables
void device_sends_drop(PatchHandle& h);     // list, tables, scratch and the note
// The bus filters: one call's work enqueued on `stream` (allocating, zeroing and uploading what is missing); state handling without a call.
int device_buses_filter(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream);
int device_busvcf_enable(PatchHandle& h, const std::vector<uint8_t>& enabled);  // the enabled set is about to become this: the state moves to its new slots
int device_busvcf_state(PatchHandle& h, float* state, uint32_t cap);            // host, f32 [cap][2][10] as the C ABI hands it out, behind a wait for the last call
void device_busvcf_changed(PatchHandle& h);  // parameters, ports or the enabled set were replaced: the next call makes the table anew
void device_busvcf_reset(PatchHandle& h);    // every state to zero, before the next call uses it
// The bus VCAs: one call's work enqueued on `stream` (allocating and uploading what is missing); state handling without a call.
int device_buses_vca(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_ctl, float* d_out, float* d_env, void* stream);
int device_busvca_modes(PatchHandle& h, const std::vector<int32_t>& mode);  // the modes are about to become these: a bus that joins or leaves GATE is made fresh
int device_busvca_state(PatchHandle& h, float* state, uint32_t cap);        // host, f32 [cap][6] as the C ABI hands it out, behind a wait for the last call
void device_busvca_changed(PatchHandle& h);  // sliders, modes or flags were replaced: the next call uploads the table
void device_busvca_reset(PatchHandle& h);    // every state fresh, before the next call uses it
// The bus oscillators: one call's work enqueued on `stream` (allocating and uploading what is missing); state handling without a call.
int device_buses_osc(PatchHandle& h, uint32_t n_samples, const float* d_cv, const float* d_sync, float* d_out, void* stream);
int device_busosc_enable(PatchHandle& h, const std::vector<uint8_t>& enabled);  // the enabled set is about to become this: a bus that joins or leaves is made fresh
int device_busosc_state(PatchHandle& h, double* state, uint32_t cap);           // host, f64 [cap][2] as the C ABI hands it out, behind a wait for the last call
void device_busosc_changed(PatchHandle& h);                 // parameters, ports, flags or the enabled set were replaced: the next call makes the table anew
void device_busosc_reset(PatchHandle& h, const double* pos);  // every state fresh (pos null) or at phase pos[b], last true, before the next call uses it
// The bus shapers: one call's work enqueued on `stream` (allocating and uploading the table when it is missing or changed).
int device_buses_shaper(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream);
void device_busshaper_changed(PatchHandle& h);  // constants or modes were replaced: the next call uploads the table
// The bus meters: one call's kernel enqueued on `stream`; d_levels or d_totals may be null, not both.
int device_buses_meter(PatchHandle& h, uint64_t first_sample, uint32_t n_samples, const float* d_rows, uint32_t row_channels, uint32_t window,
                       double* d_levels, uint32_t n_windows, double* d_totals, void* stream);

}  // namespace srack
