// runtime.hpp — the object behind `srack_patch*`: graph + voices + flattened program + device state.
#pragma once
#include <cstdint>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "buses.hpp"
#include "flatten.hpp"
#include "graph.hpp"

namespace srack {

struct DeviceState;  // HIP side, render.hip

// The bus reverbs (srack_buses_set_reverb): one Freeverb per mix bus, behind the mixer.  NOT part of the program, and not part of
// DeviceState either — that is replaced on every re-flatten, and a reverb's tail carries on across an edit of the patch.
struct BusFx {
    bool set = false;
    std::vector<double> params;     // [n_buses][SRACK_FREEVERB__NFIELDS], as the host gave them
    std::vector<uint8_t> enabled;   // [n_buses]
    uint32_t len[kFvLines] = {}, first[kFvLines] = {}, total = 0;  // the lines at the patch's sample rate (freeverb_params.hpp)
    uint32_t block = 0;             // samples the kernel takes at a time: min(256, shortest line)
    uint64_t counter = 0;           // samples processed since the last reset: every line's position is counter mod length
    // device side (render.hip); nothing of it exists before the first srack_buses_reverb
    std::vector<double*> d_state;   // [n_buses] filter states + lines of an enabled bus; null: disabled, or not allocated yet
    std::vector<uint8_t> fresh;     // [n_buses] the state is to be zeroed before the next call uses it
    void* d_tab = nullptr;          // BusFxDev [n_buses]
    size_t tab_buses = 0;
    bool tab_dirty = true;
    void* ev_done = nullptr;        // hipEvent_t recorded behind every call's kernel: the next call, and whoever frees or rewrites, waits for it
    uint32_t last_enabled = 0, last_block = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

// The master section (srack_buses_set_master / srack_buses_master): a gain per bus and channel, the buses summed to one stereo pair.
// Like the reverbs it hangs off the handle: not the program's, not DeviceState's; dropped with the table.
struct Master {
    bool set = false;
    std::vector<float> gain;        // [n_buses][2] as the host gave them; empty: 1.0f everywhere
    // device side (render.hip); nothing of it exists before the first srack_buses_master
    void* d_gain = nullptr;         // f32 [gain_buses][2]
    size_t gain_buses = 0;
    bool gain_dirty = true;
    void* d_runs = nullptr;         // the run sums, f32 [n_runs][2][n_samples]: grown on demand
    size_t runs_floats = 0;
    void* ev_done = nullptr;        // hipEvent_t behind every call's kernels: the next call, and whoever frees or rewrites, waits for it
    uint32_t last_buses = 0;        // srack_render_info, once a call has run
    bool ran = false;
};

// The bus sends (srack_buses_set_sends / srack_buses_send): aux sends from bus to bus, a gather-sum per destination bus.  Like the
// master's gains they hang off the handle: not the program's, not DeviceState's; dropped with the table.
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
    // device side (render.hip); nothing of it exists before the first srack_buses_send
    void* d_tab = nullptr;          // term_src | term_gain | runs | multi, each 16-byte aligned
    size_t tab_bytes = 0;
    bool tab_dirty = true;
    void* d_scratch = nullptr;      // f32 [scratch_rows][2][n_samples]: grown on demand
    size_t scratch_floats = 0;
    void* ev_done = nullptr;        // hipEvent_t behind every call's kernels: the next call, and whoever frees or rewrites, waits for it
    uint32_t last_sends = 0, last_runs = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

// The bus filters (srack_buses_set_filter / srack_buses_filter): a Moog ladder per enabled bus and channel, behind the mixer.  Like the
// reverbs they hang off the handle: not the program's, not DeviceState's; dropped with the table.
// The state of (enabled bus, channel) sits in slot 2 * (the bus's place among the enabled ones) + channel, on the device between calls
// as f32 [slots / 64][SRACK_BUS_FILTER_NSTATE][64] (busvcf.hip.h).  Whenever the enabled set changes the slots move: the state comes to
// the host, is laid out anew (`pending`) and goes up again before the next call's kernel.
struct BusVcf {
    bool set = false;
    std::vector<float> params;      // [n_buses][SRACK_BUS_FILTER_NPARAMS], as the host gave them
    std::vector<int32_t> port;      // [n_buses]
    std::vector<uint8_t> enabled;   // [n_buses]
    // device side (render.hip); nothing of it exists before the first srack_buses_filter
    void* d_state = nullptr;        // f32 [state_slots / 64][10][64]
    size_t state_slots = 0;         // a multiple of 64
    bool fresh = true;              // the state is to be zeroed before the next call uses it (nothing ran yet, or reset_filter)
    std::vector<float> pending;     // [slots][10] the state in the layout of `enabled`, to be uploaded before the next call; empty: none
    void* d_tab = nullptr;          // BusVcfRow [n_rows], then u32 [n_copy]: the rows of the disabled buses
    size_t tab_bytes = 0;
    bool tab_dirty = true;          // parameters, ports or the enabled set changed ...
    uint32_t tab_row_channels = 0;  // ... or a call comes with another row_channels than the table was made for
    uint32_t n_rows = 0, n_copy = 0;
    void* ev_done = nullptr;        // hipEvent_t behind every call's kernels: the next call, and whoever frees or rewrites, waits for it
    uint32_t last_enabled = 0, last_waves = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

// The bus VCAs (srack_buses_set_vca / srack_buses_vca): an ADSRModule and its VCAModules per mix bus, behind the mixer.  Like the filters
// they hang off the handle: not the program's, not DeviceState's; dropped with the table.
// The state is indexed by bus, f32 [SRACK_BUS_VCA_NSTATE][n_buses] on the device between calls, every value as the C ABI hands it out
// (busvca.hip.h): nothing moves when modes change.  A bus that is not GATE holds the fresh state there; when the set of GATE buses
// changes, the state comes to the host, the buses that joined or left are made fresh (`pending`) and it goes up again before the
// next call's kernel.
struct BusVca {
    bool set = false;
    std::vector<float> params;      // [n_buses][SRACK_BUS_VCA_NPARAMS], as the host gave them
    std::vector<int32_t> mode;      // [n_buses] SRACK_BUS_VCA_OFF / _CV / _GATE
    std::vector<uint8_t> negative;  // [n_buses]
    float rate = 0.0f;              // the f32 sample rate a fresh ADSRModule of this patch carries (Graph::adsr_sample_rate)
    // device side (render.hip); nothing of it exists before the first srack_buses_vca
    void* d_state = nullptr;        // f32 [6][n_buses]
    bool fresh = true;              // every state is to be made fresh before the next call uses it (nothing ran yet, or reset_vca)
    std::vector<float> pending;     // [6][n_buses] the state to be uploaded before the next call; empty: none
    void* d_tab = nullptr;          // BusVcaBus [n_buses]
    bool tab_dirty = true;          // sliders, modes or flags changed
    void* ev_done = nullptr;        // hipEvent_t behind every call's kernel: the next call, and whoever frees or rewrites, waits for it
    uint32_t last_on = 0, last_gated = 0;  // srack_render_info, once a call has run
    bool ran = false;
};

struct PatchHandle {
    Graph graph;
    uint32_t n_voices = 0;
    std::vector<VoiceOverride> overrides;
    uint64_t voices_revision = 0;  // bumped by configure / per-voice set_field

    FlatPair prog;
    bool prog_valid = false;
    uint64_t prog_graph_revision = 0, prog_voices_revision = 0;
    uint32_t prog_flags = 0;

    DeviceState* dev = nullptr;
    uint64_t samples_rendered = 0;  // absolute tick count: phase of the feedback rings
    bool keep_state = false;        // srack_patch_keep_state: carry the modules' device state across a re-flatten
    bool voices_fresh = true;       // set by srack_voices_configure: nothing on the device belongs to these voices yet
    // keep_state: the device state of the program that was replaced, kept until the new one is uploaded (rings and reverb lines
    // move device to device), with what it held and where
    DeviceState* dev_old = nullptr;
    struct OldTag {
        int stage;  // -1: the voice program
        uint32_t n_voices;
        FlatProgram::CarryTag tag;
    };
    std::vector<OldTag> old_tags;
    // keep_state: (module, field) pairs of STATE fields the host wrote since the last flatten — the carry leaves those alone
    // (an explicit srack_patch_set_field / srack_voices_set_field_* on a state field wins over the running value)
    std::set<std::pair<int, int>> state_writes;
    // The mix table of the voices (srack_voices_set_buses): NOT part of the program — setting it re-flattens nothing and restarts nothing.
    // n_buses 0: no table.  The plan is what the bus fold reads (buses.hpp), made when the table is set; the device copy follows bus_revision.
    uint32_t n_buses = 0;
    std::vector<int32_t> bus;
    std::vector<float> bus_gain;
    BusPlan bus_plan;
    uint64_t bus_revision = 0;
    BusFx busfx;                    // the bus reverbs; dropped with the table (srack_voices_configure, another n_buses)
    Master master;                  // the master section; dropped with the table as well
    Sends sends;                    // the bus sends; dropped with the table as well
    BusVcf busvcf;                  // the bus filters; dropped with the table as well
    BusVca busvca;                  // the bus VCAs; dropped with the table as well
    bool timing_armed = false;      // srack_render_kernel_ms has been called: renders bracket the dominant kernel with HIP events

    ~PatchHandle();
};

// (Re)flatten when the graph, the voices or the flags changed since the last render; a re-flatten
// resets the device voice state to the modules' fields (like re-loading the patch).
int ensure_program(PatchHandle& h, uint32_t flags);
// The program `flags` would render, without touching the handle (its own if current, else flattened from a copy into `scratch`).
int peek_program(PatchHandle& h, uint32_t flags, FlatPair& scratch, const FlatPair** out);

int device_render(PatchHandle& h, uint32_t n_samples, float* d_frames, float* d_mix, double* d_stats, float* d_bus_mix, uint32_t flags, void* stream);
int device_reserve(PatchHandle& h, uint32_t n_samples, bool want_mix, uint32_t flags);
int device_kernel_ms(PatchHandle& h, double* avg_ms, int* n_launches, int reset);
int device_read_rows(PatchHandle& h, int ctl_stage /* -1: the voice program */, int first_row, int n_rows, uint32_t* host_dst);
// One state field of one module as the CURRENT program holds it on the device, per voice (no re-flatten); false: not device state.
bool read_device_state(PatchHandle& h, int module, int field, std::vector<double>& values);
void device_release(DeviceState* d);
const char* device_kernel_name(const PatchHandle& h);
// The bus reverbs: one call's work enqueued on `stream` (allocating and zeroing what is missing); state handling without a call.
int device_buses_reverb(PatchHandle& h, uint32_t n_samples, const float* d_bus_mix, float* d_bus_fx, void* stream);
void device_busfx_free_bus(PatchHandle& h, uint32_t bus);  // the bus's state, once no call uses it any more
void device_busfx_drop(PatchHandle& h);                    // parameters and state of every bus
std::string device_busfx_note(const PatchHandle& h);  // " busfx=3[block 244]" once a call has run, else ""
// The master section: one call's work enqueued on `stream` (uploading the gains when they changed, growing the scratch).
int device_buses_master(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_master, double* d_master_stats, void* stream);
void device_master_gains_changed(PatchHandle& h);  // the host's gains were replaced: the next call uploads them
void device_master_drop(PatchHandle& h);           // gains, scratch and the note
std::string device_master_note(const PatchHandle& h);  // " master=4096[64 runs]" once a call has run, else ""
// The bus sends: one call's work enqueued on `stream` (uploading the tables when they changed, growing the scratch).
int device_buses_send(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_out, void* stream);
void device_sends_changed(PatchHandle& h);  // the host's list was replaced: the next call uploads the tables
void device_sends_drop(PatchHandle& h);     // list, tables, scratch and the note
std::string device_sends_note(const PatchHandle& h);  // " sends=4092[4156 runs]" once a call has run, else ""
// The bus filters: one call's work enqueued on `stream` (allocating, zeroing and uploading what is missing); state handling without a call.
int device_buses_filter(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream);
int device_busvcf_enable(PatchHandle& h, const std::vector<uint8_t>& enabled);  // the enabled set is about to become this: the state moves to its new slots
int device_busvcf_state(PatchHandle& h, float* state, uint32_t cap);            // host, f32 [cap][2][10] as the C ABI hands it out, behind a wait for the last call
void device_busvcf_changed(PatchHandle& h);  // parameters, ports or the enabled set were replaced: the next call makes the table anew
void device_busvcf_reset(PatchHandle& h);    // every state to zero, before the next call uses it
void device_busvcf_drop(PatchHandle& h);     // parameters, state, table and the note
std::string device_busvcf_note(const PatchHandle& h);  // " busvcf=48[2 waves]" once a call has run, else ""
// The bus VCAs: one call's work enqueued on `stream` (allocating and uploading what is missing); state handling without a call.
int device_buses_vca(PatchHandle& h, uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_ctl, float* d_out, float* d_env, void* stream);
int device_busvca_modes(PatchHandle& h, const std::vector<int32_t>& mode);  // the modes are about to become these: a bus that joins or leaves GATE is made fresh
int device_busvca_state(PatchHandle& h, float* state, uint32_t cap);        // host, f32 [cap][6] as the C ABI hands it out, behind a wait for the last call
void device_busvca_changed(PatchHandle& h);  // sliders, modes or flags were replaced: the next call uploads the table
void device_busvca_reset(PatchHandle& h);    // every state fresh, before the next call uses it
void device_busvca_drop(PatchHandle& h);     // settings, state, table and the note
std::string device_busvca_note(const PatchHandle& h);  // " busvca=48[32 gated]" once a call has run, else ""
std::string device_bus_note(const PatchHandle& h);  // " buses=4096[fold]" when the last render filled bus mixes, else ""
std::string device_waves_note(const PatchHandle& h);  // " waves=9[lds]" / " waves=9[global]" for a patch that renders with a wave assignment, else ""
std::string device_sequences_note(const PatchHandle& h);  // " sequences=9[global]" for a patch that renders with a sequence assignment, else ""
std::string device_jit_note(const PatchHandle& h);  // " jit=compiled(1834 ms)" / " jit=disk-cache" / " jit=memory-cache" / " jit=unavailable(why)" / ""

}  // namespace srack
