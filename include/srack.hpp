// srack.hpp — C++ host-side mirror of the reference's module-graph API, on top of the C ABI (srack_hip.h).
//
// The reference is Rust; its toolchain is not part of this build, so the host side above the C ABI is
// given in C++ with the reference's names and error behaviour, so that code (and tests) written against
// `trait SynthModule` / `plan_execution` / `execute` (src/synth.rs:97-263) read the same here:
//
//   reference                                   this header
//   ------------------------------------------  -------------------------------------------------------
//   AudioConfig{sample_rate, buffer_size, ch}    srack::AudioConfig
//   Arc<RwLock<dyn SynthModule>> (SharedSynthModule)  srack::SharedSynthModule (value handle: workspace + index)
//   OscillatorModule::new(&cfg) pushed to the    ws.add(srack::ModuleType::Oscillator)
//     workspace's module list (ui.rs:54)
//   m.set_input(i, src, port) -> Result<(),()>   m.set_input(i, src, port) -> bool   (false = Err(()))
//   m.get_input(i) / disconnect_input(i)         m.get_input(i) / m.disconnect_input(i)
//   m.get_num_inputs() / get_num_outputs()       same
//   plan_execution(output, &all_modules, &mut plan)   srack::plan_execution(output, all_modules, plan)
//   execute(&plan) once per buffer_size frames   ws.execute_batch(n_voices, n_samples, d_frames, d_mix)
//
// Header-only; link with libsrack_hip.so.  No HIP types appear: device buffers are void* / float*.
#pragma once
#include <cstdint>
#include <array>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "srack_hip.h"

namespace srack {

struct AudioConfig {  // synth.rs:20-25
    uint16_t sample_rate = 48000;
    size_t buffer_size = 1024;
    uint8_t channels = 2;
};

enum class ModuleType : int {  // the hot-path subset of SynthModuleType (synth.rs:300-317)
    Output = SRACK_MOD_OUTPUT,
    Oscillator = SRACK_MOD_OSCILLATOR,
    MoogFilter = SRACK_MOD_MOOG_FILTER,
    ADSR = SRACK_MOD_ADSR,
    VCA = SRACK_MOD_VCA,
    MonoMixer = SRACK_MOD_MONO_MIXER,
    Math = SRACK_MOD_MATH,
    GridSequencer = SRACK_MOD_GRID_SEQUENCER,
    PatternSequencer = SRACK_MOD_PATTERN_SEQUENCER,
    NonLinear = SRACK_MOD_NONLINEAR,
    Sample = SRACK_MOD_SAMPLE,
    Noise = SRACK_MOD_NOISE,
    Freeverb = SRACK_MOD_FREEVERB
};

class Error : public std::runtime_error {  // what the reference would panic with
public:
    Error(int code, const std::string& what) : std::runtime_error(what), code(code) {}
    int code;
};

class Workspace;

// Value handle with pointer-identity semantics, like an Arc clone (synth.rs:270, ByAddress in the planner).
class SharedSynthModule {
public:
    SharedSynthModule() = default;
    bool operator==(const SharedSynthModule& o) const { return ws_ == o.ws_ && index_ == o.index_; }
    bool operator!=(const SharedSynthModule& o) const { return !(*this == o); }
    int index() const { return index_; }

    std::string get_name() const;  // SynthModule::get_name
    uint8_t get_num_inputs() const;
    uint8_t get_num_outputs() const;
    // Result<(), ()>: false on a bad port index
    bool set_input(uint8_t input_idx, const SharedSynthModule& src_module, uint8_t src_port);
    bool disconnect_input(uint8_t input_idx);
    void disconnect_inputs()
    {
        for (uint8_t i = 0; i < get_num_inputs(); i++) disconnect_input(i);
    }
    // Result<Option<(SharedSynthModule, u8)>, ()>: outer nullopt = Err(()), inner nullopt = None
    std::optional<std::optional<std::pair<SharedSynthModule, uint8_t>>> get_input(uint8_t input_idx) const;
    // struct fields (what the egui sliders and serde touch), by the SRACK_<TYPE>_<FIELD> enums
    void set(int field, double value);
    double get(int field) const;
    // sequencer grid cells (sequencer.rs:137-184, 437-478) and the sample player's WaveBox (sample.rs:31-69)
    void set_step(int channel, int step, int state, int value = 0);
    void set_wave(const std::vector<float>& samples, float sample_rate);

private:
    friend class Workspace;
    SharedSynthModule(Workspace* ws, int index) : ws_(ws), index_(index) {}
    Workspace* ws_ = nullptr;
    int index_ = -1;
};

// SynthModuleWorkspaceImpl (ui.rs:52-60): owns the module list and the plan.
class Workspace {
public:
    explicit Workspace(const AudioConfig& cfg) : cfg_(cfg)
    {
        int rc = srack_patch_create(cfg.sample_rate, (uint32_t)cfg.buffer_size, cfg.channels, &p_);
        if (rc != SRACK_OK) throw Error(rc, srack_last_error());
    }
    ~Workspace() { srack_patch_destroy(p_); }
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;

    // Module::new(&audio_config) + push to `modules`
    SharedSynthModule add(ModuleType t)
    {
        int i = srack_patch_add_module(p_, (int)t);
        if (i < 0) throw Error(i, srack_last_error());
        return SharedSynthModule(this, i);
    }
    std::vector<SharedSynthModule> modules()
    {
        std::vector<SharedSynthModule> v;
        for (int i = 0; i < srack_patch_num_modules(p_); i++) v.emplace_back(SharedSynthModule(this, i));
        return v;
    }
    // SynthModuleWorkspaceImpl::plan (ui.rs:63-82): output = first OutputModule; empty plan when there is none
    std::vector<SharedSynthModule> plan()
    {
        int order[1024];
        int n = srack_patch_plan(p_, order, 1024);
        std::vector<SharedSynthModule> v;
        for (int i = 0; i < n; i++) v.emplace_back(SharedSynthModule(this, order[i]));
        return v;
    }
    // the wires that became buffer_size-sample delays (src, src_port, sink, sink_port)
    std::vector<std::array<int, 4>> delayed_edges()
    {
        int q[4 * 256];
        int n = srack_patch_delayed_edges(p_, q, 256);
        std::vector<std::array<int, 4>> v;
        for (int i = 0; i < n; i++) v.push_back({q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]});
        return v;
    }

    // ---- the batch counterpart of `execute(&plan)` ---------------------------------------------------
    void configure_voices(uint32_t n_voices) { check(srack_voices_configure(p_, n_voices)); }
    // the reference's sliders and cables change under a running graph: edits between execute_batch calls keep the voices' state
    void keep_state(bool keep = true) { check(srack_patch_keep_state(p_, keep ? 1 : 0)); }
    // NoiseModule streams: (seed, module, first_voice + voice); the reference's generator is OS-seeded
    void set_noise_seed(uint64_t seed, uint64_t first_voice = 0) { check(srack_patch_set_noise_seed(p_, seed, first_voice)); }
    void set_voice_field(const SharedSynthModule& m, int field, const float* values) { check(srack_voices_set_field_f32(p_, m.index(), field, values)); }
    int planes(int* channel_plane = nullptr, int cap = 0) { return check(srack_render_planes(p_, channel_plane, cap)); }
    // n_samples ticks for every voice, continuing from the current state; device pointers, asynchronous on `stream`
    void execute_batch(uint32_t n_samples, float* d_frames, float* d_mix, uint32_t flags = 0, void* stream = nullptr)
    {
        check(srack_render(p_, n_samples, d_frames, d_mix, flags, stream));
    }
    // MonoMixerModule's `*dst += src * gain` over voices: a gain and a bus per voice (n_voices entries each, nullptr: bus 0 / gain 1),
    // one mix per bus.  The table is not part of the program: changing it between execute_batch calls restarts nothing.
    void set_buses(uint32_t n_buses, const int* bus = nullptr, const float* gain = nullptr) { check(srack_voices_set_buses(p_, n_buses, bus, gain)); }
    uint32_t get_buses(int* bus = nullptr, float* gain = nullptr, uint32_t cap = 0) const { return (uint32_t)check(srack_voices_get_buses(p_, bus, gain, cap)); }
    // The same table with up to SRACK_MAX_VOICE_SLOTS buses per voice and a gain per channel: bus [n_voices][n_slots] (nullptr: slot 0 is
    // bus 0), gain [n_voices][n_slots][channels] (nullptr: 1).  Pan is one slot with a gain per channel, a per-voice send a second slot; the
    // fold still reads each frame once.  One table per handle: set_buses and set_bus_slots replace each other.
    void set_bus_slots(uint32_t n_buses, uint32_t n_slots, const int* bus = nullptr, const float* gain = nullptr) { check(srack_voices_set_bus_slots(p_, n_buses, n_slots, bus, gain)); }
    uint32_t get_bus_slots(int* n_slots = nullptr, int* bus = nullptr, float* gain = nullptr, uint32_t cap = 0) const { return (uint32_t)check(srack_voices_get_bus_slots(p_, n_slots, bus, gain, cap)); }
    // A wave per voice for a SampleModule: a bank of n_waves waves back to back (lengths, rates; copied) and, per voice, an index into it
    // or SRACK_WAVE_OWN (the module's own wave).  Voice v plays what a one-voice patch plays after set_wave(bank wave wave[v], its rate).
    void set_wave_bank(const SharedSynthModule& m, const float* samples, const int* lengths, const float* sample_rates, uint32_t n_waves)
    {
        check(srack_patch_set_wave_bank(p_, m.index(), samples, lengths, sample_rates, n_waves));
    }
    uint32_t get_wave_bank(const SharedSynthModule& m, int* lengths = nullptr, float* sample_rates = nullptr, uint32_t cap = 0) const
    {
        return (uint32_t)check(srack_patch_get_wave_bank(p_, m.index(), lengths, sample_rates, cap));
    }
    uint32_t get_wave_bank_samples(const SharedSynthModule& m, int wave, float* samples = nullptr, uint32_t cap = 0) const
    {
        return (uint32_t)check(srack_patch_get_wave_bank_samples(p_, m.index(), wave, samples, cap));
    }
    void set_voice_waves(const SharedSynthModule& m, const int* wave) { check(srack_voices_set_waves(p_, m.index(), wave)); }  // nullptr clears
    uint32_t get_voice_waves(const SharedSynthModule& m, int* wave = nullptr, uint32_t cap = 0) const { return (uint32_t)check(srack_voices_get_waves(p_, m.index(), wave, cap)); }
    // A sequence per voice for a grid (C = 1) or pattern (C = 8) sequencer: a bank of sequences — states u8 [n][C][64] as set_step's, the
    // grid's note values u16 [n][64] (nullptr: all 0), lengths [n] in 1..64 — and, per voice, an index into it or SRACK_SEQ_OWN (the
    // module's own cells and length).  An assignment edits cells: under keep_state every voice's step and held CV carry over.
    void set_sequence_bank(const SharedSynthModule& m, const uint8_t* states, const uint16_t* values, const int* lengths, uint32_t n_sequences)
    {
        check(srack_patch_set_sequence_bank(p_, m.index(), states, values, lengths, n_sequences));
    }
    uint32_t get_sequence_bank(const SharedSynthModule& m, uint8_t* states = nullptr, uint16_t* values = nullptr, int* lengths = nullptr, uint32_t cap = 0) const
    {
        return (uint32_t)check(srack_patch_get_sequence_bank(p_, m.index(), states, values, lengths, cap));
    }
    void set_voice_sequences(const SharedSynthModule& m, const int* seq) { check(srack_voices_set_sequences(p_, m.index(), seq)); }  // nullptr clears
    uint32_t get_voice_sequences(const SharedSynthModule& m, int* seq = nullptr, uint32_t cap = 0) const { return (uint32_t)check(srack_voices_get_sequences(p_, m.index(), seq, cap)); }
    // A stereo Freeverb per mix bus, behind the mixer: params f64 [n_buses][SRACK_FREEVERB__NFIELDS] in FreeverbModule's field order
    // (nullptr: the module's defaults), enabled [n_buses] (nullptr: every bus).  Calling set_bus_reverbs again is the slider: the
    // coefficients change, the tails stay.  Not part of the program: restarts nothing, and the tails carry on across an edit of the patch.
    void set_bus_reverbs(const double* params = nullptr, const int* enabled = nullptr) { check(srack_buses_set_reverb(p_, params, enabled)); }
    uint32_t get_bus_reverbs(double* params = nullptr, int* enabled = nullptr, uint32_t cap = 0) const { return (uint32_t)check(srack_buses_get_reverb(p_, params, enabled, cap)); }
    void reset_bus_reverbs() { check(srack_buses_reset_reverb(p_)); }  // lines and filter states to zero; the parameters stay
    void bus_reverb_plan(int* line_lengths /* 24 */, int* block) const { check(srack_buses_reverb_plan(p_, line_lengths, block)); }
    // d_bus_mix f32 [n_buses][channels][n_samples] -> d_bus_fx f32 [n_buses][2][n_samples] (no overlap), asynchronous on `stream`.  A sharded
    // host reduces the per-rank bus mixes first and reverberates on the root.
    void bus_reverb(uint32_t n_samples, const float* d_bus_mix, float* d_bus_fx, void* stream = nullptr)
    {
        check(srack_buses_reverb(p_, n_samples, d_bus_mix, d_bus_fx, stream));
    }
    // The master section: a gain per bus and channel (f32 [n_buses][2]; nullptr: 1.0f everywhere), the buses summed to one stereo pair in an
    // order that depends on n_buses alone.  Not part of the program: restarts nothing, and the gains survive an edit of the patch.
    void set_master(const float* gain = nullptr) { check(srack_buses_set_master(p_, gain)); }
    uint32_t get_master(float* gain = nullptr, uint32_t cap = 0) const { return (uint32_t)check(srack_buses_get_master(p_, gain, cap)); }
    // d_rows f32 [n_buses][row_channels][n_samples] -> d_master f32 [2][n_samples] (no overlap); d_master_stats f64 [2][SRACK_STAT_COUNT],
    // added to, or null.  Asynchronous on `stream`.  A sharded host reduces the bus mixes first and takes the master on the root.
    void master(uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_master, double* d_master_stats = nullptr, void* stream = nullptr)
    {
        check(srack_buses_master(p_, n_samples, d_rows, row_channels, d_master, d_master_stats, stream));
    }
    // The bus sends: send i adds gain[i][c] * rows[src[i]][c] to bus dst[i], every bus keeps its own row times through[b][c] (gain f32
    // [n_sends][2], through f32 [n_buses][2]; nullptr: 1.0f everywhere).  n_sends == 0 removes them.  Not part of the program: restarts
    // nothing, and the sends survive an edit of the patch.
    void set_sends(uint32_t n_sends, const int* src, const int* dst, const float* gain = nullptr, const float* through = nullptr)
    {
        check(srack_buses_set_sends(p_, n_sends, src, dst, gain, through));
    }
    uint32_t get_sends(int* src = nullptr, int* dst = nullptr, float* gain = nullptr, uint32_t cap = 0, float* through = nullptr, uint32_t through_cap = 0) const
    {
        return (uint32_t)check(srack_buses_get_sends(p_, src, dst, gain, cap, through, through_cap));
    }
    // -> the number of runs; n_terms [n_buses] (through term included), order: the send indices grouped by destination ascending
    uint32_t send_plan(int* n_terms = nullptr, uint32_t bus_cap = 0, int* order = nullptr, uint32_t order_cap = 0) const
    {
        return (uint32_t)check(srack_buses_send_plan(p_, n_terms, bus_cap, order, order_cap));
    }
    // d_rows f32 [n_buses][row_channels][n_samples] -> d_out of the same shape (no overlap): one level of routing, per destination the
    // master's order of additions over its terms.  Asynchronous on `stream`.  A sharded host reduces the bus mixes first and sends on the root.
    void send(uint32_t n_samples, const float* d_rows, uint32_t row_channels, float* d_out, void* stream = nullptr)
    {
        check(srack_buses_send(p_, n_samples, d_rows, row_channels, d_out, stream));
    }
    // A Moog ladder per mix bus, behind the mixer: params f32 [n_buses][SRACK_BUS_FILTER_NPARAMS] = frequency, resonance, CV amount (any f32;
    // nullptr: the module's defaults), port [n_buses] SRACK_VCF_OUT_* (nullptr: lowpass), enabled [n_buses] (nullptr: every bus).  Calling
    // set_bus_filter again is the slider: parameters change, state stays.  Not part of the program: restarts nothing, survives an edit.
    void set_bus_filter(const float* params = nullptr, const int* port = nullptr, const int* enabled = nullptr) { check(srack_buses_set_filter(p_, params, port, enabled)); }
    uint32_t get_bus_filter(float* params = nullptr, int* port = nullptr, int* enabled = nullptr, uint32_t cap = 0) const
    {
        return (uint32_t)check(srack_buses_get_filter(p_, params, port, enabled, cap));
    }
    void reset_bus_filter() { check(srack_buses_reset_filter(p_)); }  // every state to zero; the parameters stay
    // state f32 [n_buses][2][SRACK_BUS_FILTER_NSTATE] (host), behind a wait for the last filter call; a disabled bus reads as zeros
    uint32_t bus_filter_state(float* state = nullptr, uint32_t cap = 0) { return (uint32_t)check(srack_buses_filter_state(p_, state, cap)); }
    // d_rows f32 [n_buses][row_channels][n_samples] -> d_out of the same shape: d_rows itself (in place) or disjoint; d_cv f32
    // [n_buses][n_samples] or null (the CV port unconnected).  Asynchronous on `stream`.  A sharded host reduces the bus mixes first.
    void bus_filter(uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream = nullptr)
    {
        check(srack_buses_filter(p_, n_samples, d_rows, row_channels, d_cv, d_out, stream));
    }
    // An ADSR and a VCA per mix bus, behind the mixer: params f32 [n_buses][SRACK_BUS_VCA_NPARAMS] = attack, decay, sustain, release (any f32;
    // nullptr: the module's defaults), mode [n_buses] SRACK_BUS_VCA_* (nullptr: every bus GATE), negative [n_buses] (nullptr: false).  Calling
    // set_bus_vca again is the slider: sliders change, state stays; a bus that becomes GATE starts fresh.  Not part of the program.
    void set_bus_vca(const float* params = nullptr, const int* mode = nullptr, const int* negative = nullptr) { check(srack_buses_set_vca(p_, params, mode, negative)); }
    uint32_t get_bus_vca(float* params = nullptr, int* mode = nullptr, int* negative = nullptr, uint32_t cap = 0) const
    {
        return (uint32_t)check(srack_buses_get_vca(p_, params, mode, negative, cap));
    }
    void reset_bus_vca() { check(srack_buses_reset_vca(p_)); }  // every state fresh; the setting stays
    // state f32 [n_buses][SRACK_BUS_VCA_NSTATE] (host), behind a wait for the last call; a bus that is not GATE reads as the fresh state
    uint32_t bus_vca_state(float* state = nullptr, uint32_t cap = 0) { return (uint32_t)check(srack_buses_vca_state(p_, state, cap)); }
    // d_rows f32 [n_buses][row_channels][n_samples] -> d_out of the same shape: d_rows itself (in place) or disjoint; d_ctl f32
    // [n_buses][n_samples], the gate or CV per bus, or null (unconnected); d_env of d_ctl's shape, written, or null.  Asynchronous on `stream`.
    void bus_vca(uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_ctl, float* d_out, float* d_env = nullptr, void* stream = nullptr)
    {
        check(srack_buses_vca(p_, n_samples, d_rows, row_channels, d_ctl, d_out, d_env, stream));
    }
    // An LFO per mix bus writes the console's control rows: params f32 [n_buses][SRACK_BUS_OSC_NPARAMS] = val, depth, offset (any f32; nullptr:
    // 0, 1, 0), port [n_buses] SRACK_OSC_OUT_* (nullptr: sine), antialiasing [n_buses] (nullptr: true), enabled [n_buses] (nullptr: all).  The
    // reference's oscillator bit for bit, times depth, plus offset.  Calling set_bus_osc again is the slider: state stays; a bus that becomes
    // enabled starts fresh.  Not part of the program.
    void set_bus_osc(const float* params = nullptr, const int* port = nullptr, const int* antialiasing = nullptr, const int* enabled = nullptr)
    {
        check(srack_buses_set_osc(p_, params, port, antialiasing, enabled));
    }
    uint32_t get_bus_osc(float* params = nullptr, int* port = nullptr, int* antialiasing = nullptr, int* enabled = nullptr, uint32_t cap = 0) const
    {
        return (uint32_t)check(srack_buses_get_osc(p_, params, port, antialiasing, enabled, cap));
    }
    // every state fresh (phase 0, last true), or bus b at phase pos[b] in [0, 1) (f64 [n_buses], host; not -0.0); the setting stays
    void reset_bus_osc(const double* pos = nullptr) { check(srack_buses_reset_osc(p_, pos)); }
    // state f64 [n_buses][SRACK_BUS_OSC_NSTATE] (host): phase and last (0.0 / 1.0), behind a wait for the last call; a disabled bus reads fresh
    uint32_t bus_osc_state(double* state = nullptr, uint32_t cap = 0) { return (uint32_t)check(srack_buses_osc_state(p_, state, cap)); }
    // d_cv, d_sync f32 [n_buses][n_samples] or null (unconnected) -> d_out f32 [n_buses][n_samples], disjoint from both: what bus_filter's
    // d_cv, bus_vca's d_ctl and bus_shaper's d_cv take.  A disabled bus's row is +0.0f.  Asynchronous on `stream`.
    void bus_osc(uint32_t n_samples, const float* d_cv, const float* d_sync, float* d_out, void* stream = nullptr)
    {
        check(srack_buses_osc(p_, n_samples, d_cv, d_sync, d_out, stream));
    }
    // A drive, a waveshaper and a make-up gain per mix bus, behind the mixer: params f32 [n_buses][SRACK_BUS_SHAPER_NPARAMS] = pre, exponent,
    // post (any f32; nullptr: 1, 1, 1), mode [n_buses] SRACK_BUS_SHAPER_* (nullptr: every bus CONST).  sign(a) |a|^e with the host libm's powf,
    // bit for bit.  Calling set_bus_shaper again is the slider; there is no state.  Not part of the program.
    void set_bus_shaper(const float* params = nullptr, const int* mode = nullptr) { check(srack_buses_set_shaper(p_, params, mode)); }
    uint32_t get_bus_shaper(float* params = nullptr, int* mode = nullptr, uint32_t cap = 0) const { return (uint32_t)check(srack_buses_get_shaper(p_, params, mode, cap)); }
    // d_rows f32 [n_buses][row_channels][n_samples] -> d_out of the same shape: d_rows itself (in place) or disjoint; d_cv f32
    // [n_buses][n_samples], the exponent of a CV bus sample by sample, or null (its EXPONENT then).  Asynchronous on `stream`.
    void bus_shaper(uint32_t n_samples, const float* d_rows, uint32_t row_channels, const float* d_cv, float* d_out, void* stream = nullptr)
    {
        check(srack_buses_shaper(p_, n_samples, d_rows, row_channels, d_cv, d_out, stream));
    }
    // The bus meters, a read-only tap between any two console calls: d_rows f32 [n_buses][row_channels][n_samples] -> d_levels f64
    // [n_windows][SRACK_STAT_COUNT][n_buses][2] (record k: stream positions [k * window, (k + 1) * window); the call's samples are
    // first_sample .. first_sample + n_samples - 1) and d_totals f64 [SRACK_STAT_COUNT][n_buses][2]; either may be null, not both.  Both
    // are ADDED TO: zero-fill once, cut the stream into calls as you like.  No state on the handle.  Asynchronous on `stream`.
    void bus_meter(uint64_t first_sample, uint32_t n_samples, const float* d_rows, uint32_t row_channels, uint32_t window, double* d_levels,
                   uint32_t n_windows, double* d_totals, void* stream = nullptr)
    {
        check(srack_buses_meter(p_, first_sample, n_samples, d_rows, row_channels, window, d_levels, n_windows, d_totals, stream));
    }
    // execute_batch plus d_bus_mix, f32 [n_buses][channels][n_samples] (written); d_frames, d_mix, d_stats may each be null
    void execute_batch_buses(uint32_t n_samples, float* d_frames, float* d_mix, double* d_stats, float* d_bus_mix, uint32_t flags = 0, void* stream = nullptr)
    {
        check(srack_render_buses(p_, n_samples, d_frames, d_mix, d_stats, d_bus_mix, flags, stream));
    }

    srack_patch* handle() { return p_; }
    const AudioConfig& config() const { return cfg_; }
    int check(int rc) const
    {
        if (rc < 0) throw Error(rc, srack_last_error());
        return rc;
    }

private:
    friend class SharedSynthModule;
    AudioConfig cfg_;
    srack_patch* p_ = nullptr;
};

// The multi-GPU half (no reference counterpart: s-rack is single-threaded, main.rs:59-63): one process per GPU, voices sharded by
// global voice index, and one collective — the sum of the per-rank partial mixes.  Rank 0 makes the id, the host carries its
// 128 bytes to every rank, every rank constructs a MixComm with its device already selected (srack_device_set).
class MixComm {
public:
    static std::string unique_id()
    {
        std::string id((size_t)SRACK_DIST_ID_BYTES, '\0');
        const int rc = srack_dist_unique_id(&id[0]);
        if (rc < 0) throw Error(rc, srack_last_error());
        return id;
    }
    MixComm(const std::string& id, int n_ranks, int rank)
    {
        if (id.size() != (size_t)SRACK_DIST_ID_BYTES) throw Error(SRACK_ERR_INVALID, "MixComm: the id is SRACK_DIST_ID_BYTES bytes");
        const int rc = srack_dist_init(id.data(), n_ranks, rank, &comm_);
        if (rc < 0) throw Error(rc, srack_last_error());
    }
    MixComm(const MixComm&) = delete;
    MixComm& operator=(const MixComm&) = delete;
    ~MixComm() { srack_dist_destroy(comm_); }
    int count() const
    {
        int n = 0;
        const int rc = srack_dist_comm_count(comm_, &n);
        if (rc < 0) throw Error(rc, srack_last_error());
        return n;
    }
    // ncclReduce(sum, f32) of `count` floats at device pointer d_mix, in place, asynchronous on `stream`
    void reduce_mix(float* d_mix, size_t count, int root = 0, void* stream = nullptr)
    {
        const int rc = srack_dist_reduce_mix(comm_, d_mix, count, root, stream);
        if (rc < 0) throw Error(rc, srack_last_error());
    }

private:
    void* comm_ = nullptr;
};

inline std::string SharedSynthModule::get_name() const
{
    static const char* names[] = {"Output", "Oscillator", "Moog Filter", "ADSR", "VCA", "Mono Mixer", "Math",
                                  "Grid Sequencer", "Pattern Sequencer", "Non-Linear", "Sample", "Noise", "Freeverb"};  // each module's get_name()
    int t = srack_patch_module_type(ws_->p_, index_);
    if (t == SRACK_MOD_MATH) {
        static const char* ops[] = {"Add", "Subtract", "Multiply"};  // math.rs:37-43
        return ops[(int)get(SRACK_MATH_OPERATION) % 3];
    }
    return t >= 0 && t < SRACK_MOD__COUNT ? names[t] : "?";
}
inline uint8_t SharedSynthModule::get_num_inputs() const { return (uint8_t)ws_->check(srack_module_num_inputs(ws_->p_, index_)); }
inline uint8_t SharedSynthModule::get_num_outputs() const { return (uint8_t)ws_->check(srack_module_num_outputs(ws_->p_, index_)); }
inline bool SharedSynthModule::set_input(uint8_t input_idx, const SharedSynthModule& src, uint8_t src_port)
{
    return srack_patch_connect(ws_->p_, src.index_, src_port, index_, input_idx) == SRACK_OK;
}
inline bool SharedSynthModule::disconnect_input(uint8_t input_idx) { return srack_patch_disconnect(ws_->p_, index_, input_idx) == SRACK_OK; }
inline std::optional<std::optional<std::pair<SharedSynthModule, uint8_t>>> SharedSynthModule::get_input(uint8_t input_idx) const
{
    int m = -1, port = 0;
    if (srack_patch_get_input(ws_->p_, index_, input_idx, &m, &port) != SRACK_OK) return std::nullopt;  // Err(())
    if (m < 0) return std::optional<std::pair<SharedSynthModule, uint8_t>>{};                            // Ok(None)
    return std::optional<std::pair<SharedSynthModule, uint8_t>>{std::make_pair(SharedSynthModule(ws_, m), (uint8_t)port)};
}
inline void SharedSynthModule::set(int field, double value) { ws_->check(srack_patch_set_field(ws_->p_, index_, field, value)); }
inline void SharedSynthModule::set_step(int channel, int step, int state, int value) { ws_->check(srack_patch_set_step(ws_->p_, index_, channel, step, state, value)); }
inline void SharedSynthModule::set_wave(const std::vector<float>& samples, float sample_rate)
{
    ws_->check(srack_patch_set_wave(ws_->p_, index_, samples.data(), (uint32_t)samples.size(), sample_rate));
}
inline double SharedSynthModule::get(int field) const
{
    double v = 0;
    ws_->check(srack_patch_get_field(ws_->p_, index_, field, &v));
    return v;
}

// get_inputs (synth.rs:214-218)
inline std::vector<std::optional<std::pair<SharedSynthModule, uint8_t>>> get_inputs(const SharedSynthModule& m)
{
    std::vector<std::optional<std::pair<SharedSynthModule, uint8_t>>> v;
    for (uint8_t i = 0; i < m.get_num_inputs(); i++) v.push_back(*m.get_input(i));
    return v;
}

// plan_execution(output, &all_modules, &mut plan) (synth.rs:128-212), explicit list as in the reference's test
inline void plan_execution(Workspace& ws, const SharedSynthModule& output, const std::vector<SharedSynthModule>& all_modules,
                           std::vector<SharedSynthModule>& plan)
{
    std::vector<int> list, order(all_modules.size() + 1);
    for (const auto& m : all_modules) list.push_back(m.index());
    int n = ws.check(srack_patch_plan_list(ws.handle(), output.index(), list.data(), (int)list.size(), order.data(), (int)order.size()));
    auto mods = ws.modules();
    plan.clear();
    for (int i = 0; i < n; i++) plan.push_back(mods[(size_t)order[(size_t)i]]);
}

}  // namespace srack
