/*
 * srack_hip.h — C ABI of the MI355X batch-render path for s-rack's module-graph evaluator.
 *
 * The reference (s-rack v0.3.1, Rust) has no FFI; its operator API for this path is the trait
 * `SynthModule` (src/synth.rs:222-263) plus the free functions `plan_execution`
 * (src/synth.rs:128-212) and `execute` (src/synth.rs:97-101).  This header is the flat,
 * value-typed mirror of exactly that surface: what a Rust host would bind with `extern "C"`
 * in place of `execute(&plan)` (the binding is shown in INTEGRATION.md).
 *
 * Conventions
 *   - every function returns `int`: 0 = ok, < 0 = error (the reference's `Err(())` / panic);
 *     `srack_last_error()` gives a thread-local message for the last failure.
 *   - the caller owns every host/device buffer it passes in; the library owns the handle and
 *     the device-side voice state hanging off it.
 *   - a handle is not thread-safe: one render at a time per handle (the reference holds the plan
 *     `Mutex` during `execute`, src/main.rs:60).
 *   - no callbacks into the host during a render; no torch / C++ types in any signature.
 *   - module indices are positions in the workspace's `all_modules` list (src/ui.rs:54): the
 *     planner's result depends on that order (src/synth.rs:193-211), so modules must be added
 *     in list order.
 */
#ifndef SRACK_HIP_H
#define SRACK_HIP_H

#ifndef __HIPCC_RTC__ /* (device code specialised at run time sees this header through hiprtc: no libc headers there) */
#include <stddef.h>
#include <stdint.h>
#else
using __hip_internal::int32_t;
using __hip_internal::int64_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define SRACK_ABI_VERSION 2 /* 2: srack_dist_unique_id / init / comm_count / destroy; save_srk rejects a short buffer */

/* ---- status codes ------------------------------------------------------------------------ */
enum {
    SRACK_OK              = 0,
    SRACK_ERR_INVALID     = -1, /* bad handle / argument (reference: panic or Err(())) */
    SRACK_ERR_PORT        = -2, /* port index out of range: `Err(())` of get_input/set_input/get_output */
    SRACK_ERR_NO_OUTPUT   = -3, /* no OutputModule in the list: find_output() Err, src/ui.rs:84-96 */
    SRACK_ERR_SELF_LOOP   = -4, /* module wired to itself: RwLock self-deadlock in the reference (src/synth.rs:99,251) */
    SRACK_ERR_STATE       = -5, /* call order violated (render before voices are configured, ...) */
    SRACK_ERR_UNSUPPORTED = -6, /* module type outside the hot-path scope */
    SRACK_ERR_DEVICE      = -7, /* HIP runtime error; text in srack_last_error() */
    SRACK_ERR_NOMEM       = -8
};

/* ---- module types: the ★ rows of the scope table ------------------------------------------ */
enum {
    SRACK_MOD_OUTPUT      = 0, /* output::OutputModule        src/synth/output.rs:7-60      */
    SRACK_MOD_OSCILLATOR  = 1, /* oscillator::OscillatorModule src/synth/oscillator.rs:9-158 */
    SRACK_MOD_MOOG_FILTER = 2, /* filter::MoogFilterModule    src/synth/filter.rs:11-221    */
    SRACK_MOD_ADSR        = 3, /* adsr::ADSRModule            src/synth/adsr.rs:7-217       */
    SRACK_MOD_VCA         = 4, /* vca::VCAModule              src/synth/vca.rs:6-148        */
    SRACK_MOD_MONO_MIXER  = 5, /* mixer::MonoMixerModule      src/synth/mixer.rs:6-122      */
    SRACK_MOD_MATH        = 6, /* math::MathModule            src/synth/math.rs:13-160      */
    /* scope table (f) rank 1: the clocked note sources that sit in front of the path in real patches */
    SRACK_MOD_GRID_SEQUENCER    = 7, /* sequencer::GridSequencerModule    src/synth/sequencer.rs:12-246   */
    SRACK_MOD_PATTERN_SEQUENCER = 8, /* sequencer::PatternSequencerModule src/synth/sequencer.rs:336-533 */
    /* scope table (f) rank 4: the remaining per-voice modules */
    SRACK_MOD_NONLINEAR   = 9,  /* math::NonLinearModule       src/synth/math.rs:176-311     */
    SRACK_MOD_SAMPLE      = 10, /* sample::SampleModule        src/synth/sample.rs:72-240    */
    /* White noise: out = (rand::random::<f32>() - 0.5) * 2.0 per sample (oscillator.rs:381-387).  The reference draws from
     * rand 0.8's thread-local, OS-seeded ChaCha12: no two runs of it agree, so only the DISTRIBUTION can be matched — the
     * 2^24 equally likely values k * 2^-23 - 1 of rand's Standard f32 — and the draw itself is this library's: a
     * counter-based splitmix64 stream per (seed, module, voice), see srack_patch_set_noise_seed. */
    SRACK_MOD_NOISE       = 11, /* oscillator::NoiseModule     src/synth/oscillator.rs:308-393 */
    /* Stereo reverb: the module (freeverb.rs:8-274) routes six parameters into, and ticks, `freeverb::Freeverb` of the
     * freeverb crate 0.1.0 (Cargo.lock:1479-1482), which is NOT vendored in the reference tree.  The crate is restated
     * from its published algorithm — Jezar's Freeverb: eight parallel lowpass-feedback combs and four series allpasses per
     * channel, the classic tunings scaled by sample_rate / 44100, f64 throughout — see oracle/srack_oracle.c for the
     * restatement and its status ("parity unpinned": no reference test or vector exercises it). */
    SRACK_MOD_FREEVERB    = 12, /* freeverb::FreeverbModule    src/synth/freeverb.rs:8-274     */
    SRACK_MOD__COUNT      = 13
};

/* ---- ports (u8 in the reference) --------------------------------------------------------- */
enum { SRACK_OSC_IN_CV = 0, SRACK_OSC_IN_SYNC = 1 };                        /* oscillator.rs:164-170 */
enum { SRACK_OSC_OUT_SINE = 0, SRACK_OSC_OUT_SQUARE = 1, SRACK_OSC_OUT_SAW = 2 }; /* oscillator.rs:90-97 */
enum { SRACK_VCF_IN_AUDIO = 0, SRACK_VCF_IN_CV = 1 };                       /* filter.rs:113-119 */
enum { SRACK_VCF_OUT_LOWPASS = 0, SRACK_VCF_OUT_BANDPASS = 1, SRACK_VCF_OUT_HIGHPASS = 2 }; /* filter.rs:166-172 */
enum { SRACK_ADSR_IN_GATE = 0 };                                            /* adsr.rs:77-82 */
enum { SRACK_VCA_IN_AUDIO = 0, SRACK_VCA_IN_CV = 1 };                       /* vca.rs:50-56 */
enum { SRACK_SAMPLE_IN_GATE = 0, SRACK_SAMPLE_IN_CV = 1 };                  /* sample.rs:166-172 */
enum { SRACK_FREEVERB_IN_LEFT = 0, SRACK_FREEVERB_IN_RIGHT = 1 };           /* freeverb.rs:139-145 */
enum { SRACK_FREEVERB_OUT_LEFT = 0, SRACK_FREEVERB_OUT_RIGHT = 1 };         /* freeverb.rs:192-198 */
enum { SRACK_SEQ_IN_STEP = 0, SRACK_SEQ_IN_SYNC = 1 };                      /* sequencer.rs:253-259, 543-549 */
enum { SRACK_GRIDSEQ_OUT_CV = 0, SRACK_GRIDSEQ_OUT_GATE = 1, SRACK_GRIDSEQ_OUT_SYNC = 2 }; /* sequencer.rs:291-298 */
enum { SRACK_PATSEQ_OUT_GATE0 = 0, SRACK_PATSEQ_OUT_SYNC = 8 };             /* gates 0..7, then sync (sequencer.rs:578-586) */

/* ---- fields: the serialisable struct members of each module (params AND runtime state) ---- */
/* Values travel as double (exact for f32, f64, bool, small ints). `mode`: see SRACK_ADSR_MODE_*. */
enum { /* OscillatorModule, oscillator.rs:10-24 */
    SRACK_OSC_VAL = 0,          /* f32, 1 V/oct offset; 0 => 440 Hz */
    SRACK_OSC_ANTIALIASING = 1, /* bool */
    SRACK_OSC_POS = 2,          /* f64 phase in [0,1) (state) */
    SRACK_OSC_SYNC_LAST = 3,    /* bool, TransitionDetector.last (state; starts true, synth.rs:283) */
    SRACK_OSC__NFIELDS = 4
};
enum { /* MoogFilterModule + InternalMoogFilterState, filter.rs:12-56 */
    SRACK_VCF_FREQ = 0, SRACK_VCF_RES = 1, SRACK_VCF_EXP_AMT = 2,
    SRACK_VCF_ST_F = 3, SRACK_VCF_ST_P = 4, SRACK_VCF_ST_Q = 5,
    SRACK_VCF_ST_B0 = 6, SRACK_VCF_ST_B1 = 7, SRACK_VCF_ST_B2 = 8, SRACK_VCF_ST_B3 = 9, SRACK_VCF_ST_B4 = 10,
    SRACK_VCF_ST_FREQ = 11, SRACK_VCF_ST_RES = 12,
    SRACK_VCF__NFIELDS = 13
};
enum { /* ADSRModule, adsr.rs:8-24 */
    SRACK_ADSR_A_SEC = 0, SRACK_ADSR_D_SEC = 1, SRACK_ADSR_S_VAL = 2, SRACK_ADSR_R_SEC = 3,
    SRACK_ADSR_PHASE = 4, SRACK_ADSR_MODE = 5, SRACK_ADSR_R_VAL = 6, SRACK_ADSR_FROM_A_VAL = 7,
    SRACK_ADSR_SAMPLE_RATE = 8, /* f32 copy taken at new(); NOT refreshed by set_audio_config (adsr.rs:69-71) */
    SRACK_ADSR_GATE_LAST = 9,   /* TransitionDetector.last */
    SRACK_ADSR__NFIELDS = 10
};
enum { SRACK_ADSR_MODE_ATTACK = 0, SRACK_ADSR_MODE_DECAY = 1, SRACK_ADSR_MODE_SUSTAIN = 2,
       SRACK_ADSR_MODE_RELEASE = 3, SRACK_ADSR_MODE_NONE = 4 };             /* adsr.rs:27-33 */
enum { SRACK_VCA_NEGATIVE = 0, SRACK_VCA__NFIELDS = 1 };                    /* vca.rs:14 */
enum { SRACK_MIX_GAIN0 = 0, SRACK_MIX_GAIN1 = 1, SRACK_MIX_GAIN2 = 2, SRACK_MIX_GAIN3 = 3,
       SRACK_MIX__NFIELDS = 4 };                                            /* mixer.rs:11 */
enum { SRACK_MATH_CONSTANT = 0, SRACK_MATH_OPERATION = 1, SRACK_MATH__NFIELDS = 2 }; /* math.rs:21-22 */
enum { SRACK_MATH_ADD = 0, SRACK_MATH_SUBTRACT = 1, SRACK_MATH_MULTIPLY = 2 };       /* math.rs:7-11 */
enum { /* GridSequencerModule, sequencer.rs:13-30 (the sequence itself: srack_patch_set_step) */
    SRACK_GRIDSEQ_STEPS_PER_OCTAVE = 0, /* u16, default 12 */
    SRACK_GRIDSEQ_OCTAVES = 1,          /* u8, UI only */
    SRACK_GRIDSEQ_LENGTH = 2,           /* sequence.len(), 1..64, default 64 */
    SRACK_GRIDSEQ_CURRENT_STEP = 3,     /* u16 (state) */
    SRACK_GRIDSEQ_STEP_LAST = 4,        /* transition_detector.last (state) */
    SRACK_GRIDSEQ_SYNC_LAST = 5,        /* sync_transition_detector.last (state) */
    SRACK_GRIDSEQ_LAST = 6,             /* f32: the CV held over empty steps (state) */
    SRACK_GRIDSEQ__NFIELDS = 7
};
enum { /* PatternSequencerModule, sequencer.rs:337-349 */
    SRACK_PATSEQ_LENGTH = 0,            /* sequence[0].len(), 1..64, default 64 */
    SRACK_PATSEQ_CURRENT_STEP = 1, SRACK_PATSEQ_STEP_LAST = 2, SRACK_PATSEQ_SYNC_LAST = 3,
    SRACK_PATSEQ__NFIELDS = 4
};
enum { SRACK_NONLIN_CONSTANT = 0 /* f32 exponent used when In2 is unconnected, default 1.0 */,
       SRACK_NONLIN__NFIELDS = 1 };                                         /* math.rs:177-185 */
enum { /* SampleModule + WaveBox, sample.rs:15-20, 72-85 (the samples themselves: srack_patch_set_wave) */
    SRACK_SAMPLE_SAMPLE_RATE = 0,      /* f32 copy of the audio sample rate */
    SRACK_SAMPLE_WAVE_SAMPLE_RATE = 1, /* f32 wavebox.sample_rate; 0.0 until a wave is set */
    SRACK_SAMPLE_WAVE_NEW = 2,         /* wavebox.new: the next render starts with pos = 0, playing = false */
    SRACK_SAMPLE_POS = 3,              /* f32 read position in wave samples (state) */
    SRACK_SAMPLE_PLAYING = 4,          /* bool (state) */
    SRACK_SAMPLE_GATE_LAST = 5,        /* transition_detector.last (state) */
    SRACK_SAMPLE__NFIELDS = 6
};
enum { /* FreeverbModule, freeverb.rs:19-30: the *_ctl members (what the sliders hold; calc() copies them into the reverb, :88-114).
        * All f64 except FREEZE (bool).  Per-voice overrides are not supported for this module. */
    SRACK_FREEVERB_DAMPENING = 0,      /* default 0.5, slider 0..2 */
    SRACK_FREEVERB_FREEZE = 1,         /* default false */
    SRACK_FREEVERB_WET = 2,            /* default 1.0 */
    SRACK_FREEVERB_WIDTH = 3,          /* default 0.5 */
    SRACK_FREEVERB_ROOM_SIZE = 4,      /* default 0.5 */
    SRACK_FREEVERB_DRY = 5,            /* default 0.0 */
    SRACK_FREEVERB__NFIELDS = 6
};
/* step contents for srack_patch_set_step.
 * Grid: sequence[step] = None | Some((value, hold)) (sequencer.rs:19);  Pattern: sequence[channel][step] = None | Some(false) | Some(true). */
enum { SRACK_STEP_NONE = 0, SRACK_STEP_ON = 1 /* Some((v,false)) / Some(false): gate follows the clock */,
       SRACK_STEP_HOLD = 2 /* Some((v,true)) / Some(true): gate held at 1.0 */ };

/* ---- render flags ------------------------------------------------------------------------- */
enum {
    SRACK_RENDER_DEFAULT    = 0,
    /* oscillator PolyBLEP in f64 with true division and f64 sin/pow, as the reference spells it
     * (oscillator.rs:43-67,132-152): saw/square bit-identical to the CPU tick, at ~2x VALU cost. */
    SRACK_RENDER_EXACT_OSC  = 1u << 0,
    /* never pick one of the hand-matched fused chain kernels: the patch takes the general path — a kernel specialised
     * for the flattened program at run time (below), or the tile interpreter */
    SRACK_RENDER_NO_FUSION  = 1u << 1,
    /* do not hoist voice-invariant sub-graphs into the control track; evaluate them per lane */
    SRACK_RENDER_NO_UNIFORM_HOIST = 1u << 2,
    /* evaluate the control program as one stage instead of a pipeline of dependency depths */
    SRACK_RENDER_NO_CTL_STAGES = 1u << 3,
    /* The general path.  A patch that matches none of the fused shapes is rendered by a kernel SPECIALISED for its flattened
     * program: the op list is turned into one straight-line HIP kernel over the same per-module device functions (wires and
     * module state in registers, control tracks through scalar loads, frames through buffer stores) and compiled for gfx950
     * with hiprtc, once per program structure (parameter values are not part of it), when the program is first used
     * (srack_render_reserve / first render: ~1 s).  By default that happens for renders of 4096 voices or more; smaller
     * ones, programs with the one module the generator does not cover (FreeverbModule) and hosts without hiprtc use the tile
     * interpreter, which executes the same device functions
     * tile by tile with the wires in LDS.  Both are parity-tested against the oracle. */
    SRACK_RENDER_NO_SPECIALIZE = 1u << 4, /* always the tile interpreter */
    SRACK_RENDER_SPECIALIZE    = 1u << 5, /* specialise whatever the voice count (fails loudly if it cannot) */
    /* Default mode decides per patch which of its cheaper forms each module takes, from a first-order error bound against the 1e-5
     * contract over a ten-minute render (csrc/approx.cpp; srack_render_info: "approx[bound 2.3e-06]").  Where the graph has an unbounded
     * error gain — a loop that amplifies, a ladder near self-oscillation, a loop through a gate or a pitch (BASELINE config 4's FM
     * feedback) — the oscillators behind it are evaluated exactly as the reference spells them ("; exact osc 0,3"), and a patch whose
     * VALUES have no bound, or with an unbounded gain behind a module without an exact form of its own (the sample player's pitch, a
     * NonLinear), is rendered in the exact flavour altogether ("approx[exact: ...]").  This flag keeps the default forms where the reason
     * is an unbounded GAIN (the f32 PolyBLEP / contracted ladder are still denied module by module where the bound asks for it): faster —
     * config 4: 7 ms per second of audio against 18.5 — and inside the contract for renders of seconds, not minutes ("approx[kept
     * default: ...]").  It does NOT waive "unbounded values": there the default forms' clamps treat a NaN differently from the
     * reference's min / max and the render is wrong from the first overflow on — such a patch stays exact. */
    SRACK_RENDER_KEEP_DEFAULT  = 1u << 6
};

typedef struct srack_patch srack_patch; /* opaque: the workspace's module list + plan + device voice state */

/* ---- library ------------------------------------------------------------------------------ */
int         srack_abi_version(void);
const char* srack_last_error(void);

/* ---- patch graph (host only; no GPU needed) ----------------------------------------------- */
/* AudioConfig{sample_rate:u16, buffer_size:usize, channels:u8}, synth.rs:20-25.
 * sample_rate must fit the reference's u16 (1..65535); buffer_size >= 1 is also the length of a
 * broken feedback edge's delay; channels = number of OutputModule inputs. */
int srack_patch_create(uint32_t sample_rate, uint32_t buffer_size, uint32_t channels, srack_patch** out);
int srack_patch_destroy(srack_patch* p);

/* `Module::new(&audio_config)` with the reference defaults, appended to all_modules.
 * Returns the module index (>= 0) or an error (< 0). */
int srack_patch_add_module(srack_patch* p, int module_type);
int srack_patch_num_modules(const srack_patch* p);
int srack_patch_module_type(const srack_patch* p, int module);
int srack_module_num_inputs(const srack_patch* p, int module);  /* SynthModule::get_num_inputs  */
int srack_module_num_outputs(const srack_patch* p, int module); /* SynthModule::get_num_outputs */

/* field access = the struct members egui sliders / serde touch.  Uniform across voices.
 * NOTE on state: the voices' running state lives on the device between renders.  Any edit of the patch after a render — a module,
 * a connection, a field (srack_patch_set_field, set_step, set_wave, set_noise_seed), a per-voice field, or a different `flags` argument
 * to srack_render — makes the next render re-flatten the patch and START AGAIN from the state stored in the patch (the state fields
 * as last set; the modules' defaults otherwise), sample counter 0.  Rendering with unchanged patch and flags continues seamlessly.
 * (The reference's sliders change a parameter without touching module state: srack_patch_keep_state below carries the modules'
 * state across an edit.  By hand it is: read the state fields back with srack_voices_get_field BEFORE the edit and set them as
 * per-voice fields — both tested bit for bit in tests/test_gpu_parity.py.) */
int srack_patch_set_field(srack_patch* p, int module, int field, double value);
int srack_patch_get_field(const srack_patch* p, int module, int field, double* value);
/* keep != 0: from now on an edit between renders no longer restarts the voices.  Before the patch is re-flattened, every
 * module's state fields (phases, filter states, envelope phases and modes, detector bits, sequencer steps, sampler positions) are
 * read back from the device, per voice, and become the starting state of the re-flattened program; the delay rings of feedback
 * edges and the reverbs' delay lines move device to device into the ring / reverb of the same module; the sample counter runs on.
 * (A ring or reverb whose module moves between the per-voice program and the voice-invariant control program in the edit is
 * broadcast to every voice, respectively taken from voice 0.)  srack_voices_configure always starts afresh.
 * With keep, every module of the plan is evaluated, as the reference's execute() does — by default modules that cannot influence
 * any output are skipped and their state stays as stored — so that a module wired into the audible graph later has run all along.
 * Default: off (an edit restarts the voices, as documented above). */
int srack_patch_keep_state(srack_patch* p, int keep);

/* Sequencer grid cells (the egui grid editors write these, sequencer.rs:137-184, 437-478).
 * Grid sequencer: channel must be 0, `value` is the note index (u16); pattern sequencer: channel 0..7, value ignored. */
int srack_patch_set_step(srack_patch* p, int module, int channel, int step, int state, int value);
int srack_patch_get_step(const srack_patch* p, int module, int channel, int step, int* state, int* value);

/* SampleModule's WaveBox as WaveBox::load leaves it (sample.rs:31-69): the first channel of the file as
 * f32 samples (copied), the file's sample rate, and new = true.  Shared by every voice.
 * get_wave copies up to `cap` samples and returns the wave's length. */
int srack_patch_set_wave(srack_patch* p, int module, const float* samples, uint32_t n_samples, float sample_rate);
int srack_patch_get_wave(const srack_patch* p, int module, float* samples, uint32_t cap, float* sample_rate);

/* SynthModule::set_input / disconnect_input / get_input. */
int srack_patch_connect(srack_patch* p, int src_module, int src_port, int sink_module, int sink_port);
int srack_patch_disconnect(srack_patch* p, int sink_module, int sink_port);
int srack_patch_get_input(const srack_patch* p, int sink_module, int sink_port, int* src_module /* -1 = None */, int* src_port);

/* plan_execution (synth.rs:128-212) driven as the workspace does (ui.rs:63-82): output = first
 * OutputModule in list order.  Writes the execution order (module indices) to `order` (capacity
 * `cap`, may be NULL) and returns its length.  Re-run automatically by render when the graph changed. */
int srack_patch_plan(srack_patch* p, int* order, int cap);
/* plan_execution(output, &all_modules, &mut plan) with an explicit, possibly shuffled module list —
 * what the reference's own test drives (synth.rs:561-568).  Does not affect later renders. */
int srack_patch_plan_list(srack_patch* p, int output, const int* all_modules, int n_all, int* order, int cap);
/* The scheduler edges phase 2 of the last plan removed (synth.rs:176-191): up to `cap` pairs
 * (from, module) meaning "`from` no longer waits for `module`"; returns the count. */
int srack_patch_removed_edges(srack_patch* p, int* pairs, int cap);
/* The wires that end up as block delays: every wire whose source runs after its sink in the plan, so
 * the sink reads the previous block's buffer.  Up to `cap` quadruples
 * (src_module, src_port, sink_module, sink_port); returns the count. */
int srack_patch_delayed_edges(srack_patch* p, int* quads, int cap);

/* ---- .srk rack files (scope table (f) rank 2) ------------------------------------------------- */
/* FileFormat{modules, connections, positions} (ui.rs:578-586) in rmp-serde 1.3.0's compact MessagePack form.
 * load = SynthModuleWorkspaceImpl::deserialize (ui.rs:116-135) against the host's AudioConfig: the module list comes
 * out in REVERSE file order (ui.rs:654-660), V0 variants migrate, saved buffers survive only at the same buffer_size,
 * connections with unknown ids or bad ports are dropped.  Every SynthModuleType variant of the reference loads.
 * save = serialize (ui.rs:98-114): writes at most `cap` bytes to `buf` (may be NULL) and the full size to *n_bytes.  The state
 * members written are the ones stored in the patch; with srack_patch_keep_state, after a render, they are the RUNNING state of
 * voice 0 (the app saves the rack as it plays; a rack file is one instance). */
int srack_patch_load_srk(const void* bytes, size_t n_bytes, uint32_t sample_rate, uint32_t buffer_size, uint32_t channels, srack_patch** out);
int srack_patch_save_srk(const srack_patch* p, void* buf, size_t cap, size_t* n_bytes);
/* SynthModule::get_id: the UUID string that keys a file's connection list.  Returns its length. */
int srack_patch_module_id(const srack_patch* p, int module, char* buf, size_t cap);
/* Workspace position of a module's window (FileFormat.positions); get returns 1 if the module has one, else 0. */
int srack_patch_set_module_position(srack_patch* p, int module, float x, float y);
int srack_patch_get_module_position(const srack_patch* p, int module, float* x, float* y);
/* Contents of one output buffer before the first tick (what a loaded file carries): `n` = buffer_size samples, or 0
 * for a fresh, zeroed buffer.  Only the sink of a broken feedback edge ever observes it. */
int srack_patch_set_output_buffer(srack_patch* p, int module, int port, const float* samples, uint32_t n);
/* SynthModule::get_output (synth.rs:243) as far as a host can observe it before the first tick: the block the patch holds for this
 * port — what srack_patch_set_output_buffer or a loaded file put there.  Copies up to `cap` samples, returns how many the port holds
 * (0: a fresh, zeroed buffer).  Err(()) for a bad port is SRACK_ERR_PORT. */
int srack_patch_get_output_buffer(const srack_patch* p, int module, int port, float* dst, uint32_t cap);
/* Noise modules (SRACK_MOD_NOISE).  With sm(x) = splitmix64's output function applied to x + 0x9E3779B97F4A7C15,
 *   base(module)  = sm(seed ^ sm(module))                       module = its index in the patch
 *   key(voice)    = sm(base ^ (first_voice + voice))            voice  = its index in this handle
 *   sample n      = ((sm(key + n * 0x9E3779B97F4A7C15) >> 40) * 2^-24 - 0.5) * 2.0
 * i.e. sample n is output n of a splitmix64 generator seeded with key; n counts the samples rendered since
 * srack_voices_configure.  Independent of chunking, of the render flags and of how voices are sharded: a rank that owns
 * the global voices [r*V, (r+1)*V) passes first_voice = r*V.  Defaults: seed 0, first_voice 0. */
int srack_patch_set_noise_seed(srack_patch* p, uint64_t seed, uint64_t first_voice);

/* ---- voices: N independent instances of the patch ----------------------------------------- */
/* Fix the number of voices (lanes) and drop any earlier per-voice data and device state. */
int srack_voices_configure(srack_patch* p, uint32_t n_voices);
/* Per-voice override of one field (the only concept with no reference counterpart: the reference
 * has one instance of each parameter).  `values` has n_voices entries, host memory. */
int srack_voices_set_field_f32(srack_patch* p, int module, int field, const float* values);
int srack_voices_set_field_f64(srack_patch* p, int module, int field, const double* values);

/* ---- a wave bank: every voice of a SampleModule its own recording --------------------------- */
/* The bank: `n_waves` waves laid back to back in `samples`; wave k has lengths[k] >= 0 samples (0: the reference's empty wave, which
 * plays 0.0) and the rate sample_rates[k].  Copied; any f32 is accepted.  n_waves == 0 removes the bank (pointers may be NULL).  A bank
 * does nothing until voices are assigned to it: the module's own wave (srack_patch_set_wave) and SRACK_SAMPLE_WAVE_SAMPLE_RATE stay as
 * they are, and a patch with a bank and no assignment renders the same bits through the same kernel as without one.  Setting a bank
 * drops the module's voice assignment (the voices play the own wave again, as after a srack_patch_set_wave of it).
 * get_wave_bank copies up to `cap` lengths and rates (either may be NULL) and returns n_waves; get_wave_bank_samples copies up to `cap`
 * samples of one wave and returns that wave's length.
 * The assignment: wave[v] in [0, n_waves), or SRACK_WAVE_OWN: that voice plays the module's own wave at the rate of the field (or its
 * per-voice override), exactly as without a bank.  A voice with wave[v] >= 0 renders what a one-voice patch renders after
 * srack_patch_set_wave(bank wave wave[v], its rate): the bank's rate replaces wave_sample_rate, and a per-voice override of that field
 * applies to the SRACK_WAVE_OWN voices only.  `wave` has n_voices entries; NULL clears the assignment.  A bad index (outside
 * [-1, n_waves), or >= 0 without a bank) is SRACK_ERR_INVALID and leaves the earlier assignment in place.
 * Changing the assignment loads a wave (WaveBox::load: new = true): the patch is re-flattened and the next render starts every voice
 * of that player at pos = 0, playing = false — also under srack_patch_keep_state, where everything else carries over.
 * srack_voices_configure drops assignments.  Rack files carry neither bank nor assignment (no counterpart in the reference).  A sharded
 * host sets the same bank on every rank and each rank's own voices' indices.
 * get_waves copies up to `cap` entries and returns n_voices, or 0 when no assignment is set. */
#define SRACK_WAVE_OWN (-1)
int srack_patch_set_wave_bank(srack_patch* p, int module, const float* samples, const int* lengths, const float* sample_rates, uint32_t n_waves);
int srack_patch_get_wave_bank(const srack_patch* p, int module, int* lengths, float* sample_rates, uint32_t cap);
int srack_patch_get_wave_bank_samples(const srack_patch* p, int module, int wave, float* samples, uint32_t cap);
int srack_voices_set_waves(srack_patch* p, int module, const int* wave);
int srack_voices_get_waves(const srack_patch* p, int module, int* wave, uint32_t cap);

/* ---- a sequence bank: every voice of a sequencer its own notes, pattern and length ----------- */
/* The bank: `n_sequences` sequences for a GridSequencerModule (C = 1) or a PatternSequencerModule (C = 8, its gate channels):
 *   states  : u8 [n_sequences][C][64]  SRACK_STEP_NONE / _ON / _HOLD, exactly srack_patch_set_step's `state`
 *   values  : u16 [n_sequences][64]    the grid sequencer's note index; NULL = all 0; ignored (may be NULL) for a pattern sequencer
 *   lengths : int [n_sequences]        1..64: what SRACK_GRIDSEQ_LENGTH / SRACK_PATSEQ_LENGTH is for the module's own sequence
 * Copied (and shared between copies of the graph); cells at or past a sequence's length are never played and are not kept: they read
 * back as SRACK_STEP_NONE, as does the value of a SRACK_STEP_NONE cell as 0.  n_sequences == 0 removes the bank (pointers may be NULL).
 * A bank does nothing until voices are assigned to it: the module's own cells (srack_patch_set_step) and *_LENGTH stay as they are, and
 * a patch with a bank and no assignment renders the same bits through the same kernel as without one.  Setting a bank drops the
 * module's voice assignment.  SRACK_ERR_INVALID, with the earlier bank and assignment left in place, for a module that is no
 * sequencer, a state outside 0..2, a length outside 1..64 and n_sequences > SRACK_MAX_SEQUENCES.
 * get_sequence_bank copies up to `cap` sequences (any pointer may be NULL) and returns n_sequences.
 * The assignment: seq[v] in [0, n_sequences), or SRACK_SEQ_OWN: that voice plays the module's own cells at *_LENGTH, exactly as without
 * a bank.  A voice with seq[v] >= 0 renders what a one-voice patch renders whose module holds that bank sequence's cells
 * (srack_patch_set_step) and length (*_LENGTH).  steps_per_octave stays the module's field (it can differ per voice on its own).
 * `seq` has n_voices entries; NULL clears the assignment.  A bad index (outside [-1, n_sequences), or >= 0 without a bank) is
 * SRACK_ERR_INVALID and leaves the earlier assignment in place; SRACK_ERR_STATE before srack_voices_configure.
 * An assignment is an edit of cells — what the reference's grid editor does — not a load: the patch is re-flattened like after
 * srack_patch_set_step, so by default the voices restart, and under srack_patch_keep_state current_step, both edge detectors and the
 * grid sequencer's held CV carry over per voice; a current_step at or past the voice's new length wraps to 0 on the next sample (the
 * sequencer's own rule).  This differs on purpose from the wave bank, where an assignment loads a wave.
 * srack_voices_configure drops assignments.  Rack files carry neither bank nor assignment (no counterpart in the reference).  A sharded
 * host sets the same bank on every rank and each rank's own voices' indices.
 * get_sequences copies up to `cap` entries and returns n_voices, or 0 when no assignment is set.
 * (`states` and `values` are declared as untyped pointers: they point at uint8_t and uint16_t arrays of the layouts above.) */
#define SRACK_SEQ_OWN (-1)
#define SRACK_MAX_SEQUENCES 65536
int srack_patch_set_sequence_bank(srack_patch* p, int module, const void* states, const void* values, const int* lengths, uint32_t n_sequences);
int srack_patch_get_sequence_bank(const srack_patch* p, int module, void* states, void* values, int* lengths, uint32_t cap);
int srack_voices_set_sequences(srack_patch* p, int module, const int* seq);
int srack_voices_get_sequences(const srack_patch* p, int module, int* seq, uint32_t cap);

/* ---- render (needs the GPU) ---------------------------------------------------------------- */
/* Number of distinct wires feeding the OutputModule's channels and, per channel, which plane of
 * `d_frames` it is (-1 = unconnected => silence).  P1/P2 wire both channels to one source => 1 plane. */
int srack_render_planes(srack_patch* p, int* channel_plane, int cap);

/* Offline render of `n_samples` ticks for every voice, continuing from the current voice state
 * (first call: the modules' initial state), like calling execute() ceil(n/B) times and keeping
 * the first n frames (main.rs:59-90).
 *   d_frames : device, f32 [planes][n_samples][n_voices]  (voice-minor: one wave store = 256 B)
 *              may be NULL (mix only).
 *   d_mix    : device, f32 [channels][n_samples] = sum over voices of the channel's frames
 *              (the N-voice generalisation of MonoMixerModule's gain-1 sum, mixer.rs:109-118);
 *              may be NULL.
 *   stream   : hipStream_t (NULL = default stream).  The call is asynchronous w.r.t. the host.  The library enqueues on the stream
 *              during the call and never touches it afterwards (a later call, edit or state read-back that depends on this call's
 *              work waits for an event of the library's own): the host may destroy the stream whenever it could for its own work.
 */
int srack_render(srack_patch* p, uint32_t n_samples, float* d_frames, float* d_mix,
                 uint32_t flags, void* stream);

/* srack_render plus per-voice statistics of the output, folded into d_stats (device, f64 [planes][SRACK_STAT_COUNT][n_voices], 8-byte
 * aligned) — for a host that wants one number per voice without writing and re-reading the frames.  For every sample x of plane p and
 * voice v (the f32 value the call writes, or would write, to d_frames): NaN / +-inf adds 1 to NONFINITE and nothing else; otherwise
 * SUM += (double)x, SUM_SQ += (double)x * x, PEAK_POS = max(PEAK_POS, x), PEAK_NEG = max(PEAK_NEG, -x), and |x| > 1 adds 1 to CLIPPED (a peak moves
 * only to a value strictly above it: from the zero fill, a peak of nothing is +0.0).
 * The call adds to what the buffer holds: zero-fill it once and the statistics cover every call since (tick sessions, segments, edits,
 * srack_patch_keep_state).  The sums are taken in sample order: bit for bit the sequential f64 loop, however the render is cut.
 * d_frames and d_mix may be NULL independently of d_stats (statistics only: no frames are written); d_stats NULL is srack_render.
 * Every voice kernel: the fused voice chains accumulate them in registers (no frames written when none are asked for); any other kernel's
 * frames — the host's, or one launch's worth of library scratch — are folded after each launch, in sample order as well.  Asking for
 * statistics changes neither the kernel, the chunks nor any bit of frames, mix or voice state.  A patch with no plane returns SRACK_OK
 * and leaves d_stats untouched. */
enum {
    SRACK_STAT_SUM = 0, SRACK_STAT_SUM_SQ = 1, SRACK_STAT_PEAK_POS = 2, SRACK_STAT_PEAK_NEG = 3,
    SRACK_STAT_NONFINITE = 4, SRACK_STAT_CLIPPED = 5, SRACK_STAT_COUNT = 6
};
int srack_render_stats(srack_patch* p, uint32_t n_samples, float* d_frames, float* d_mix,
                       double* d_stats, uint32_t flags, void* stream);

/* ---- mix buses: a gain and a bus per voice, one mix per bus ---------------------------------------------------
 * MonoMixerModule is `*dst += src * gain` with a gain per input (mixer.rs:110-117); d_mix above is its gain-1 sum over all voices.
 * The faithful N-voice generalisation has a gain per voice, and hosts group voices (chords, sweep values, left / right, data-set
 * items): every voice gets a gain and a bus, and a render fills one mix per bus — without the host writing, re-reading and reducing
 * the frames itself. */
#define SRACK_MAX_BUSES 65536
#define SRACK_BUS_NONE  (-1)

/* The mix table of the handle's voices.  Host memory, n_voices entries each, copied.
 *   bus  : bus[v] in [0, n_buses) or SRACK_BUS_NONE (the voice is in no bus); NULL = every voice in bus 0
 *   gain : any f32 (0, negative, non-finite included);                        NULL = 1.0f for every voice
 * 1 <= n_buses <= SRACK_MAX_BUSES; a bus may be empty.  SRACK_ERR_STATE before srack_voices_configure, SRACK_ERR_INVALID for a
 * bus index outside the range (the table set before stays).  srack_voices_configure drops the table.
 * The table is NOT part of the patch's program: setting or changing it between renders does not re-flatten, does not restart
 * the voices and changes no bit of frames, mix, statistics or voice state. */
int srack_voices_set_buses(srack_patch* p, uint32_t n_buses, const int* bus, const float* gain);
/* returns n_buses (0: no table set); copies up to cap entries of each (either pointer may be NULL) */
int srack_voices_get_buses(const srack_patch* p, int* bus, float* gain, uint32_t cap);
/* Diagnostics (tests, tools): how the table was laid out for the bus fold.  Voices are taken in tiles of 64; a SEGMENT is the voices of
 * one tile that share a bus.  Returns the number of segments and writes, for the first segment_cap of them in ascending (tile, bus)
 * order, four ints — tile, bus, the segment's row of the fold's scratch (-1: the bus's only segment, which needs none), voices — and
 * to `order` (up to order_cap entries) the voices segment after segment, each segment's in the order they are added.  Within a bus
 * the scratch rows ascend with the tile: that is the order the bus's segments are added in.  Either pointer may be NULL. */
int srack_voices_bus_plan(const srack_patch* p, int* segments, uint32_t segment_cap, int* order, uint32_t order_cap);

/* ---- voice bus slots: each voice in up to four buses, a gain per channel ---------------------------------------
 * The mix table generalised the way a console expects it: a voice feeds up to n_slots buses, each with a gain PER CHANNEL.  Pan is
 * one slot with different gains for Left and Right — in the reference two MonoMixerModules fed by the same wire, each with its own gain
 * per input (mixer.rs:106-119) — and costs no second plane; a per-voice send amount ("this voice dry, that one drenched") is a second
 * slot naming an aux bus.  Host memory, copied:
 *   bus  : [n_voices][n_slots], bus[v][k] in [0, n_buses) or SRACK_BUS_NONE;  NULL = slot 0 is bus 0, the other slots are none
 *   gain : [n_voices][n_slots][channels], any f32, copied bit for bit;         NULL = 1.0f
 * 1 <= n_slots <= SRACK_MAX_VOICE_SLOTS; `channels` is the channel count the patch was created with.  A voice may name the same bus
 * in several slots: there are then two terms.  Errors and lifetime follow srack_voices_set_buses: SRACK_ERR_STATE before
 * srack_voices_configure; SRACK_ERR_INVALID for a bad count or index, the earlier table (of either kind) left in place;
 * srack_voices_configure drops the table; another n_buses drops the console's stages, the same n_buses keeps them.  The table is not
 * part of the program: setting it re-flattens nothing, restarts nothing, changes no bit of frames, mix, statistics or voice state and
 * does not change which kernel renders.
 * There is ONE mix table per handle and the two setters replace each other; every console call that needs "a mix table" accepts either.
 * srack_voices_get_buses on a slot table returns n_buses and copies slot 0 and channel 0; srack_voices_get_bus_slots on a table set
 * through srack_voices_set_buses reports n_slots = 1 with the gain repeated per channel.  srack_voices_bus_plan on a slot table: a
 * segment's "tile" is the GROUP index tile * n_slots + slot, `order` holds real voice numbers; for n_slots == 1 the answer equals the
 * plan the same table gives through srack_voices_set_buses.  srack_render_info writes " buses=<n>[fold slots=<K>]".
 *
 * srack_render_buses with a slot table fills d_bus_mix as before.  For bus b and channel c with plane(c) >= 0 the terms are all (v, k)
 * with bus[v][k] == b, each term p = fl32(gain[v][k][c] * x[plane(c)][t][v]).  A GROUP is the terms of one (tile = v / 64, slot k),
 * voices ascending; a group's sum is its first product, then one f32 addition per further term, in order; the bus's sample is the first
 * group's sum, then one f32 addition per further group, in ascending (tile, slot).  IEEE f32, one rounding per operation, no fma, no
 * atomics.  A bus without terms is +0.0f, an unconnected channel is 0.  A non-finite gain or sample reaches the buses and channels it
 * is sent to, and no others.  The order depends on the table and the voice count alone — never on n_samples, on how the render is cut
 * or on what else the call is asked for.  With n_slots == 1 and equal gains across channels this is the definition of
 * srack_render_buses below word for word, and the bits are the same.  Each frame is read from device memory once per fold, whatever
 * n_slots and the channel count are. */
#define SRACK_MAX_VOICE_SLOTS 4
int srack_voices_set_bus_slots(srack_patch* p, uint32_t n_buses, uint32_t n_slots, const int* bus, const float* gain);
/* returns n_buses (0: no table set; *n_slots is then 0); copies up to cap VOICES of each (any pointer may be NULL) */
int srack_voices_get_bus_slots(const srack_patch* p, int* n_slots, int* bus, float* gain, uint32_t cap);

/* srack_render_stats plus the bus mixes:
 *   d_bus_mix : device, f32 [n_buses][channels][n_samples]
 *   d_bus_mix[b][c][t] = sum over the voices v with bus[v] == b of  fl32(gain[v] * x[plane(c)][t][v])
 * x is the f32 sample the call writes (or would write) to d_frames; channels map to planes as for d_mix (an unconnected
 * channel is 0); product and sum are IEEE f32 (a NaN or inf sample, or 0 * inf, makes that bus's sample non-finite and touches
 * no other bus); an empty bus is 0.  The call WRITES d_bus_mix (it does not add to it).
 * d_frames, d_mix, d_stats may each be NULL independently.  d_bus_mix NULL is srack_render_stats exactly.
 * SRACK_ERR_STATE if d_bus_mix is given and no table is set.
 * The order of the f32 additions is fixed by the table and the voice count (no floating-point atomics): within a tile of 64 voices a
 * bus's voices in ascending order, then the bus's tiles in ascending order.  So sample t of every bus has the same bits from run to
 * run, however the render is cut into calls, and whatever else the call is asked for.  Every voice kernel: each launch's frames —
 * the host's, or one launch's worth of library scratch — are folded right behind it.  Asking for bus mixes changes neither the
 * kernel, the chunks nor any bit of frames, mix, statistics or voice state.
 * Sharded: each rank sets the table of its own voices with GLOBAL bus numbers and the same n_buses, and the per-rank bus mixes are
 * summed by srack_dist_reduce_mix with count = n_buses * channels * n_samples. */
int srack_render_buses(srack_patch* p, uint32_t n_samples, float* d_frames, float* d_mix, double* d_stats,
                       float* d_bus_mix, uint32_t flags, void* stream);

/* ---- bus reverbs: a stereo Freeverb per mix bus, behind the mixer ------------------------------------------------
 * In real patches FreeverbModule sits behind the mixer, on the sum: the voices of a bus share one room.  Every bus may carry one
 * reverb.  The reverb of bus b renders what FreeverbModule renders (SRACK_MOD_FREEVERB above: the freeverb crate restated, f64, one
 * rounding per operation), configured by the module's six parameters and ticked once per sample with
 *   in0 = (double)bus_mix[b][0][t],  in1 = (double)bus_mix[b][1][t]  (0.0 for a patch of one channel: the module with Right
 *   unconnected; channels beyond the second are ignored),            fx[b][0][t] = (float)out0,  fx[b][1][t] = (float)out1.
 * A patch whose sample rate is below 784 Hz has no Freeverb (SRACK_ERR_UNSUPPORTED, as for the module).
 *
 * set_reverb: params is f64 [n_buses][SRACK_FREEVERB__NFIELDS] in the module's field order (DAMPENING, FREEZE, WET, WIDTH, ROOM_SIZE,
 * DRY), NULL = the module's defaults (0.5, 0, 1, 0.5, 0.5, 0) for every bus; ANY f64 is accepted, as the reference accepts any (a NaN
 * parameter makes that bus's output NaN and touches no other bus); FREEZE is zero or non-zero.  enabled is int [n_buses], zero = the
 * bus has no reverb, NULL = every bus has one.  A bus without a reverb costs no state; its fx rows are the bus mix's channels 0 and 1,
 * copied (channel 1 zeros for a patch of one channel).
 * Calling it again is the reference's slider (set_freeverb(false)): the coefficients change, delay lines and filter states stay.  A
 * bus enabled later starts with a fresh reverb (zeroed lines); disabling a bus drops its state.
 * The reverbs are NOT part of the patch's program: setting, changing or ticking them does not re-flatten, restarts nothing, changes no
 * bit of frames, mix, statistics, bus mixes or voice state and not the kernel a patch renders with; they carry on across an edit that
 * re-flattens the patch.  srack_voices_configure drops parameters and state; so does srack_voices_set_buses with another n_buses
 * (with the same n_buses both stay).  Rack files carry nothing of this (no counterpart in the reference).
 * SRACK_ERR_INVALID for a null handle; SRACK_ERR_STATE for any of the five calls before srack_voices_configure or before a mix table
 * exists, and for srack_buses_reverb / srack_buses_reset_reverb before srack_buses_set_reverb.  A failed call leaves the earlier
 * setting in place.
 * get_reverb copies up to cap buses (either pointer may be NULL) and returns n_buses, or 0 when no reverbs are set.
 * reset_reverb: delay lines and filter states to zero, the sample counter to 0; the parameters stay.
 * reverb_plan (diagnostics: tests, tools): the 24 line lengths at the patch's sample rate — line = 2 * unit + channel, units 0..7 the
 * combs, 8..11 the allpasses; (uint32_t)(tuning * sample_rate / 44100.0), the right channel's tuning the left's plus 23 — and the number
 * of samples the kernel takes at a time, min(256, shortest line).  Either pointer may be NULL.
 *
 * srack_buses_reverb is an entry of its own, not one more pointer on srack_render_buses: it runs on whatever bus mix the host hands it.
 * A sharded host reduces the per-rank bus mixes first (srack_dist_reduce_mix) and reverberates on the root — the reverb of a sum is
 * not, bit for bit, the sum of reverbs.
 *   d_bus_mix : device, f32 [n_buses][channels][n_samples]      (what srack_render_buses writes)
 *   d_bus_fx  : device, f32 [n_buses][2][n_samples], written; must not overlap d_bus_mix (SRACK_ERR_INVALID)
 *   stream    : as for srack_render: asynchronous, and the library touches the stream only during the call.
 * One sample counter per handle counts the samples processed since the last reset; every line's position is counter mod length, so
 * the result does not depend on how the samples are cut into calls (a fresh reverb is all zeros, whatever its position: one counter
 * serves reverbs enabled at different times).  State per enabled bus: 16 filter states and the 24 lines in f64 on the device (about
 * 220 KB at 48 kHz), allocated at the first call that needs it; SRACK_ERR_NOMEM if that fails.  The kernel takes a workgroup per bus
 * and min(256, shortest line) samples at a time (csrc/busfx.hip.h).  srack_render_info says " busfx=<enabled>[block <T>]" once a call has run. */
int srack_buses_set_reverb(srack_patch* p, const double* params, const int* enabled);
int srack_buses_get_reverb(const srack_patch* p, double* params, int* enabled, uint32_t cap);
int srack_buses_reset_reverb(srack_patch* p);
int srack_buses_reverb_plan(const srack_patch* p, int* line_lengths, int* block);
int srack_buses_reverb(srack_patch* p, uint32_t n_samples, const float* d_bus_mix, float* d_bus_fx, void* stream);

/* ---- master section: a gain per bus and channel, one stereo sum over the buses, its statistics -------------------
 * MonoMixerModule behind the effects (mixer.rs:106-119: output.fill(0.0); *dst += src * gain, one gain per input), generalised to
 * N buses: a host with thousands of buses wants one stereo pair, not f32 [n_buses][2][T] to read back and add up itself.
 *   master[c][t] = sum over the buses b of  fl32(gain[b][c] * rows[b][c][t]),   c = 0, 1
 * Product and sum are IEEE f32, one rounding per operation, no fma.  ANY f32 gain is accepted, the reference's way: 0 * inf is NaN; a
 * non-finite sample or gain makes that channel's sample non-finite and touches nothing else.
 *
 * The order of the additions is part of the ABI.  It depends on n_buses alone — never on n_samples, on how a render is cut into
 * calls, or on what else the call is asked for:
 *   run r    = ((+0.0f + p[64r]) + p[64r+1]) + ...   over its up to SRACK_MASTER_RUN buses, ascending   (p[b] the product of bus b)
 *   block k  = +0.0f plus its up to SRACK_MASTER_BLOCK run sums, ascending
 *   master   = +0.0f plus the up to 16 block sums, ascending
 * Up to 64 buses that is MonoMixerModule's loop exactly; up to 65 it coincides with the plain sequential sum, from 66 on it does not.
 *
 * set_master: gain is host memory, f32 [n_buses][2] (channel 0, channel 1 of every bus), copied bit for bit; NULL = 1.0f everywhere.
 * get_master copies up to cap buses (gain may be NULL) and returns n_buses, or 0 when no gains are set.  Before set_master the master
 * runs with every gain 1.0f.
 * The gains belong to the handle, NOT to the patch's program: setting or changing them, or running the master, does not re-flatten,
 * restarts nothing, changes no bit of frames, mix, statistics, bus mixes, fx or voice state and not the kernel a patch renders with;
 * they survive an edit that re-flattens the patch.  srack_voices_configure drops them; so does srack_voices_set_buses with another
 * n_buses (the same n_buses keeps them).  Rack files carry nothing of this.
 *
 * The master call:
 *   d_rows         : device, f32 [n_buses][row_channels][n_samples] — what srack_buses_reverb writes (row_channels = 2) or what
 *                    srack_render_buses writes (row_channels = the patch's channels).  1 <= row_channels <= 8; channels 0 and 1 are
 *                    used, channels beyond the second are ignored (the reverb's convention).  Any 4-byte aligned address; rows that
 *                    are 16-byte aligned (the base is, and n_samples % 4 == 0) are read four samples at a time.
 *   d_master       : device, f32 [2][n_samples], written; must not overlap d_rows (SRACK_ERR_INVALID).  With row_channels == 1,
 *                    d_master[1] is +0.0f throughout and no product is taken for it.
 *   d_master_stats : device, f64 [2][SRACK_STAT_COUNT], 8-byte aligned, or NULL.  The per-voice definitions of the statistics above,
 *                    applied to the f32 master sample the call writes: NaN / +-inf adds 1 to NONFINITE and nothing else; otherwise
 *                    SUM, SUM_SQ, PEAK_POS, PEAK_NEG and CLIPPED (|x| > 1) are updated as there.  The call adds to what the buffer
 *                    holds; SUM and SUM_SQ are taken in sample order: bit for bit the sequential f64 loop, however the samples are
 *                    cut into calls.  With row_channels == 1 channel 1's row is left untouched.
 *   stream         : as for srack_render: asynchronous, and the library touches the stream only during the call.
 * Errors, in this order: SRACK_ERR_INVALID for a null handle; SRACK_ERR_STATE before srack_voices_configure or before a mix table
 * exists (all three calls); n_samples == 0 is SRACK_OK and touches nothing; SRACK_ERR_INVALID for a null d_rows or d_master,
 * row_channels outside 1..8, a misaligned d_master_stats or an overlap.  A failed set_master leaves the earlier gains in place.
 * The run sums pass through scratch of the handle's, f32 [runs][2][n_samples] (1/64 of the input), grown on demand: SRACK_ERR_NOMEM
 * if that fails, the earlier state intact.  No floating-point atomics (csrc/master.hip.h).  A sharded host reduces the per-rank bus
 * mixes first, reverberates on the root and takes the master there: a sum of per-rank masters has another association and other bits.
 * srack_render_info says " master=<n_buses>[<runs> runs]" once a master call has run. */
#define SRACK_MASTER_RUN   64   /* buses per run   (level 1) */
#define SRACK_MASTER_BLOCK 64   /* runs per block  (level 2): 4096 buses; at most 16 blocks (level 3) */
int srack_buses_set_master(srack_patch* p, const float* gain);
int srack_buses_get_master(const srack_patch* p, float* gain, uint32_t cap);
int srack_buses_master(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels,
                       float* d_master, double* d_master_stats, void* stream);

/* ---- bus sends: aux sends from bus to bus, one gather-sum per destination bus ------------------------------------
 * MonoMixerModule (mixer.rs:106-119: output.fill(0.0); *dst += src * gain) in front of every bus, with as many inputs as the bus has
 * feeders: a host with thousands of group buses wants a handful of aux buses that carry the rooms, every group bus sending some of
 * its signal there, and not f32 [n_buses][channels][T] to read back and mix itself.
 * The sends are a list of n_sends triples (src[i], dst[i], gain[i][2]), and there is a through gain through[b][2] per bus.  For every
 * destination bus d the terms are: term 0 = (d, through[d]); then the sends i with dst[i] == d, in ascending i — a stable grouping of
 * the host's list, which need not be sorted.  Each term is
 *   p_k = fl32(g_k[c] * rows[src_k][c][t]),   c = 0, 1
 * and out[d][c][t] is the master section's three-level tree over p_0 .. p_{n-1}:
 *   run r    = ((+0.0f + p[64r]) + p[64r+1]) + ...   over its up to SRACK_MASTER_RUN terms, ascending
 *   block k  = +0.0f plus its up to SRACK_MASTER_BLOCK run sums, ascending
 *   out      = +0.0f plus the up to 16 block sums, ascending
 * Product and sum are IEEE f32, one rounding per operation, no fma.  The order of the additions is part of the ABI.  It depends on
 * the send list alone — never on n_samples or on how the samples are cut into calls.  Up to 64 terms it is MonoMixerModule's loop
 * exactly; a bus with no sends is +0.0f + p_0: its row times the through gain, -0.0 becoming +0.0.  (A run sum is never -0.0, so a
 * level with a single addend changes no bit.)
 * Sends read the input rows only, never the output: one call is one level of routing, a chain of sends is two calls.  src == dst is
 * allowed (a second gain on the bus's own row), so are duplicate pairs, and ANY f32 gain, the reference's way: 0 * inf is NaN; a
 * non-finite sample or gain reaches the destinations it is sent to and no others.
 * Limits: n_sends <= SRACK_MAX_SENDS; a destination has at most 65536 terms, the through term included — the tree's capacity.
 *
 * set_sends: src, dst (int [n_sends]), gain (f32 [n_sends][2], NULL = 1.0f) and through (f32 [n_buses][2], NULL = 1.0f) are host
 * memory, the gains copied bit for bit.  n_sends == 0 removes the sends (the pointers may be NULL, through is ignored).
 * SRACK_ERR_INVALID — the earlier sends staying in place — for n_sends > SRACK_MAX_SENDS, a null src or dst with n_sends > 0, an index
 * outside [0, n_buses), a destination with more than 65535 sends.
 * get_sends copies up to cap sends and up to through_cap buses (any pointer may be NULL) and returns n_sends, or 0 when none are set.
 * send_plan: how the list is laid out — n_terms[b] the terms of bus b (through term included; up to bus_cap buses), order the send
 * indices grouped by destination ascending, a destination's in the order they are added (up to order_cap) — and returns the number
 * of runs, the sum over the buses of ceil(n_terms / SRACK_MASTER_RUN); 0 when no sends are set.
 * The sends belong to the handle, NOT to the patch's program, exactly as the master's gains: setting, changing or running them does
 * not re-flatten, restarts nothing, changes no bit of frames, mix, statistics, bus mixes, fx, master or voice state and not the kernel
 * a patch renders with; they survive an edit that re-flattens the patch.  srack_voices_configure drops them; so does
 * srack_voices_set_buses with another n_buses (the same n_buses keeps them).  Rack files carry nothing of this.
 *
 * The send call:
 *   d_rows : device, f32 [n_buses][row_channels][n_samples] — what srack_render_buses writes.  1 <= row_channels <= 8; channels 0
 *            and 1 are mixed, channels beyond the second are neither read nor written.  Any 4-byte aligned address; rows that are
 *            16-byte aligned (both bases are, and n_samples % 4 == 0) are read four samples at a time.
 *   d_out  : device, the same shape, written — every bus's row, a bus without sends included; srack_buses_reverb (row_channels = the
 *            patch's channels) and srack_buses_master take it.  Must not overlap d_rows (SRACK_ERR_INVALID).
 *   stream : as for srack_render: asynchronous, and the library touches the stream only during the call.
 * Errors, in this order: SRACK_ERR_INVALID for a null handle; SRACK_ERR_STATE before srack_voices_configure or before a mix table
 * exists (all four calls); SRACK_ERR_STATE for the send call before set_sends; n_samples == 0 is SRACK_OK and touches nothing;
 * SRACK_ERR_INVALID for a null d_rows or d_out, row_channels outside 1..8 or an overlap.
 * The run sums of the destinations of more than one run pass through scratch of the handle's, grown on demand: SRACK_ERR_NOMEM if that
 * fails, the earlier state intact.  No floating-point atomics, every output float is written once (csrc/sends.hip.h).  A sharded host
 * reduces the per-rank bus mixes first (srack_dist_reduce_mix) and sends on the root: a sum of per-rank sends has another association
 * and other bits.  srack_render_info says " sends=<n_sends>[<runs> runs]" behind " buses=" once a send call has run. */
#define SRACK_MAX_SENDS 1048576
int srack_buses_set_sends(srack_patch* p, uint32_t n_sends, const int* src, const int* dst,
                          const float* gain, const float* through);
int srack_buses_get_sends(const srack_patch* p, int* src, int* dst, float* gain, uint32_t cap,
                          float* through, uint32_t through_cap);
int srack_buses_send_plan(const srack_patch* p, int* n_terms, uint32_t bus_cap, int* order, uint32_t order_cap);
int srack_buses_send(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels,
                     float* d_out, void* stream);

/* ---- the bus filters: a Moog ladder per mix bus, behind the mixer ---------------------------------------------------
 * The one processor a console strip has besides level, sends and a room: a filter on the bus.  Channel c (0 or 1) of an enabled bus b
 * is one MoogFilterModule (filter.rs:182-221 with InternalMoogFilterState::calc and clamp_buffers, filter.rs:58-92): its three
 * sliders are the bus's params, its Audio input d_rows[b][c][t], its CV input d_cv[b][t]; it is ticked once per sample and writes the
 * chosen port to d_out[b][c][t].  The two channels of a bus are two modules with the same sliders and the same CV, each with its own
 * state.  A ladder on the sum is not the sum of ladders (the cubic and the clamps are non-linear), so this is not what a filter in
 * every voice gives.  Every operation is IEEE f32, one rounding each, in the reference's order: no fma, the clamps the literal
 * min-then-max (a NaN state clamps to +1.0, the reference's way); the coefficients are recomputed only when the clamped
 * (frequency, res) differs from the pair they were computed for — the reference's quirk included that a fresh filter at frequency 0
 * and resonance 0 never computes them.  State starts at all zeros (Default).  ANY f32 parameter is accepted, as the reference accepts
 * any; a non-finite sample, CV or parameter affects that bus's rows and no other.
 *
 * params: f32 [n_buses][SRACK_BUS_FILTER_NPARAMS] = FREQ, RES, EXP_AMT (SRACK_VCF_FREQ .. SRACK_VCF_EXP_AMT); NULL = the module's defaults 0.2f, 0.5f, 0.5f
 * port:   int [n_buses], SRACK_VCF_OUT_LOWPASS / _BANDPASS / _HIGHPASS: which of the module's three outputs the bus takes; NULL = lowpass
 * enabled: int [n_buses], zero = no filter on that bus; NULL = every bus
 * All three are host memory.  A port outside 0..2 is SRACK_ERR_INVALID and leaves the earlier setting in place.
 * Lifecycle (the reverbs' rules): calling set_filter again is the slider — parameters change, state stays.  A bus enabled later
 * starts from zeros; disabling a bus drops its state.  reset_filter zeroes every state and keeps the parameters.  get_filter copies up
 * to cap buses (any pointer may be NULL) and returns n_buses, or 0 when no filters are set.  filter_state waits for the last filter
 * call and copies up to cap buses of state — per bus and channel the ten values SRACK_VCF_ST_F .. SRACK_VCF_ST_RES, a disabled bus as
 * zeros — and returns n_buses.  The state lives on the device between calls: the result cannot depend on how the samples are cut
 * into calls.
 * The filters belong to the handle, NOT to the patch's program, exactly as the reverbs: setting, changing or running them does not
 * re-flatten, restarts nothing, changes no bit of frames, mix, statistics, bus mixes, sends, fx, master or voice state and not the
 * kernel a patch renders with; they survive an edit that re-flattens the patch.  srack_voices_configure drops them; so does
 * srack_voices_set_buses with another n_buses (the same n_buses keeps them).  Rack files carry nothing of this.
 *
 * The filter call:
 *   d_rows : device, f32 [n_buses][row_channels][n_samples] — what srack_render_buses or srack_buses_send writes.
 *            1 <= row_channels <= 8; channels 0 and 1 are filtered, channels beyond the second are neither read nor written.
 *   d_cv   : device, f32 [n_buses][n_samples], one CV per bus, shared by its channels; NULL = the CV port is unconnected:
 *            cv = 0.0f, the arithmetic freq + 0.0f * exp_amt still carried out, as the reference does.
 *   d_out  : device, the shape of d_rows, written: d_rows itself (in place) or disjoint from it; a partial overlap is
 *            SRACK_ERR_INVALID, and so is d_cv overlapping d_out.  A disabled bus's channels 0 and 1 are copied bit for bit (-0.0
 *            stays -0.0); in place they are left alone.  A disabled bus costs no state.
 *   Any 4-byte aligned address is accepted for all three.
 *   stream : as for srack_render: asynchronous, and the library touches the stream only during the call.
 * Errors, in this order: SRACK_ERR_INVALID for a null handle; SRACK_ERR_STATE before srack_voices_configure or before a mix table
 * exists (all five calls); SRACK_ERR_STATE for srack_buses_filter, reset_filter and filter_state before set_filter; n_samples == 0 is
 * SRACK_OK and touches nothing; SRACK_ERR_INVALID for a null d_rows or d_out, row_channels outside 1..8 or an overlap as above;
 * SRACK_ERR_NOMEM if the state cannot be allocated, the earlier state intact.
 * The kernel takes a lane per (enabled bus, channel) row — the ladder is serial in time — and one wave per workgroup; tiles of 64 rows
 * x 64 samples pass through LDS so that memory is touched in whole lines (csrc/busvcf.hip.h).  Until every SIMD has a wave (32 768
 * stereo buses) the call's time is set by one row's dependency chain, not by the number of buses.  srack_render_info says
 * " busvcf=<enabled buses>[<waves> waves]" between " sends=" and " busfx=" once a filter call has run. */
#define SRACK_BUS_FILTER_NPARAMS 3
#define SRACK_BUS_FILTER_NSTATE  10   /* SRACK_VCF_ST_F .. SRACK_VCF_ST_RES, index = field - SRACK_VCF_ST_F */
int srack_buses_set_filter(srack_patch* p, const float* params, const int* port, const int* enabled);
int srack_buses_get_filter(const srack_patch* p, float* params, int* port, int* enabled, uint32_t cap);
int srack_buses_reset_filter(srack_patch* p);
int srack_buses_filter_state(srack_patch* p, float* state /* host, f32 [n_buses][2][SRACK_BUS_FILTER_NSTATE] */, uint32_t cap);
int srack_buses_filter(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels,
                       const float* d_cv, float* d_out, void* stream);

/* ---- the bus VCAs: an ADSR and a VCA per mix bus, behind the mixer, driven by a gate or CV row ------------------------------------
 * What moves a strip's level in time.  Every bus has one control row d_ctl[b][t] and a mode:
 *   SRACK_BUS_VCA_GATE  the row is the Gate input of one ADSRModule (adsr.rs:134-217) with the sliders params[b]; the envelope is the
 *                       CV of one VCAModule (vca.rs:117-148) per channel c in {0, 1}: Audio input d_rows[b][c][t], flag negative[b],
 *                       output d_out[b][c][t] — the pair every patch of the reference ends in (patch P1 wires exactly that).
 *   SRACK_BUS_VCA_CV    no ADSR and no state: the row is the VCAs' CV itself (automation).
 *   SRACK_BUS_VCA_OFF   the bus passes.
 * Every operation is IEEE f32, one rounding each, in the reference's order, no fma: the envelope is adsr.rs's literal sequence
 * (a_sec = 0 gives an increment of +inf: Attack lasts one sample; a NaN gate is neither high nor low), the VCA is
 * negative || cv > 0 ? audio * cv : +0.0f.  The ADSR's sample rate is the f32 a fresh ADSR module of this patch carries
 * (SRACK_ADSR_SAMPLE_RATE).  ANY f32 slider is accepted; a non-finite sample, control value or slider affects that bus's rows and no
 * other.  Fresh state is NOT all zeros: phase 0, mode SRACK_ADSR_MODE_NONE, r_val 0, from_a_val 0, TransitionDetector.last TRUE.
 *
 * params:   f32 [n_buses][SRACK_BUS_VCA_NPARAMS] = A_SEC, D_SEC, S_VAL, R_SEC (SRACK_ADSR_A_SEC .. SRACK_ADSR_R_SEC); NULL = the module's
 *           defaults 0, 0.5, 0.25, 0.5
 * mode:     int [n_buses], SRACK_BUS_VCA_*; NULL = every bus GATE
 * negative: int [n_buses], non-zero = the VCAs' `negative` flag; NULL = false
 * All three are host memory.  A mode outside 0..2 is SRACK_ERR_INVALID and leaves the earlier setting in place.
 * Lifecycle (the filters' rules): calling set_vca again is the slider — sliders, flags change, state stays.  A bus that becomes GATE
 * starts fresh; a bus that leaves GATE drops its state.  reset_vca makes every state fresh and keeps the setting.  get_vca copies up to
 * cap buses (any pointer may be NULL) and returns n_buses, or 0 when no VCAs are set.  vca_state waits for the last call and copies
 * up to cap buses of state — per bus the six values SRACK_ADSR_PHASE .. SRACK_ADSR_GATE_LAST as f32: mode and last as their small
 * integers, the sample-rate slot the f32 rate; a bus that is not GATE reads as the fresh state (0, 4, 0, 0, rate, 1) — and returns
 * n_buses.  The state lives on the device between calls: the result cannot depend on how the samples are cut into calls.
 * The VCAs belong to the handle, NOT to the patch's program, exactly as the filters: setting, changing or running them does not
 * re-flatten, restarts nothing, changes no bit of frames, mix, statistics, bus mixes, sends, filters, fx, master or voice state;
 * they survive an edit that re-flattens the patch.  srack_voices_configure drops them; so does srack_voices_set_buses with another
 * n_buses (the same n_buses keeps them).  Rack files carry nothing of this.
 *
 * The call:
 *   d_rows : device, f32 [n_buses][row_channels][n_samples] — what srack_render_buses, srack_buses_send or srack_buses_filter writes.
 *            1 <= row_channels <= 8; channels 0 and 1 are processed, channels beyond the second are neither read nor written.
 *   d_ctl  : device, f32 [n_buses][n_samples], or NULL = the control port is unconnected: a GATE bus runs its ADSR with no gate
 *            (gate_in_buf is None: Sustain falls to Release, mode None stays None), a CV bus writes +0.0f (output.fill(0.0)).
 *   d_out  : device, the shape of d_rows, written: d_rows itself (in place) or disjoint from it.  An OFF bus's channels 0 and 1 are
 *            copied as 32-bit words (-0.0 stays -0.0, a NaN keeps its payload); in place they are left alone.
 *   d_env  : device, f32 [n_buses][n_samples], written, or NULL: a GATE bus's envelope, a CV bus's control row word for word (+0.0
 *            when d_ctl is NULL), +0.0 for an OFF bus — e.g. to sweep the bus filters with the same gate through
 *            srack_buses_filter's d_cv.  What d_out gets does not depend on whether d_env is given.
 *   d_env and d_ctl must not overlap d_out or each other, d_env must not overlap d_rows; those, and a partial overlap of d_rows and
 *   d_out, are SRACK_ERR_INVALID.  Any 4-byte aligned address is accepted for all four.
 *   stream : as for srack_render: asynchronous, and the library touches the stream only during the call.
 * Errors, in this order: SRACK_ERR_INVALID for a null handle; SRACK_ERR_STATE before srack_voices_configure or before a mix table
 * exists (all five calls); SRACK_ERR_STATE for srack_buses_vca, reset_vca and vca_state before set_vca; n_samples == 0 is SRACK_OK
 * and touches nothing; SRACK_ERR_INVALID for a null d_rows or d_out, row_channels outside 1..8 or an overlap as above;
 * SRACK_ERR_NOMEM if state and table cannot be allocated.
 * The kernel takes a workgroup of eight waves per 64 buses: the envelopes — serial in time — a lane per bus on the first wave, a tile
 * of 64 buses x 64 control samples turned through LDS; the VCAs elementwise on all eight waves, lanes on time (csrc/busvca.hip.h).  A
 * workgroup without a GATE bus is a plain streaming pass.  srack_render_info says " busvca=<buses not OFF>[<GATE buses> gated]"
 * between " busvcf=" and " busfx=" once a call has run. */
#define SRACK_BUS_VCA_NPARAMS 4   /* SRACK_ADSR_A_SEC .. SRACK_ADSR_R_SEC */
#define SRACK_BUS_VCA_NSTATE  6   /* SRACK_ADSR_PHASE .. SRACK_ADSR_GATE_LAST, index = field - SRACK_ADSR_PHASE */
enum { SRACK_BUS_VCA_OFF = 0, SRACK_BUS_VCA_CV = 1, SRACK_BUS_VCA_GATE = 2 };
int srack_buses_set_vca(srack_patch* p, const float* params, const int* mode, const int* negative);
int srack_buses_get_vca(const srack_patch* p, float* params, int* mode, int* negative, uint32_t cap);
int srack_buses_reset_vca(srack_patch* p);
int srack_buses_vca_state(srack_patch* p, float* state /* host, f32 [n_buses][SRACK_BUS_VCA_NSTATE] */, uint32_t cap);
int srack_buses_vca(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels,
                    const float* d_ctl, float* d_out, float* d_env, void* stream);

/* ---- the bus oscillators: an LFO per mix bus writes the console's control rows -------------------------------------------------------
 * What makes the rows that move a strip: the filters' d_cv, the VCAs' d_ctl (a gate or a CV), the shapers' d_cv — sweeps, tremolos and
 * gate clocks made on the device instead of uploaded.  On the samples of a call every enabled bus runs three reference modules in
 * series, ticked once per sample:
 *   OscillatorModule       (oscillator.rs:108-157) CV = d_cv[b][t], Sync = d_sync[b][t]; val = VAL, antialiasing[b]; output port[b]
 *   MathModule(Multiply)   In1 = that output, In2 unconnected, constant = DEPTH   (math.rs:150-155: a * constant)
 *   MathModule(Add)        In1 = that product, In2 unconnected, constant = OFFSET -> d_out[b][t]
 * The oscillator is the reference's own operation sequence, whatever mode the patch renders in (the console has no approximations):
 * pos += delta; pos %= 1.0 in f64; delta = 440 * 2^(f64(cv) + f64(val)) / f64(sample_rate) with the host libm's pow; the sine
 * (pos * PI * 2.0).sin() as f32 with the host libm's sin; square and saw with poly_blep in f64 as spelled; the TransitionDetector on
 * sync > 0.0, its `last` starting TRUE (a sync row whose first sample is high resets nothing).  The two Math operations are IEEE f32,
 * one rounding each, no fma, and they ALWAYS run: with the defaults DEPTH 1 and OFFSET 0 a -0.0 of the oscillator comes out as +0.0
 * (-0.0 * 1 = -0.0, -0.0 + 0.0 = +0.0), as the modules would make it.
 * d_cv == NULL: the CV port is unconnected (2^f64(val)) — the same bits as a row of +0.0f.  d_sync == NULL: sync_val = 0.0, never a
 * transition, and `last` becomes false.  ANY f32 is accepted for VAL, DEPTH, OFFSET and the rows; a non-finite value affects that bus's
 * row and no other.  The sample rate is the patch's, as f64.
 *
 * params:       f32 [n_buses][SRACK_BUS_OSC_NPARAMS] = VAL, DEPTH, OFFSET; NULL = 0, 1, 0
 * port:         int [n_buses], SRACK_OSC_OUT_*; NULL = Sine.  A port outside 0..2 is SRACK_ERR_INVALID and leaves the earlier setting
 *               in place.
 * antialiasing: int [n_buses], non-zero = true; NULL = true
 * enabled:      int [n_buses], non-zero = the bus has an oscillator; NULL = all
 * All four are host memory.
 * Lifecycle (the VCAs' rules): calling set_osc again is the slider — parameters, ports and flags change, state stays.  A bus that
 * becomes enabled starts fresh; a bus that leaves drops its state.  get_osc copies up to cap buses (any pointer may be NULL) and returns
 * n_buses, or 0 when no oscillators are set.  reset_osc(NULL) makes every state fresh — phase 0.0, last TRUE, as OscillatorModule::new —
 * and keeps the setting; reset_osc(pos) with pos f64 [n_buses] (host) starts bus b at phase pos[b], the phase a rack file would carry:
 * quadrature LFOs, a spread per strip.  Every pos[b] must be in [0, 1): anything else — NaN, 1.0, a negative number, and -0.0, which no
 * `pos %= 1.0` of non-negative numbers produces and whose wrap is not +0.0's — is SRACK_ERR_INVALID, and nothing is reset.  osc_state
 * waits for the last call and copies up to cap buses of state — per bus SRACK_OSC_POS and SRACK_OSC_SYNC_LAST (0.0 / 1.0) as f64; a
 * disabled bus reads fresh (0.0, 1.0) — and returns n_buses.  The state lives on the device between calls: no bit depends on how the
 * samples are cut into calls (the held-CV cache of the kernel is not state: every call starts with it empty).
 * The oscillators belong to the handle, NOT to the patch's program, exactly as the VCAs: setting, changing or running them does not
 * re-flatten, restarts nothing and changes no bit of any other output; they survive an edit that re-flattens the patch.
 * srack_voices_configure drops them; so does srack_voices_set_buses with another n_buses (the same n_buses keeps them).  Rack files
 * carry nothing of this.
 *
 * The call:
 *   d_cv   : device, f32 [n_buses][n_samples], or NULL
 *   d_sync : device, f32 [n_buses][n_samples], or NULL
 *   d_out  : device, f32 [n_buses][n_samples], written: the shape of srack_buses_filter's d_cv, srack_buses_vca's d_ctl and
 *            srack_buses_shaper's d_cv.  A disabled bus's row is written as +0.0f, the convention of srack_buses_vca's d_env.
 *   d_out must not overlap d_cv or d_sync (SRACK_ERR_INVALID).  Any 4-byte aligned address is accepted for all three.
 *   stream : as for srack_buses_vca: asynchronous, and the library touches the stream only during the call.
 * Errors, in this order: SRACK_ERR_INVALID for a null handle; SRACK_ERR_STATE before srack_voices_configure or before a mix table
 * exists (all five calls); SRACK_ERR_STATE for srack_buses_osc, reset_osc and osc_state before set_osc; n_samples == 0 is SRACK_OK and
 * touches nothing; SRACK_ERR_INVALID for a null d_out or an overlap as above; SRACK_ERR_NOMEM if state and table cannot be allocated.
 * The kernel takes a lane per enabled bus, a wave of 64 buses per workgroup, tiles of 64 buses x 64 samples of the CV and sync rows
 * turned through LDS, the state in registers for the call (csrc/busosc.hip.h); without a CV row the increment is computed once per bus
 * on the host.  srack_render_info says " busosc=<enabled>[<cv|-><sync|->]" in front of " busvcf=" once a call has run. */
#define SRACK_BUS_OSC_NPARAMS 3
enum { SRACK_BUS_OSC_VAL = 0, SRACK_BUS_OSC_DEPTH = 1, SRACK_BUS_OSC_OFFSET = 2 };
#define SRACK_BUS_OSC_NSTATE 2   /* SRACK_OSC_POS, SRACK_OSC_SYNC_LAST (0.0 / 1.0), as f64 */
int srack_buses_set_osc(srack_patch* p, const float* params, const int* port, const int* antialiasing, const int* enabled);
int srack_buses_get_osc(const srack_patch* p, float* params, int* port, int* antialiasing, int* enabled, uint32_t cap);
int srack_buses_reset_osc(srack_patch* p, const double* pos);
int srack_buses_osc_state(srack_patch* p, double* state /* host, f64 [n_buses][2] */, uint32_t cap);
int srack_buses_osc(srack_patch* p, uint32_t n_samples, const float* d_cv, const float* d_sync, float* d_out, void* stream);

/* ---- the bus shapers: a drive, a waveshaper and a make-up gain per mix bus, behind the mixer ---------------------------------------
 * The non-linearity of a strip: saturating a drum group, expanding an aux bus, riding the curve from an automation row.  A shaper on
 * the sum is not the sum of shapers, so no patch can stand in for it.  Channel c in {0, 1} of a bus that is not OFF is three reference
 * modules in series, ticked once per sample:
 *   MathModule(Multiply)   In1 = d_rows[b][c][t], In2 unconnected, constant = PRE
 *   NonLinearModule        (math.rs:203-205, 292-311) In1 = that product: a > 0 ? a.powf(e) : -(-a).powf(e).  The exponent e is
 *                          d_cv[b][t] when the bus is SRACK_BUS_SHAPER_CV and d_cv is given (In2 connected); otherwise In2 is unconnected
 *                          and e is EXPONENT (the module's (Some, None) arm) — for a CONST bus always.
 *   MathModule(Multiply)   by POST, written to d_out[b][c][t]
 * The two products are IEEE f32, one rounding each, no fma.  The power is the HOST libm's powf (Rust's f32::powf is glibc's), operation
 * for operation and misroundings included — never a correctly rounded power, never the device library's — in every render mode.  A
 * sample that is not > 0 takes the second arm: both zeros and NaN do (+0.0 with exponent -1 is -(-0.0).powf(-1) = +inf, -0.0 gives -inf).  ANY f32 parameter is accepted;
 * a non-finite sample, CV value or parameter affects that bus's rows and no other.  There is no state: no reset call, no state call, and
 * the result cannot depend on how the samples are cut into calls.
 *
 * params: f32 [n_buses][SRACK_BUS_SHAPER_NPARAMS] = PRE, EXPONENT, POST; NULL = 1, 1, 1
 * mode:   int [n_buses], SRACK_BUS_SHAPER_*; NULL = every bus CONST
 * Both are host memory.  A mode outside 0..2 is SRACK_ERR_INVALID and leaves the earlier setting in place.  get_shaper copies up to cap
 * buses (any pointer may be NULL) and returns n_buses, or 0 when no shapers are set.
 * Lifecycle (the VCAs' rules): the shapers belong to the handle, NOT to the patch's program: setting, changing or running them does not
 * re-flatten, restarts nothing, changes no bit of any other output; they survive an edit that re-flattens the patch.
 * srack_voices_configure drops them; so does srack_voices_set_buses with another n_buses (the same n_buses keeps them).  Rack files
 * carry nothing of this.
 *
 * The call:
 *   d_rows : device, f32 [n_buses][row_channels][n_samples], as for srack_buses_vca.  1 <= row_channels <= 8; channels 0 and 1 are
 *            processed, channels beyond the second are neither read nor written.
 *   d_cv   : device, f32 [n_buses][n_samples], or NULL; one row per bus, shared by its channels.  Must not overlap d_out.
 *   d_out  : device, the shape of d_rows, written: d_rows itself (in place) or disjoint from it.  An OFF bus's channels 0 and 1 are
 *            copied as 32-bit words; in place they are left alone (no work is launched for them).
 *   Any 4-byte aligned address is accepted for all three.
 *   stream : as for srack_render: asynchronous, and the library touches the stream only during the call.
 * Errors, in this order: SRACK_ERR_INVALID for a null handle; SRACK_ERR_STATE before srack_voices_configure or before a mix table
 * exists (all three calls); SRACK_ERR_STATE for srack_buses_shaper before set_shaper; n_samples == 0 is SRACK_OK and touches nothing;
 * SRACK_ERR_INVALID for a null d_rows or d_out, row_channels outside 1..8 or an overlap as above; SRACK_ERR_NOMEM if the table cannot
 * be allocated, the earlier table kept.
 * The kernel is a streaming pass, lanes on time: a wave takes 1024 samples of one bus and both its channels, several loads in flight,
 * the libm's tables in LDS (csrc/busshape.hip.h).  srack_render_info says " busshp=<buses not OFF>[<CV buses> cv]" between " busvca="
 * and " busfx=" once a call has run. */
#define SRACK_BUS_SHAPER_NPARAMS 3
enum { SRACK_BUS_SHAPER_PRE = 0, SRACK_BUS_SHAPER_EXPONENT = 1, SRACK_BUS_SHAPER_POST = 2 };
enum { SRACK_BUS_SHAPER_OFF = 0, SRACK_BUS_SHAPER_CONST = 1, SRACK_BUS_SHAPER_CV = 2 };
int srack_buses_set_shaper(srack_patch* p, const float* params, const int* mode);
int srack_buses_get_shaper(const srack_patch* p, float* params, int* mode, uint32_t cap);
int srack_buses_shaper(srack_patch* p, uint32_t n_samples, const float* d_rows, uint32_t row_channels,
                       const float* d_cv, float* d_out, void* stream);

/* ---- the bus meters: windowed level tracks and totals per mix bus, a read-only tap between any two console calls ---------------------
 * Which strip clips behind its shaper, how loud an aux bus is after its reverb, what the envelope of a drum group looks like over the
 * second: the per-voice statistics (srack_render_stats) applied to the f32 words of bus rows, per window of a stream and over all of it,
 * without the rows ever leaving the device.
 *   d_rows   : device, f32 [n_buses][row_channels][n_samples]: what any console call writes.  1 <= row_channels <= 8; channels 0 and 1
 *              are metered, channels beyond the second are not read.  Any 4-byte aligned address.  Never written.
 *   first_sample, n_samples : the call's samples are positions first_sample .. first_sample + n_samples - 1 of a metered stream that the
 *              HOST counts.
 *   d_levels : device, f64 [n_windows][SRACK_STAT_COUNT][n_buses][2], 8-byte aligned, or NULL.  Entity-minor like the per-voice
 *              statistics: one window is one contiguous frame of every strip's meters.  Record k of (bus, channel) covers stream
 *              positions [k * window, (k + 1) * window).  window >= SRACK_BUS_METER_MIN_WINDOW, n_windows >= 1 and
 *              first_sample + n_samples <= (uint64)n_windows * window.
 *   d_totals : device, f64 [SRACK_STAT_COUNT][n_buses][2], 8-byte aligned, or NULL: the same six numbers over everything the calls
 *              were given.
 * The definitions are the per-voice ones (SRACK_STAT_*), through the same device function: NaN or +-inf adds 1 to NONFINITE and nothing
 * else; otherwise SUM, SUM_SQ, PEAK_POS, PEAK_NEG and CLIPPED (|x| > 1; exactly +-1.0 does not clip) are updated, a peak only to a
 * strictly larger value.  RMS and dB are the host's division and root.
 * The call ADDS TO WHAT THE BUFFERS HOLD, for every record it touches and for the totals: SUM and SUM_SQ continue the sequential f64
 * loop in sample order from the stored value, bit for bit; the peaks are read back as f32; the counts are added as integers.  So the
 * host zero-fills once, a window cut by a call boundary is finished by the next call, and no bit depends on how the samples are cut
 * into calls.  For that reason the stage has no state on the handle: no reset call, no state call.
 * Untouched: records of windows outside floor(first_sample / window) .. floor((first_sample + n_samples - 1) / window) are neither
 * read nor written; with row_channels == 1 every channel-1 entry is left alone (the master's convention).
 * d_levels and d_totals must not overlap d_rows or each other.
 * Errors, in this order: SRACK_ERR_INVALID for a null handle; SRACK_ERR_STATE before srack_voices_configure or before a mix table
 * exists; n_samples == 0 is SRACK_OK and touches nothing; SRACK_ERR_INVALID for a null d_rows, row_channels outside 1..8, both outputs
 * NULL, a misaligned output, with d_levels given a window below the minimum, n_windows == 0 or a span too short, or an overlap.  With
 * d_levels == NULL, window, n_windows and first_sample are ignored.
 * The stage belongs to the handle like every console stage, and owns nothing: running it does not re-flatten, restarts nothing and
 * changes no bit of any other output or state.  srack_render_info says " meter=<n_buses>[w<window>]" behind " master=" once a call has
 * run; the window reads "-" when only totals were taken.
 * The kernel is the bus filters' shape: a lane per (bus, channel) row, tiles of 64 rows x 64 samples turned through LDS, two sets of
 * statistics in registers, the open record stored and the next one loaded at a window boundary (csrc/busmeter.hip.h). */
#define SRACK_BUS_METER_MIN_WINDOW 64
int srack_buses_meter(srack_patch* p, uint64_t first_sample, uint32_t n_samples,
                      const float* d_rows, uint32_t row_channels, uint32_t window,
                      double* d_levels, uint32_t n_windows, double* d_totals, void* stream);

/* Optional: do everything a later srack_render(p, <= n_samples, ..., flags) would do on first use — flatten the graph,
 * upload the programs and the voice table, size the scratch buffers (mix partials when want_mix, control tracks) — so
 * that the first render costs what every render costs.  Renders nothing and leaves the voice state untouched. */
int srack_render_reserve(srack_patch* p, uint32_t n_samples, int want_mix, uint32_t flags);

/* Diagnostics of the specialised kernel (tests, tools): the HIP source generated for the voice program of the current patch
 * under `flags` (returns its length, copies at most cap - 1 characters; SRACK_ERR_UNSUPPORTED if the program holds an op the
 * generator does not cover), and its compilation for gfx950 without rendering anything (needs hiprtc, but no GPU). */
int srack_render_kernel_source(srack_patch* p, uint32_t flags, char* buf, size_t cap);
int srack_render_kernel_compile(srack_patch* p, uint32_t flags);

/* Scratch the render needs for the mix-down partials etc. is owned by the handle; this reports it. */
/* Human-readable: the programs (ops, rows, units), "approx[...]" — the default mode's error bound or why the flavour is exact —, any
 * SRACK_* tuning variable the process carries ("knobs=[...]": such a process does not render what was tested), "buses=<n>[fold]" when the
 * last render filled the mixes of n buses (by a fold over each launch's frames), "busfx=<n>[block <T>]" once the bus reverbs have run, where the kernel came from, and last "kernel=<name>".  Returns the length; copies at most cap - 1 characters (buf may be NULL to ask for the length). */
int srack_render_info(srack_patch* p, char* buf, size_t cap);

/* Average duration in ms of the dominant render kernel over the renders since the last call with
 * reset != 0, measured with HIP events on the render's own stream.  Returns the number of launches
 * in *n_launches. */
int srack_render_kernel_ms(srack_patch* p, double* avg_ms, int* n_launches, int reset);

/* Read back one field of every voice's state after a render (host buffer, n_voices doubles). */
int srack_voices_get_field(srack_patch* p, int module, int field, double* values);

/* ---- the cache of run-time specialised kernels ------------------------------------------------------------
 * A general patch (anything the hand-matched kernels do not cover) renders through a kernel compiled for its STRUCTURE with hiprtc
 * the first time that structure is seen (0.3 - 2 s).  Code objects are kept in memory (the last SRACK_KERNEL_CACHE_MAX structures,
 * default 64, least recently used first out; a module is unloaded once no patch renders with it) and ON DISK, so the next start of
 * the host — and every other rank of a multi-GPU job — loads instead of compiling (ranks starting together serialise on a file
 * lock: one compiles).  The directory: srack_kernel_cache_set_dir(path); "off" disables the disk level; NULL restores the default
 * resolution — $SRACK_KERNEL_CACHE_DIR, else `.srack_kernel_cache` next to this library if writable, else $XDG_CACHE_HOME/srack_hip
 * or ~/.cache/srack_hip.  srack_render_info names where a patch's kernel came from: jit=compiled(N ms) | disk-cache | memory-cache |
 * unavailable(reason).  No counterpart in the reference (its modules are compiled Rust, src/synth.rs:300-317). */
typedef struct srack_kernel_cache_info {
    uint64_t compiled;               /* hiprtc compilations by this process */
    uint64_t disk_hits, memory_hits;
    uint64_t modules_loaded;
    uint64_t code_evictions, module_evictions;
    uint64_t resident_code_objects, resident_modules;
    double compile_ms;               /* total hiprtc time */
    char directory[512];             /* the disk cache in use; "" = none */
} srack_kernel_cache_info;
int srack_kernel_cache_set_dir(const char* dir);
int srack_kernel_cache_stats(srack_kernel_cache_info* out);

/* ---- device helpers for hosts without a HIP binding ---------------------------------------- */
int srack_device_count(int* n);
int srack_device_set(int device);
/* The calling thread's current device — the one srack_render launches on — and its PCI bus id ("0000:05:00.0"), so that a
 * multi-rank host can check that its ranks really are on different GPUs.  Either pointer may be NULL. */
int srack_device_get(int* device, char* pci_bus_id, size_t cap);
int srack_device_alloc(void** d_ptr, size_t bytes);
int srack_device_free(void* d_ptr);
/* Waits for `stream`, then copies through pinned buffers of the library's own (the caller's memory may be pageable; per device, double-buffered,
 * large copies on several helper threads: 51 GB/s for 50 GB on the GPU box); returns when h_dst holds the bytes. */
int srack_device_to_host(void* h_dst, const void* d_src, size_t bytes, void* stream);
/* The other way (e.g. a statistics buffer to start from): enqueued on `stream`, returns once h_src may be reused. */
int srack_device_from_host(void* d_dst, const void* h_src, size_t bytes, void* stream);
int srack_device_sync(void* stream);

/* ---- multi-GPU mix-down --------------------------------------------------------------------- */
/* Voices shard across ranks (one process per GPU) with no exchange during the render; the only collective is the sum of
 * the per-rank partial mixes over RCCL / xGMI.  The reference has no counterpart: it is single-threaded
 * (src/main.rs:59-63); SURVEY 8(b) item 8 / 8(e) define this surface.
 *
 *   rank 0:      srack_dist_unique_id(id)                  ncclGetUniqueId; the host carries the SRACK_DIST_ID_BYTES to
 *                                                          every rank over any side channel it has
 *   every rank:  srack_device_set(local_rank); srack_dist_init(id, n_ranks, rank, &comm)     ncclCommInitRank
 *                srack_render(...); srack_dist_reduce_mix(comm, d_mix, channels * n_samples, 0, stream)
 *                srack_dist_destroy(comm)
 *
 * `comm` is a plain RCCL `ncclComm_t`: a host that already owns one may pass it to srack_dist_reduce_mix directly.
 * srack_dist_reduce_mix is ncclReduce(sum, f32, root) on `stream`, in place on `d_mix`. */
#define SRACK_DIST_ID_BYTES 128
int srack_dist_unique_id(void* id_out /* SRACK_DIST_ID_BYTES */);
int srack_dist_init(const void* id /* SRACK_DIST_ID_BYTES */, int n_ranks, int rank, void** comm_out);
int srack_dist_comm_count(void* comm, int* n_ranks); /* ncclCommCount: the ranks the communicator really spans */
int srack_dist_destroy(void* comm);
int srack_dist_reduce_mix(void* comm, float* d_mix, size_t count, int root, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRACK_HIP_H */
