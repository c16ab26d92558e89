//! Safe-ish Rust wrapper over the C ABI of the MI355X batch-render path (`include/srack_hip.h`).
//!
//! NOT COMPILED in the build image (no rustc there) — reviewed against the header by hand.  It is the
//! "Rust host" of the north star: the s-rack crate would depend on this crate behind a `gpu` feature and
//! call [`Patch::execute_batch`] where the audio callback calls `synth::execute(&plan)` (src/main.rs:59-63).
//!
//! Error mapping: every C entry point returns `int` (0 ok, < 0 error).  The reference's `Result<_, ()>`
//! becomes `Result<_, Error>` with the status code and the library's thread-local message.
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct SrackPatch {
    _private: [u8; 0],
}

#[allow(non_camel_case_types)]
mod ffi {
    use super::*;
    /// `srack_kernel_cache_info` (include/srack_hip.h)
    #[repr(C)]
    pub struct SrackKernelCacheInfo {
        pub compiled: u64,
        pub disk_hits: u64,
        pub memory_hits: u64,
        pub modules_loaded: u64,
        pub code_evictions: u64,
        pub module_evictions: u64,
        pub resident_code_objects: u64,
        pub resident_modules: u64,
        pub compile_ms: f64,
        pub directory: [c_char; 512],
    }

    extern "C" {
        pub fn srack_abi_version() -> c_int;
        pub fn srack_last_error() -> *const c_char;
        pub fn srack_patch_create(sample_rate: u32, buffer_size: u32, channels: u32, out: *mut *mut SrackPatch) -> c_int;
        pub fn srack_patch_destroy(p: *mut SrackPatch) -> c_int;
        pub fn srack_patch_add_module(p: *mut SrackPatch, module_type: c_int) -> c_int;
        pub fn srack_patch_set_field(p: *mut SrackPatch, module: c_int, field: c_int, value: f64) -> c_int;
        pub fn srack_patch_get_field(p: *const SrackPatch, module: c_int, field: c_int, value: *mut f64) -> c_int;
        pub fn srack_patch_set_step(p: *mut SrackPatch, module: c_int, channel: c_int, step: c_int, state: c_int, value: c_int) -> c_int;
        pub fn srack_patch_set_output_buffer(p: *mut SrackPatch, module: c_int, port: c_int, samples: *const f32, n: u32) -> c_int;
        pub fn srack_patch_get_output_buffer(p: *const SrackPatch, module: c_int, port: c_int, dst: *mut f32, cap: u32) -> c_int;
        pub fn srack_patch_set_noise_seed(p: *mut SrackPatch, seed: u64, first_voice: u64) -> c_int;
        pub fn srack_patch_keep_state(p: *mut SrackPatch, keep: c_int) -> c_int;
        pub fn srack_patch_set_wave(p: *mut SrackPatch, module: c_int, samples: *const f32, n_samples: u32, sample_rate: f32) -> c_int;
        pub fn srack_patch_load_srk(bytes: *const c_void, n_bytes: usize, sample_rate: u32, buffer_size: u32, channels: u32, out: *mut *mut SrackPatch) -> c_int;
        pub fn srack_patch_save_srk(p: *const SrackPatch, buf: *mut c_void, cap: usize, n_bytes: *mut usize) -> c_int;
        pub fn srack_patch_connect(p: *mut SrackPatch, src: c_int, src_port: c_int, sink: c_int, sink_port: c_int) -> c_int;
        pub fn srack_patch_disconnect(p: *mut SrackPatch, sink: c_int, sink_port: c_int) -> c_int;
        pub fn srack_patch_plan(p: *mut SrackPatch, order: *mut c_int, cap: c_int) -> c_int;
        pub fn srack_voices_configure(p: *mut SrackPatch, n_voices: u32) -> c_int;
        pub fn srack_voices_set_field_f32(p: *mut SrackPatch, module: c_int, field: c_int, values: *const f32) -> c_int;
        pub fn srack_render_planes(p: *mut SrackPatch, channel_plane: *mut c_int, cap: c_int) -> c_int;
        pub fn srack_render(p: *mut SrackPatch, n_samples: u32, d_frames: *mut f32, d_mix: *mut f32, flags: u32, stream: *mut c_void) -> c_int;
        pub fn srack_render_stats(p: *mut SrackPatch, n_samples: u32, d_frames: *mut f32, d_mix: *mut f32, d_stats: *mut f64, flags: u32, stream: *mut c_void) -> c_int;
        pub fn srack_voices_set_buses(p: *mut SrackPatch, n_buses: u32, bus: *const c_int, gain: *const f32) -> c_int;
        pub fn srack_voices_get_buses(p: *const SrackPatch, bus: *mut c_int, gain: *mut f32, cap: u32) -> c_int;
        pub fn srack_voices_set_bus_slots(p: *mut SrackPatch, n_buses: u32, n_slots: u32, bus: *const c_int, gain: *const f32) -> c_int;
        pub fn srack_voices_get_bus_slots(p: *const SrackPatch, n_slots: *mut c_int, bus: *mut c_int, gain: *mut f32, cap: u32) -> c_int;
        pub fn srack_patch_set_wave_bank(p: *mut SrackPatch, module: c_int, samples: *const f32, lengths: *const c_int, sample_rates: *const f32, n_waves: u32) -> c_int;
        pub fn srack_patch_get_wave_bank(p: *const SrackPatch, module: c_int, lengths: *mut c_int, sample_rates: *mut f32, cap: u32) -> c_int;
        pub fn srack_patch_get_wave_bank_samples(p: *const SrackPatch, module: c_int, wave: c_int, samples: *mut f32, cap: u32) -> c_int;
        pub fn srack_voices_set_waves(p: *mut SrackPatch, module: c_int, wave: *const c_int) -> c_int;
        pub fn srack_voices_get_waves(p: *const SrackPatch, module: c_int, wave: *mut c_int, cap: u32) -> c_int;
        pub fn srack_patch_set_sequence_bank(p: *mut SrackPatch, module: c_int, states: *const u8, values: *const c_void, lengths: *const c_int, n_sequences: u32) -> c_int;
        pub fn srack_patch_get_sequence_bank(p: *const SrackPatch, module: c_int, states: *mut u8, values: *mut c_void, lengths: *mut c_int, cap: u32) -> c_int;
        pub fn srack_voices_set_sequences(p: *mut SrackPatch, module: c_int, seq: *const c_int) -> c_int;
        pub fn srack_voices_get_sequences(p: *const SrackPatch, module: c_int, seq: *mut c_int, cap: u32) -> c_int;
        pub fn srack_render_buses(p: *mut SrackPatch, n_samples: u32, d_frames: *mut f32, d_mix: *mut f32, d_stats: *mut f64, d_bus_mix: *mut f32, flags: u32, stream: *mut c_void) -> c_int;
        pub fn srack_buses_set_reverb(p: *mut SrackPatch, params: *const f64, enabled: *const c_int) -> c_int;
        pub fn srack_buses_get_reverb(p: *const SrackPatch, params: *mut f64, enabled: *mut c_int, cap: u32) -> c_int;
        pub fn srack_buses_reset_reverb(p: *mut SrackPatch) -> c_int;
        pub fn srack_buses_reverb_plan(p: *const SrackPatch, line_lengths: *mut c_int, block: *mut c_int) -> c_int;
        pub fn srack_buses_reverb(p: *mut SrackPatch, n_samples: u32, d_bus_mix: *const f32, d_bus_fx: *mut f32, stream: *mut c_void) -> c_int;
        pub fn srack_buses_set_master(p: *mut SrackPatch, gain: *const f32) -> c_int;
        pub fn srack_buses_get_master(p: *const SrackPatch, gain: *mut f32, cap: u32) -> c_int;
        pub fn srack_buses_master(p: *mut SrackPatch, n_samples: u32, d_rows: *const f32, row_channels: u32, d_master: *mut f32, d_master_stats: *mut f64, stream: *mut c_void) -> c_int;
        pub fn srack_buses_set_sends(p: *mut SrackPatch, n_sends: u32, src: *const c_int, dst: *const c_int, gain: *const f32, through: *const f32) -> c_int;
        pub fn srack_buses_get_sends(p: *const SrackPatch, src: *mut c_int, dst: *mut c_int, gain: *mut f32, cap: u32, through: *mut f32, through_cap: u32) -> c_int;
        pub fn srack_buses_send_plan(p: *const SrackPatch, n_terms: *mut c_int, bus_cap: u32, order: *mut c_int, order_cap: u32) -> c_int;
        pub fn srack_buses_send(p: *mut SrackPatch, n_samples: u32, d_rows: *const f32, row_channels: u32, d_out: *mut f32, stream: *mut c_void) -> c_int;
        pub fn srack_buses_set_filter(p: *mut SrackPatch, params: *const f32, port: *const c_int, enabled: *const c_int) -> c_int;
        pub fn srack_buses_get_filter(p: *const SrackPatch, params: *mut f32, port: *mut c_int, enabled: *mut c_int, cap: u32) -> c_int;
        pub fn srack_buses_reset_filter(p: *mut SrackPatch) -> c_int;
        pub fn srack_buses_filter_state(p: *mut SrackPatch, state: *mut f32, cap: u32) -> c_int;
        pub fn srack_buses_filter(p: *mut SrackPatch, n_samples: u32, d_rows: *const f32, row_channels: u32, d_cv: *const f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
        pub fn srack_buses_set_vca(p: *mut SrackPatch, params: *const f32, mode: *const c_int, negative: *const c_int) -> c_int;
        pub fn srack_buses_get_vca(p: *const SrackPatch, params: *mut f32, mode: *mut c_int, negative: *mut c_int, cap: u32) -> c_int;
        pub fn srack_buses_reset_vca(p: *mut SrackPatch) -> c_int;
        pub fn srack_buses_vca_state(p: *mut SrackPatch, state: *mut f32, cap: u32) -> c_int;
        pub fn srack_buses_vca(p: *mut SrackPatch, n_samples: u32, d_rows: *const f32, row_channels: u32, d_ctl: *const f32, d_out: *mut f32, d_env: *mut f32, stream: *mut c_void) -> c_int;
        pub fn srack_buses_set_osc(p: *mut SrackPatch, params: *const f32, port: *const c_int, antialiasing: *const c_int, enabled: *const c_int) -> c_int;
        pub fn srack_buses_get_osc(p: *const SrackPatch, params: *mut f32, port: *mut c_int, antialiasing: *mut c_int, enabled: *mut c_int, cap: u32) -> c_int;
        pub fn srack_buses_reset_osc(p: *mut SrackPatch, pos: *const f64) -> c_int;
        pub fn srack_buses_osc_state(p: *mut SrackPatch, state: *mut f64, cap: u32) -> c_int;
        pub fn srack_buses_osc(p: *mut SrackPatch, n_samples: u32, d_cv: *const f32, d_sync: *const f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
        pub fn srack_buses_set_shaper(p: *mut SrackPatch, params: *const f32, mode: *const c_int) -> c_int;
        pub fn srack_buses_get_shaper(p: *const SrackPatch, params: *mut f32, mode: *mut c_int, cap: u32) -> c_int;
        pub fn srack_buses_shaper(p: *mut SrackPatch, n_samples: u32, d_rows: *const f32, row_channels: u32, d_cv: *const f32, d_out: *mut f32, stream: *mut c_void) -> c_int;
        pub fn srack_buses_meter(p: *mut SrackPatch, first_sample: u64, n_samples: u32, d_rows: *const f32, row_channels: u32, window: u32, d_levels: *mut f64, n_windows: u32, d_totals: *mut f64, stream: *mut c_void) -> c_int;
        pub fn srack_device_alloc(d_ptr: *mut *mut c_void, bytes: usize) -> c_int;
        pub fn srack_device_free(d_ptr: *mut c_void) -> c_int;
        pub fn srack_device_to_host(h_dst: *mut c_void, d_src: *const c_void, bytes: usize, stream: *mut c_void) -> c_int;
        pub fn srack_device_from_host(d_dst: *mut c_void, h_src: *const c_void, bytes: usize, stream: *mut c_void) -> c_int;
        pub fn srack_device_set(device: c_int) -> c_int;
        pub fn srack_device_get(device: *mut c_int, pci_bus_id: *mut c_char, cap: usize) -> c_int;
        pub fn srack_kernel_cache_set_dir(dir: *const c_char) -> c_int;
        pub fn srack_kernel_cache_stats(out: *mut SrackKernelCacheInfo) -> c_int;
        pub fn srack_render_reserve(p: *mut SrackPatch, n_samples: u32, want_mix: c_int, flags: u32) -> c_int;
        pub fn srack_dist_unique_id(id_out: *mut u8) -> c_int;
        pub fn srack_dist_init(id: *const u8, n_ranks: c_int, rank: c_int, comm_out: *mut *mut c_void) -> c_int;
        pub fn srack_dist_comm_count(comm: *mut c_void, n_ranks: *mut c_int) -> c_int;
        pub fn srack_dist_reduce_mix(comm: *mut c_void, d_mix: *mut f32, count: usize, root: c_int, stream: *mut c_void) -> c_int;
        pub fn srack_dist_destroy(comm: *mut c_void) -> c_int;
    }
}

/// Fields of a statistics buffer (values of `SRACK_STAT_*`): `[planes][STAT_COUNT][n_voices]` f64.
pub mod stat {
    pub const SUM: usize = 0;
    pub const SUM_SQ: usize = 1;
    pub const PEAK_POS: usize = 2;
    pub const PEAK_NEG: usize = 3;
    pub const NONFINITE: usize = 4;
    pub const CLIPPED: usize = 5;
    pub const COUNT: usize = 6;
}

/// Mix buses (`SRACK_MAX_BUSES`, `SRACK_BUS_NONE`).
pub const MAX_BUSES: u32 = 65536;
pub const BUS_NONE: i32 = -1;
/// The most buses a voice can feed through `set_bus_slots` (`SRACK_MAX_VOICE_SLOTS`).
pub const MAX_VOICE_SLOTS: u32 = 4;
/// A voice that plays its SampleModule's own wave, not one of the bank (`SRACK_WAVE_OWN`).
pub const WAVE_OWN: i32 = -1;
/// A voice that plays its sequencer's own cells at the module's length, not a sequence of the bank (`SRACK_SEQ_OWN`).
pub const SEQ_OWN: i32 = -1;
/// The most sequences a bank may hold (`SRACK_MAX_SEQUENCES`).
pub const MAX_SEQUENCES: u32 = 65536;

/// Render flags (values of `SRACK_RENDER_*`).
pub mod render_flags {
    pub const DEFAULT: u32 = 0;
    pub const EXACT_OSC: u32 = 1 << 0;
    pub const NO_FUSION: u32 = 1 << 1;
    pub const NO_UNIFORM_HOIST: u32 = 1 << 2;
    pub const NO_CTL_STAGES: u32 = 1 << 3;
    /// the general path always through the tile interpreter
    pub const NO_SPECIALIZE: u32 = 1 << 4;
    /// the general path through a kernel specialised for the program, whatever the voice count
    pub const SPECIALIZE: u32 = 1 << 5;
    /// keep the default mode's fast forms where its error bound would make oscillators (or the patch) exact: a render of seconds, not minutes
    pub const KEEP_DEFAULT: u32 = 1 << 6;
}

pub const DIST_ID_BYTES: usize = 128;

/// Module types of the hot path (values of `SRACK_MOD_*`).
#[repr(i32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ModuleType {
    Output = 0,
    Oscillator = 1,
    MoogFilter = 2,
    Adsr = 3,
    Vca = 4,
    MonoMixer = 5,
    Math = 6,
    GridSequencer = 7,
    PatternSequencer = 8,
    NonLinear = 9,
    Sample = 10,
    Noise = 11,
    Freeverb = 12,
}

#[derive(Debug)]
pub struct Error {
    pub code: i32,
    pub message: String,
}

fn check(rc: c_int) -> Result<c_int, Error> {
    if rc >= 0 {
        return Ok(rc);
    }
    let message = unsafe { CStr::from_ptr(ffi::srack_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

/// Device buffer owned by the caller (freed on drop).
pub struct DeviceBuffer {
    ptr: *mut c_void,
    bytes: usize,
}

impl DeviceBuffer {
    pub fn new(bytes: usize) -> Result<Self, Error> {
        let mut ptr = std::ptr::null_mut();
        check(unsafe { ffi::srack_device_alloc(&mut ptr, bytes) })?;
        Ok(Self { ptr, bytes })
    }
    pub fn as_f32(&self) -> *mut f32 {
        self.ptr as *mut f32
    }
    pub fn to_host(&self, dst: &mut [f32]) -> Result<(), Error> {
        assert!(dst.len() * 4 <= self.bytes);
        check(unsafe { ffi::srack_device_to_host(dst.as_mut_ptr() as *mut c_void, self.ptr, dst.len() * 4, std::ptr::null_mut()) }).map(|_| ())
    }
    pub fn as_f64(&self) -> *mut f64 {
        self.ptr as *mut f64
    }
    pub fn to_host_f64(&self, dst: &mut [f64]) -> Result<(), Error> {
        assert!(dst.len() * 8 <= self.bytes);
        check(unsafe { ffi::srack_device_to_host(dst.as_mut_ptr() as *mut c_void, self.ptr, dst.len() * 8, std::ptr::null_mut()) }).map(|_| ())
    }
    pub fn from_host_f64(&mut self, src: &[f64]) -> Result<(), Error> {
        assert!(src.len() * 8 <= self.bytes);
        check(unsafe { ffi::srack_device_from_host(self.ptr, src.as_ptr() as *const c_void, src.len() * 8, std::ptr::null_mut()) }).map(|_| ())
    }
}

impl Drop for DeviceBuffer {
    fn drop(&mut self) {
        unsafe { ffi::srack_device_free(self.ptr) };
    }
}

/// The workspace's module list + plan + N voices (mirror of `SynthModuleWorkspaceImpl`, src/ui.rs:52-60).
pub struct Patch {
    raw: *mut SrackPatch,
}

impl Patch {
    /// `AudioConfig { sample_rate, buffer_size, channels }` (src/synth.rs:20-25).
    pub fn new(sample_rate: u16, buffer_size: usize, channels: u8) -> Result<Self, Error> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::srack_patch_create(sample_rate as u32, buffer_size as u32, channels as u32, &mut raw) })?;
        Ok(Self { raw })
    }
    /// `Module::new(&audio_config)` pushed to the module list; returns its index in `all_modules`.
    pub fn add_module(&mut self, t: ModuleType) -> Result<i32, Error> {
        check(unsafe { ffi::srack_patch_add_module(self.raw, t as c_int) })
    }
    pub fn set_field(&mut self, module: i32, field: i32, value: f64) -> Result<(), Error> {
        check(unsafe { ffi::srack_patch_set_field(self.raw, module, field, value) }).map(|_| ())
    }
    pub fn get_field(&self, module: i32, field: i32) -> Result<f64, Error> {
        let mut v = 0.0;
        check(unsafe { ffi::srack_patch_get_field(self.raw, module, field, &mut v) })?;
        Ok(v)
    }
    pub fn set_step(&mut self, module: i32, channel: i32, step: i32, state: i32, value: i32) -> Result<(), Error> {
        check(unsafe { ffi::srack_patch_set_step(self.raw, module, channel, step, state, value) }).map(|_| ())
    }
    /// What `WaveBox::load` leaves behind (src/synth/sample.rs:31-69): first channel as f32 + the file's sample rate.
    /// Edits between renders carry the modules' state over instead of restarting the voices (the reference's sliders do not reset state).
    pub fn keep_state(&mut self, keep: bool) -> Result<(), Error> {
        check(unsafe { ffi::srack_patch_keep_state(self.raw, keep as c_int) }).map(|_| ())
    }

    /// NoiseModule streams are keyed by (seed, module, first_voice + voice); the reference's generator is OS-seeded.
    pub fn set_noise_seed(&mut self, seed: u64, first_voice: u64) -> Result<(), Error> {
        check(unsafe { ffi::srack_patch_set_noise_seed(self.raw, seed, first_voice) }).map(|_| ())
    }

    pub fn set_wave(&mut self, module: i32, samples: &[f32], sample_rate: f32) -> Result<(), Error> {
        check(unsafe { ffi::srack_patch_set_wave(self.raw, module, samples.as_ptr(), samples.len() as u32, sample_rate) }).map(|_| ())
    }
    /// `SynthModuleWorkspaceImpl::deserialize` (src/ui.rs:116-135): a saved rack against this host's AudioConfig.
    pub fn load_srk(bytes: &[u8], sample_rate: u16, buffer_size: usize, channels: u8) -> Result<Self, Error> {
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            ffi::srack_patch_load_srk(bytes.as_ptr() as *const c_void, bytes.len(), sample_rate as u32, buffer_size as u32, channels as u32, &mut raw)
        })?;
        Ok(Self { raw })
    }
    /// `serialize` (src/ui.rs:98-114).
    pub fn save_srk(&self) -> Result<Vec<u8>, Error> {
        let mut n = 0usize;
        check(unsafe { ffi::srack_patch_save_srk(self.raw, std::ptr::null_mut(), 0, &mut n) })?;
        let mut buf = vec![0u8; n];
        check(unsafe { ffi::srack_patch_save_srk(self.raw, buf.as_mut_ptr() as *mut c_void, n, &mut n) })?;
        Ok(buf)
    }
    /// `SynthModule::set_input(input_idx, src_module, src_port)`.
    pub fn set_input(&mut self, sink: i32, input_idx: u8, src: i32, src_port: u8) -> Result<(), Error> {
        check(unsafe { ffi::srack_patch_connect(self.raw, src, src_port as c_int, sink, input_idx as c_int) }).map(|_| ())
    }
    pub fn disconnect_input(&mut self, sink: i32, input_idx: u8) -> Result<(), Error> {
        check(unsafe { ffi::srack_patch_disconnect(self.raw, sink, input_idx as c_int) }).map(|_| ())
    }
    /// `plan_execution` as the workspace drives it: the execution order as module indices.
    pub fn plan(&mut self) -> Result<Vec<i32>, Error> {
        let mut order = vec![0 as c_int; 1024];
        let n = check(unsafe { ffi::srack_patch_plan(self.raw, order.as_mut_ptr(), order.len() as c_int) })?;
        order.truncate(n as usize);
        Ok(order)
    }
    pub fn configure_voices(&mut self, n_voices: u32) -> Result<(), Error> {
        check(unsafe { ffi::srack_voices_configure(self.raw, n_voices) }).map(|_| ())
    }
    pub fn set_voice_field(&mut self, module: i32, field: i32, values: &[f32]) -> Result<(), Error> {
        check(unsafe { ffi::srack_voices_set_field_f32(self.raw, module, field, values.as_ptr()) }).map(|_| ())
    }
    /// Number of distinct output planes and the plane of each channel (-1 = unconnected).
    pub fn planes(&mut self, channels: usize) -> Result<(usize, Vec<i32>), Error> {
        let mut cp = vec![0 as c_int; channels];
        let n = check(unsafe { ffi::srack_render_planes(self.raw, cp.as_mut_ptr(), channels as c_int) })?;
        Ok((n as usize, cp))
    }
    /// The batch counterpart of `execute(&plan)`: `n_samples` ticks of every voice, asynchronous on the default
    /// stream.  `frames`: `[planes][n_samples][n_voices]` f32, `mix`: `[channels][n_samples]` f32 (either may be None).
    pub fn execute_batch(&mut self, n_samples: u32, frames: Option<&DeviceBuffer>, mix: Option<&DeviceBuffer>, flags: u32) -> Result<(), Error> {
        let f = frames.map_or(std::ptr::null_mut(), |b| b.as_f32());
        let m = mix.map_or(std::ptr::null_mut(), |b| b.as_f32());
        check(unsafe { ffi::srack_render(self.raw, n_samples, f, m, flags, std::ptr::null_mut()) }).map(|_| ())
    }
    /// `execute_batch` plus per-voice statistics folded into `stats`: `[planes][STAT_COUNT][n_voices]` f64, zero-filled once by the
    /// host (`from_host_f64`) and added to by every call (`srack_render_stats`).
    pub fn execute_batch_stats(&mut self, n_samples: u32, frames: Option<&DeviceBuffer>, mix: Option<&DeviceBuffer>, stats: &DeviceBuffer, flags: u32) -> Result<(), Error> {
        let f = frames.map_or(std::ptr::null_mut(), |b| b.as_f32());
        let m = mix.map_or(std::ptr::null_mut(), |b| b.as_f32());
        check(unsafe { ffi::srack_render_stats(self.raw, n_samples, f, m, stats.as_f64(), flags, std::ptr::null_mut()) }).map(|_| ())
    }
    /// The mix table of the voices: `bus[v]` in `0 .. n_buses` or `BUS_NONE` (None: every voice in bus 0), `gain[v]` any f32 (None: 1.0).
    /// Not part of the program: changing it between renders restarts nothing (`srack_voices_set_buses`).
    pub fn set_buses(&mut self, n_buses: u32, bus: Option<&[i32]>, gain: Option<&[f32]>) -> Result<(), Error> {
        let b = bus.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        let g = gain.map_or(std::ptr::null(), |x| x.as_ptr());
        check(unsafe { ffi::srack_voices_set_buses(self.raw, n_buses, b, g) }).map(|_| ())
    }
    /// `(n_buses, bus, gain)` of the table set, `n_voices` entries each; `n_buses` 0: none set.
    pub fn get_buses(&self, n_voices: usize) -> Result<(u32, Vec<i32>, Vec<f32>), Error> {
        let (mut b, mut g) = (vec![0 as c_int; n_voices], vec![0f32; n_voices]);
        let n = check(unsafe { ffi::srack_voices_get_buses(self.raw, b.as_mut_ptr(), g.as_mut_ptr(), n_voices as u32) })?;
        Ok((n as u32, b, g))
    }
    /// The mix table with up to `MAX_VOICE_SLOTS` buses per voice and a gain per channel: `bus[v][k]` (None: slot 0 is bus 0, the others
    /// none), `gain[v][k][c]` any f32 (None: 1.0).  Pan is one slot with a gain per channel, a per-voice send a second slot.  Replaces a
    /// table set with `set_buses`, and is replaced by it (`srack_voices_set_bus_slots`).
    pub fn set_bus_slots(&mut self, n_buses: u32, n_slots: u32, bus: Option<&[i32]>, gain: Option<&[f32]>) -> Result<(), Error> {
        let b = bus.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        let g = gain.map_or(std::ptr::null(), |x| x.as_ptr());
        check(unsafe { ffi::srack_voices_set_bus_slots(self.raw, n_buses, n_slots, b, g) }).map(|_| ())
    }
    /// `(n_buses, n_slots, bus [n_voices][n_slots], gain [n_voices][n_slots][channels])` of the table set; `n_buses` 0: none set.
    pub fn get_bus_slots(&self, n_voices: usize, channels: usize) -> Result<(u32, u32, Vec<i32>, Vec<f32>), Error> {
        let mut k: c_int = 0;
        let n = check(unsafe { ffi::srack_voices_get_bus_slots(self.raw, &mut k, std::ptr::null_mut(), std::ptr::null_mut(), 0) })?;
        let (mut b, mut g) = (vec![0 as c_int; n_voices * k as usize], vec![0f32; n_voices * k as usize * channels]);
        check(unsafe { ffi::srack_voices_get_bus_slots(self.raw, &mut k, b.as_mut_ptr(), g.as_mut_ptr(), n_voices as u32) })?;
        Ok((n as u32, k as u32, b, g))
    }
    /// A bank of waves for a SampleModule, laid back to back in `samples`: wave k has `lengths[k]` samples and the rate `sample_rates[k]`
    /// (`srack_patch_set_wave_bank`; an empty bank removes it).  Inert until `set_voice_waves` assigns voices to it.
    pub fn set_wave_bank(&mut self, module: i32, samples: &[f32], lengths: &[i32], sample_rates: &[f32]) -> Result<(), Error> {
        assert!(lengths.len() == sample_rates.len() && lengths.iter().map(|&n| n.max(0) as usize).sum::<usize>() <= samples.len());
        check(unsafe { ffi::srack_patch_set_wave_bank(self.raw, module, samples.as_ptr(), lengths.as_ptr() as *const c_int, sample_rates.as_ptr(), lengths.len() as u32) }).map(|_| ())
    }
    /// `(lengths, sample_rates)` of the bank; empty without one.
    pub fn get_wave_bank(&self, module: i32) -> Result<(Vec<i32>, Vec<f32>), Error> {
        let n = check(unsafe { ffi::srack_patch_get_wave_bank(self.raw, module, std::ptr::null_mut(), std::ptr::null_mut(), 0) })? as usize;
        let (mut l, mut r) = (vec![0 as c_int; n], vec![0f32; n]);
        check(unsafe { ffi::srack_patch_get_wave_bank(self.raw, module, l.as_mut_ptr(), r.as_mut_ptr(), n as u32) })?;
        Ok((l, r))
    }
    /// The samples of one wave of the bank.
    pub fn get_wave_bank_samples(&self, module: i32, wave: i32) -> Result<Vec<f32>, Error> {
        let n = check(unsafe { ffi::srack_patch_get_wave_bank_samples(self.raw, module, wave, std::ptr::null_mut(), 0) })? as usize;
        let mut s = vec![0f32; n];
        check(unsafe { ffi::srack_patch_get_wave_bank_samples(self.raw, module, wave, s.as_mut_ptr(), n as u32) })?;
        Ok(s)
    }
    /// Which wave of the bank every voice plays: `wave[v]` in `0 .. n_waves` or `WAVE_OWN` (the module's own wave); None clears.  Voice v
    /// renders what a one-voice patch renders after `set_wave(bank wave wave[v], its rate)` (`srack_voices_set_waves`).
    pub fn set_voice_waves(&mut self, module: i32, wave: Option<&[i32]>) -> Result<(), Error> {
        let w = wave.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        check(unsafe { ffi::srack_voices_set_waves(self.raw, module, w) }).map(|_| ())
    }
    /// The assignment, `n_voices` entries; None when none is set.
    pub fn get_voice_waves(&self, module: i32, n_voices: usize) -> Result<Option<Vec<i32>>, Error> {
        let mut w = vec![0 as c_int; n_voices];
        let n = check(unsafe { ffi::srack_voices_get_waves(self.raw, module, w.as_mut_ptr(), n_voices as u32) })?;
        Ok(if n == 0 { None } else { Some(w) })
    }
    /// A bank of sequences for a grid (C = 1) or pattern (C = 8 gate channels) sequencer: `states` is `[n][C][64]` step states (0 none, 1 on,
    /// 2 hold, as `set_step`), `values` the grid's `[n][64]` note indices (None: all 0; unused by a pattern sequencer), `lengths` `[n]` in
    /// 1..=64 (`srack_patch_set_sequence_bank`; an empty bank removes it).  Inert until `set_voice_sequences` assigns voices to it.
    pub fn set_sequence_bank(&mut self, module: i32, states: &[u8], values: Option<&[u16]>, lengths: &[i32]) -> Result<(), Error> {
        assert!(states.len() >= lengths.len() * 64 && values.map_or(true, |v| v.len() >= lengths.len() * 64));
        let v = values.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_void);
        check(unsafe { ffi::srack_patch_set_sequence_bank(self.raw, module, states.as_ptr(), v, lengths.as_ptr() as *const c_int, lengths.len() as u32) }).map(|_| ())
    }
    /// `(states [n][channels][64], values [n][64], lengths [n])` of the bank, `channels` = 1 for a grid and 8 for a pattern sequencer; empty
    /// without a bank.
    pub fn get_sequence_bank(&self, module: i32, channels: usize) -> Result<(Vec<u8>, Vec<u16>, Vec<i32>), Error> {
        let n = check(unsafe { ffi::srack_patch_get_sequence_bank(self.raw, module, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), 0) })? as usize;
        let (mut s, mut v, mut l) = (vec![0u8; n * channels * 64], vec![0u16; n * 64], vec![0 as c_int; n]);
        check(unsafe { ffi::srack_patch_get_sequence_bank(self.raw, module, s.as_mut_ptr(), v.as_mut_ptr() as *mut c_void, l.as_mut_ptr(), n as u32) })?;
        Ok((s, v, l))
    }
    /// Which sequence of the bank every voice plays: `seq[v]` in `0 .. n_sequences` or `SEQ_OWN` (the module's own cells and length); None
    /// clears.  An edit of cells, not a load: under `keep_state` every voice's step and held CV carry over (`srack_voices_set_sequences`).
    pub fn set_voice_sequences(&mut self, module: i32, seq: Option<&[i32]>) -> Result<(), Error> {
        let q = seq.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        check(unsafe { ffi::srack_voices_set_sequences(self.raw, module, q) }).map(|_| ())
    }
    /// The assignment, `n_voices` entries; None when none is set.
    pub fn get_voice_sequences(&self, module: i32, n_voices: usize) -> Result<Option<Vec<i32>>, Error> {
        let mut q = vec![0 as c_int; n_voices];
        let n = check(unsafe { ffi::srack_voices_get_sequences(self.raw, module, q.as_mut_ptr(), n_voices as u32) })?;
        Ok(if n == 0 { None } else { Some(q) })
    }
    /// `execute_batch` plus one weighted mix per bus: `bus_mix` is `[n_buses][channels][n_samples]` f32, written by the call
    /// (`srack_render_buses`); frames, mix and statistics may each be None.
    pub fn execute_batch_buses(&mut self, n_samples: u32, frames: Option<&DeviceBuffer>, mix: Option<&DeviceBuffer>, stats: Option<&DeviceBuffer>,
                               bus_mix: &DeviceBuffer, flags: u32) -> Result<(), Error> {
        let f = frames.map_or(std::ptr::null_mut(), |b| b.as_f32());
        let m = mix.map_or(std::ptr::null_mut(), |b| b.as_f32());
        let s = stats.map_or(std::ptr::null_mut(), |b| b.as_f64());
        check(unsafe { ffi::srack_render_buses(self.raw, n_samples, f, m, s, bus_mix.as_f32(), flags, std::ptr::null_mut()) }).map(|_| ())
    }
    /// A stereo Freeverb per mix bus, behind the mixer (`srack_buses_set_reverb`): `params` is `[n_buses][6]` f64 in FreeverbModule's field
    /// order — dampening, freeze, wet, width, room size, dry; None: the module's defaults — and `enabled` `[n_buses]` (None: every bus).
    /// Calling it again is the slider: the coefficients change, the tails stay.  Not part of the program: restarts nothing.
    pub fn set_bus_reverbs(&mut self, params: Option<&[f64]>, enabled: Option<&[i32]>) -> Result<(), Error> {
        let a = params.map_or(std::ptr::null(), |x| x.as_ptr());
        let e = enabled.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        check(unsafe { ffi::srack_buses_set_reverb(self.raw, a, e) }).map(|_| ())
    }
    /// `(params [n_buses][6], enabled [n_buses])` of the reverbs set; None when none are.
    pub fn get_bus_reverbs(&self) -> Result<Option<(Vec<f64>, Vec<i32>)>, Error> {
        let n = check(unsafe { ffi::srack_buses_get_reverb(self.raw, std::ptr::null_mut(), std::ptr::null_mut(), 0) })? as usize;
        if n == 0 {
            return Ok(None);
        }
        let (mut a, mut e) = (vec![0f64; n * 6], vec![0 as c_int; n]);
        check(unsafe { ffi::srack_buses_get_reverb(self.raw, a.as_mut_ptr(), e.as_mut_ptr(), n as u32) })?;
        Ok(Some((a, e)))
    }
    /// Delay lines and filter states to zero, the sample counter to 0; the parameters stay.
    pub fn reset_bus_reverbs(&mut self) -> Result<(), Error> {
        check(unsafe { ffi::srack_buses_reset_reverb(self.raw) }).map(|_| ())
    }
    /// `(the 24 line lengths at the patch's sample rate, the samples the kernel takes at a time)`.
    pub fn bus_reverb_plan(&self) -> Result<([i32; 24], i32), Error> {
        let (mut l, mut b) = ([0 as c_int; 24], 0 as c_int);
        check(unsafe { ffi::srack_buses_reverb_plan(self.raw, l.as_mut_ptr(), &mut b) })?;
        Ok((l, b))
    }
    /// The bus mixes through their reverbs: `bus_mix` `[n_buses][channels][n_samples]` f32 in, `bus_fx` `[n_buses][2][n_samples]` f32 out, two
    /// buffers that do not overlap (`srack_buses_reverb`).  A sharded host reduces the per-rank bus mixes first (`MixComm::reduce_mix`) and
    /// reverberates on the root: the reverb of a sum is not, bit for bit, the sum of reverbs.
    pub fn bus_reverb(&mut self, n_samples: u32, bus_mix: &DeviceBuffer, bus_fx: &DeviceBuffer) -> Result<(), Error> {
        check(unsafe { ffi::srack_buses_reverb(self.raw, n_samples, bus_mix.as_f32() as *const f32, bus_fx.as_f32(), std::ptr::null_mut()) }).map(|_| ())
    }
    /// The master section's gains (`srack_buses_set_master`): `[n_buses][2]` f32, a gain per bus and channel, any f32; None: 1.0 everywhere.
    /// Not part of the program: restarts nothing, and the gains survive an edit of the patch.
    pub fn set_master(&mut self, gain: Option<&[f32]>) -> Result<(), Error> {
        check(unsafe { ffi::srack_buses_set_master(self.raw, gain.map_or(std::ptr::null(), |x| x.as_ptr())) }).map(|_| ())
    }
    /// The gains set, `[n_buses][2]`; None when none are (the master then runs with 1.0 everywhere).
    pub fn get_master(&self) -> Result<Option<Vec<f32>>, Error> {
        let n = check(unsafe { ffi::srack_buses_get_master(self.raw, std::ptr::null_mut(), 0) })? as usize;
        if n == 0 {
            return Ok(None);
        }
        let mut g = vec![0f32; n * 2];
        check(unsafe { ffi::srack_buses_get_master(self.raw, g.as_mut_ptr(), n as u32) })?;
        Ok(Some(g))
    }
    /// The buses summed to one stereo pair (`srack_buses_master`): `rows` `[n_buses][row_channels][n_samples]` f32 in — what `bus_reverb`
    /// (2 row channels) or `execute_batch_buses` (the patch's channels) wrote —, `master` `[2][n_samples]` f32 out, `stats`
    /// `[2][STAT_COUNT]` f64 added to.  The order of the additions depends on `n_buses` alone: runs of 64 buses, blocks of 64 runs.  A sharded
    /// host reduces the per-rank bus mixes first, reverberates on the root and takes the master there.
    pub fn master(&mut self, n_samples: u32, rows: &DeviceBuffer, row_channels: u32, master: &DeviceBuffer, stats: Option<&DeviceBuffer>) -> Result<(), Error> {
        let s = stats.map_or(std::ptr::null_mut(), |b| b.as_f64());
        check(unsafe { ffi::srack_buses_master(self.raw, n_samples, rows.as_f32() as *const f32, row_channels, master.as_f32(), s, std::ptr::null_mut()) }).map(|_| ())
    }
    /// The bus sends (`srack_buses_set_sends`): send `i` adds `gain[i][c] * rows[src[i]][c]` to bus `dst[i]`, and every bus keeps its own
    /// row times `through[b][c]` — `gain` `[n_sends][2]`, `through` `[n_buses][2]`, any f32; None: 1.0 everywhere.  An empty list removes
    /// the sends.  Not part of the program: restarts nothing, and the sends survive an edit of the patch.
    pub fn set_sends(&mut self, src: &[i32], dst: &[i32], gain: Option<&[f32]>, through: Option<&[f32]>) -> Result<(), Error> {
        assert_eq!(src.len(), dst.len());
        assert!(gain.map_or(true, |g| g.len() == 2 * src.len()));
        check(unsafe {
            ffi::srack_buses_set_sends(self.raw, src.len() as u32, src.as_ptr(), dst.as_ptr(), gain.map_or(std::ptr::null(), |x| x.as_ptr()),
                                       through.map_or(std::ptr::null(), |x| x.as_ptr()))
        })
        .map(|_| ())
    }
    /// The sends set: `(src, dst, gain [n_sends][2], through [n_buses][2])`; None when none are.
    pub fn get_sends(&self) -> Result<Option<(Vec<i32>, Vec<i32>, Vec<f32>, Vec<f32>)>, Error> {
        let n = check(unsafe { ffi::srack_buses_get_sends(self.raw, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), 0, std::ptr::null_mut(), 0) })? as usize;
        if n == 0 {
            return Ok(None);
        }
        let nb = check(unsafe { ffi::srack_voices_get_buses(self.raw, std::ptr::null_mut(), std::ptr::null_mut(), 0) })? as usize;
        let (mut s, mut d, mut g, mut t) = (vec![0i32; n], vec![0i32; n], vec![0f32; n * 2], vec![0f32; nb * 2]);
        check(unsafe { ffi::srack_buses_get_sends(self.raw, s.as_mut_ptr(), d.as_mut_ptr(), g.as_mut_ptr(), n as u32, t.as_mut_ptr(), nb as u32) })?;
        Ok(Some((s, d, g, t)))
    }
    /// How the list is laid out (`srack_buses_send_plan`): the terms of every bus (through term included), the send indices grouped by
    /// destination ascending, and the number of runs; None when no sends are set.
    pub fn send_plan(&self) -> Result<Option<(Vec<i32>, Vec<i32>, u32)>, Error> {
        let n = check(unsafe { ffi::srack_buses_get_sends(self.raw, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), 0, std::ptr::null_mut(), 0) })? as usize;
        if n == 0 {
            return Ok(None);
        }
        let nb = check(unsafe { ffi::srack_voices_get_buses(self.raw, std::ptr::null_mut(), std::ptr::null_mut(), 0) })? as usize;
        let (mut terms, mut order) = (vec![0i32; nb], vec![0i32; n]);
        let runs = check(unsafe { ffi::srack_buses_send_plan(self.raw, terms.as_mut_ptr(), nb as u32, order.as_mut_ptr(), n as u32) })?;
        Ok(Some((terms, order, runs as u32)))
    }
    /// One level of routing (`srack_buses_send`): `rows` `[n_buses][row_channels][n_samples]` f32 in — what `execute_batch_buses` wrote —,
    /// `out` of the same shape written (channels 0 and 1; no overlap), ready for `bus_reverb` and `master`.  Per destination the master's
    /// order of additions over its terms, a function of the send list alone.  A sharded host reduces the per-rank bus mixes first and
    /// sends on the root.
    pub fn send(&mut self, n_samples: u32, rows: &DeviceBuffer, row_channels: u32, out: &DeviceBuffer) -> Result<(), Error> {
        check(unsafe { ffi::srack_buses_send(self.raw, n_samples, rows.as_f32() as *const f32, row_channels, out.as_f32(), std::ptr::null_mut()) }).map(|_| ())
    }
    /// A Moog ladder per mix bus, behind the mixer (`srack_buses_set_filter`): `params` is `[n_buses][3]` f32 — frequency, resonance, CV
    /// amount, any f32; None: the module's defaults 0.2, 0.5, 0.5 —, `port` `[n_buses]` 0 lowpass, 1 bandpass, 2 highpass (None: lowpass),
    /// `enabled` `[n_buses]` (None: every bus).  Calling it again is the slider: parameters change, state stays.  Not part of the
    /// program: restarts nothing, and the filters carry on across an edit of the patch.
    pub fn set_bus_filter(&mut self, params: Option<&[f32]>, port: Option<&[i32]>, enabled: Option<&[i32]>) -> Result<(), Error> {
        let a = params.map_or(std::ptr::null(), |x| x.as_ptr());
        let o = port.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        let e = enabled.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        check(unsafe { ffi::srack_buses_set_filter(self.raw, a, o, e) }).map(|_| ())
    }
    /// `(params [n_buses][3], port [n_buses], enabled [n_buses])` of the filters set; None when none are.
    pub fn get_bus_filter(&self) -> Result<Option<(Vec<f32>, Vec<i32>, Vec<i32>)>, Error> {
        let n = check(unsafe { ffi::srack_buses_get_filter(self.raw, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), 0) })? as usize;
        if n == 0 {
            return Ok(None);
        }
        let (mut a, mut o, mut e) = (vec![0f32; n * 3], vec![0 as c_int; n], vec![0 as c_int; n]);
        check(unsafe { ffi::srack_buses_get_filter(self.raw, a.as_mut_ptr(), o.as_mut_ptr(), e.as_mut_ptr(), n as u32) })?;
        Ok(Some((a, o, e)))
    }
    /// Every filter's state to zero; the parameters stay.
    pub fn reset_bus_filter(&mut self) -> Result<(), Error> {
        check(unsafe { ffi::srack_buses_reset_filter(self.raw) }).map(|_| ())
    }
    /// The filters' state behind the last call, `[n_buses][2][10]` f32: f, p, q, b0 .. b4 and the (frequency, resonance) the coefficients
    /// were computed for, per bus and channel; a disabled bus reads as zeros.
    pub fn bus_filter_state(&mut self) -> Result<Vec<f32>, Error> {
        let n = check(unsafe { ffi::srack_buses_filter_state(self.raw, std::ptr::null_mut(), 0) })? as usize;
        let mut st = vec![0f32; n * 2 * 10];
        check(unsafe { ffi::srack_buses_filter_state(self.raw, st.as_mut_ptr(), n as u32) })?;
        Ok(st)
    }
    /// The bus rows through their filters (`srack_buses_filter`): `rows` `[n_buses][row_channels][n_samples]` f32 in, `cv`
    /// `[n_buses][n_samples]` f32 (None: the CV port unconnected), `out` of the shape of `rows` written — None: in place.  Channels 0 and 1
    /// are filtered; a disabled bus passes bit for bit.  A sharded host reduces the per-rank bus mixes first and filters on the root:
    /// a ladder on a sum is not the sum of ladders.
    pub fn bus_filter(&mut self, n_samples: u32, rows: &DeviceBuffer, row_channels: u32, cv: Option<&DeviceBuffer>, out: Option<&DeviceBuffer>) -> Result<(), Error> {
        let c = cv.map_or(std::ptr::null(), |b| b.as_f32() as *const f32);
        let o = out.map_or(rows.as_f32(), |b| b.as_f32());
        check(unsafe { ffi::srack_buses_filter(self.raw, n_samples, rows.as_f32() as *const f32, row_channels, c, o, std::ptr::null_mut()) }).map(|_| ())
    }
    /// An ADSR and a VCA per mix bus, behind the mixer (`srack_buses_set_vca`): `params` is `[n_buses][4]` f32 — attack, decay (seconds),
    /// sustain level, release (seconds), any f32; None: the module's defaults 0, 0.5, 0.25, 0.5 —, `mode` `[n_buses]` 0 off, 1 the control
    /// row is the VCA's CV, 2 it is the envelope's gate (None: every bus gated), `negative` `[n_buses]` the VCAs' flag (None: false).
    /// Calling it again is the slider: sliders change, state stays; a bus that becomes gated starts fresh.  Not part of the program:
    /// restarts nothing, and the envelopes carry on across an edit of the patch.
    pub fn set_bus_vca(&mut self, params: Option<&[f32]>, mode: Option<&[i32]>, negative: Option<&[i32]>) -> Result<(), Error> {
        let a = params.map_or(std::ptr::null(), |x| x.as_ptr());
        let m = mode.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        let g = negative.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        check(unsafe { ffi::srack_buses_set_vca(self.raw, a, m, g) }).map(|_| ())
    }
    /// `(params [n_buses][4], mode [n_buses], negative [n_buses])` of the VCAs set; None when none are.
    pub fn get_bus_vca(&self) -> Result<Option<(Vec<f32>, Vec<i32>, Vec<i32>)>, Error> {
        let n = check(unsafe { ffi::srack_buses_get_vca(self.raw, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), 0) })? as usize;
        if n == 0 {
            return Ok(None);
        }
        let (mut a, mut m, mut g) = (vec![0f32; n * 4], vec![0 as c_int; n], vec![0 as c_int; n]);
        check(unsafe { ffi::srack_buses_get_vca(self.raw, a.as_mut_ptr(), m.as_mut_ptr(), g.as_mut_ptr(), n as u32) })?;
        Ok(Some((a, m, g)))
    }
    /// Every envelope's state fresh (mode None, the gate detector armed as at `new()`); the setting stays.
    pub fn reset_bus_vca(&mut self) -> Result<(), Error> {
        check(unsafe { ffi::srack_buses_reset_vca(self.raw) }).map(|_| ())
    }
    /// The envelopes' state behind the last call, `[n_buses][6]` f32: phase, mode, r_val, from_a_val, the f32 sample rate, gate_last; a
    /// bus that is not gated reads as the fresh state (0, 4, 0, 0, rate, 1).
    pub fn bus_vca_state(&mut self) -> Result<Vec<f32>, Error> {
        let n = check(unsafe { ffi::srack_buses_vca_state(self.raw, std::ptr::null_mut(), 0) })? as usize;
        let mut st = vec![0f32; n * 6];
        check(unsafe { ffi::srack_buses_vca_state(self.raw, st.as_mut_ptr(), n as u32) })?;
        Ok(st)
    }
    /// The bus rows through their VCAs (`srack_buses_vca`): `rows` `[n_buses][row_channels][n_samples]` f32 in, `ctl`
    /// `[n_buses][n_samples]` f32 the gate or CV per bus (None: the control port unconnected), `out` of the shape of `rows` written — None:
    /// in place —, `env` `[n_buses][n_samples]` written when given: the envelopes, e.g. as the `cv` of `bus_filter`.  Channels 0 and 1 are
    /// processed; a bus that is off passes word for word.
    pub fn bus_vca(&mut self, n_samples: u32, rows: &DeviceBuffer, row_channels: u32, ctl: Option<&DeviceBuffer>, out: Option<&DeviceBuffer>, env: Option<&DeviceBuffer>) -> Result<(), Error> {
        let c = ctl.map_or(std::ptr::null(), |b| b.as_f32() as *const f32);
        let o = out.map_or(rows.as_f32(), |b| b.as_f32());
        let e = env.map_or(std::ptr::null_mut(), |b| b.as_f32());
        check(unsafe { ffi::srack_buses_vca(self.raw, n_samples, rows.as_f32() as *const f32, row_channels, c, o, e, std::ptr::null_mut()) }).map(|_| ())
    }
    /// An LFO per mix bus writes the console's control rows (`srack_buses_set_osc`): `params` is `[n_buses][3]` f32 — val (1 V/oct, 0 is
    /// 440 Hz), depth, offset, any f32; None: 0, 1, 0 —, `port` `[n_buses]` 0 sine, 1 square, 2 sawtooth (None: sine), `antialiasing`
    /// `[n_buses]` (None: true), `enabled` `[n_buses]` (None: all).  The reference's oscillator bit for bit, times depth, plus offset.
    /// Calling it again is the slider: state stays; a bus that becomes enabled starts fresh.  Not part of the program: restarts nothing.
    pub fn set_bus_osc(&mut self, params: Option<&[f32]>, port: Option<&[i32]>, antialiasing: Option<&[i32]>, enabled: Option<&[i32]>) -> Result<(), Error> {
        let a = params.map_or(std::ptr::null(), |x| x.as_ptr());
        let po = port.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        let aa = antialiasing.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        let e = enabled.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        check(unsafe { ffi::srack_buses_set_osc(self.raw, a, po, aa, e) }).map(|_| ())
    }
    /// `(params [n_buses][3], port [n_buses], antialiasing [n_buses], enabled [n_buses])` of the oscillators set; None when none are.
    pub fn get_bus_osc(&self) -> Result<Option<(Vec<f32>, Vec<i32>, Vec<i32>, Vec<i32>)>, Error> {
        let null = std::ptr::null_mut::<c_int>();
        let n = check(unsafe { ffi::srack_buses_get_osc(self.raw, std::ptr::null_mut(), null, null, null, 0) })? as usize;
        if n == 0 {
            return Ok(None);
        }
        let (mut a, mut po, mut aa, mut e) = (vec![0f32; n * 3], vec![0 as c_int; n], vec![0 as c_int; n], vec![0 as c_int; n]);
        check(unsafe { ffi::srack_buses_get_osc(self.raw, a.as_mut_ptr(), po.as_mut_ptr(), aa.as_mut_ptr(), e.as_mut_ptr(), n as u32) })?;
        Ok(Some((a, po, aa, e)))
    }
    /// Every oscillator's state fresh (phase 0, the sync detector armed as at `new()`), or, with `pos` `[n_buses]` f64, each in `[0, 1)`
    /// and not -0.0, bus b at phase `pos[b]`; the setting stays.
    pub fn reset_bus_osc(&mut self, pos: Option<&[f64]>) -> Result<(), Error> {
        check(unsafe { ffi::srack_buses_reset_osc(self.raw, pos.map_or(std::ptr::null(), |x| x.as_ptr())) }).map(|_| ())
    }
    /// The oscillators' state behind the last call, `[n_buses][2]` f64: phase, sync last (0.0 / 1.0); a disabled bus reads fresh (0, 1).
    pub fn bus_osc_state(&mut self) -> Result<Vec<f64>, Error> {
        let n = check(unsafe { ffi::srack_buses_osc_state(self.raw, std::ptr::null_mut(), 0) })? as usize;
        let mut st = vec![0f64; n * 2];
        check(unsafe { ffi::srack_buses_osc_state(self.raw, st.as_mut_ptr(), n as u32) })?;
        Ok(st)
    }
    /// `n_samples` of every bus's oscillator (`srack_buses_osc`): `cv` and `sync` `[n_buses][n_samples]` f32 (None: the port is
    /// unconnected), `out` `[n_buses][n_samples]` f32 written — what `bus_filter`'s `cv`, `bus_vca`'s `ctl` and `bus_shaper`'s `cv` take.
    /// A disabled bus's row is +0.0.
    pub fn bus_osc(&mut self, n_samples: u32, cv: Option<&DeviceBuffer>, sync: Option<&DeviceBuffer>, out: &DeviceBuffer) -> Result<(), Error> {
        let c = cv.map_or(std::ptr::null(), |b| b.as_f32() as *const f32);
        let g = sync.map_or(std::ptr::null(), |b| b.as_f32() as *const f32);
        check(unsafe { ffi::srack_buses_osc(self.raw, n_samples, c, g, out.as_f32(), std::ptr::null_mut()) }).map(|_| ())
    }
    /// A drive, a waveshaper and a make-up gain per mix bus, behind the mixer (`srack_buses_set_shaper`): `params` is `[n_buses][3]` f32 —
    /// pre, exponent, post, any f32; None: 1, 1, 1 —, `mode` `[n_buses]` 0 off, 1 the exponent is the constant, 2 it is the bus's CV row
    /// (None: every bus constant).  `sign(a) |a|^e` with the host libm's `powf`, bit for bit.  Calling it again is the slider; there is no
    /// state.  Not part of the program: restarts nothing.
    pub fn set_bus_shaper(&mut self, params: Option<&[f32]>, mode: Option<&[i32]>) -> Result<(), Error> {
        let a = params.map_or(std::ptr::null(), |x| x.as_ptr());
        let m = mode.map_or(std::ptr::null(), |x| x.as_ptr() as *const c_int);
        check(unsafe { ffi::srack_buses_set_shaper(self.raw, a, m) }).map(|_| ())
    }
    /// `(params [n_buses][3], mode [n_buses])` of the shapers set; None when none are.
    pub fn get_bus_shaper(&self) -> Result<Option<(Vec<f32>, Vec<i32>)>, Error> {
        let n = check(unsafe { ffi::srack_buses_get_shaper(self.raw, std::ptr::null_mut(), std::ptr::null_mut(), 0) })? as usize;
        if n == 0 {
            return Ok(None);
        }
        let (mut a, mut m) = (vec![0f32; n * 3], vec![0 as c_int; n]);
        check(unsafe { ffi::srack_buses_get_shaper(self.raw, a.as_mut_ptr(), m.as_mut_ptr(), n as u32) })?;
        Ok(Some((a, m)))
    }
    /// The bus rows through their shapers (`srack_buses_shaper`): `rows` `[n_buses][row_channels][n_samples]` f32 in, `cv`
    /// `[n_buses][n_samples]` f32 the exponent of a CV bus sample by sample (None: its constant), `out` of the shape of `rows` written —
    /// None: in place.  Channels 0 and 1 are processed; a bus that is off passes word for word.
    pub fn bus_shaper(&mut self, n_samples: u32, rows: &DeviceBuffer, row_channels: u32, cv: Option<&DeviceBuffer>, out: Option<&DeviceBuffer>) -> Result<(), Error> {
        let c = cv.map_or(std::ptr::null(), |b| b.as_f32() as *const f32);
        let o = out.map_or(rows.as_f32(), |b| b.as_f32());
        check(unsafe { ffi::srack_buses_shaper(self.raw, n_samples, rows.as_f32() as *const f32, row_channels, c, o, std::ptr::null_mut()) }).map(|_| ())
    }
    /// The bus meters (`srack_buses_meter`), a read-only tap on bus rows: `rows` `[n_buses][row_channels][n_samples]` f32 are positions
    /// `first_sample ..` of a stream the caller counts; `levels` `(buffer, window, n_windows)` is f64
    /// `[n_windows][6][n_buses][2]`, record `k` covering `[k * window, (k + 1) * window)`; `totals` is f64 `[6][n_buses][2]`.  Both are
    /// added to: zero-fill once, cut the stream into calls at will.  One of the two must be given.
    pub fn bus_meter(&mut self, first_sample: u64, n_samples: u32, rows: &DeviceBuffer, row_channels: u32, levels: Option<(&DeviceBuffer, u32, u32)>, totals: Option<&DeviceBuffer>) -> Result<(), Error> {
        let (l, window, n_windows) = levels.map_or((std::ptr::null_mut(), 0, 0), |(b, w, n)| (b.as_f64(), w, n));
        let t = totals.map_or(std::ptr::null_mut(), |b| b.as_f64());
        check(unsafe { ffi::srack_buses_meter(self.raw, first_sample, n_samples, rows.as_f32() as *const f32, row_channels, window, l, n_windows, t, std::ptr::null_mut()) }).map(|_| ())
    }
}

impl Drop for Patch {
    fn drop(&mut self) {
        unsafe { ffi::srack_patch_destroy(self.raw) };
    }
}

pub fn abi_version() -> i32 {
    unsafe { ffi::srack_abi_version() }
}

/// The multi-GPU half: one process per GPU, voices sharded by global voice index, and ONE collective — the RCCL sum of the
/// per-rank partial mixes.  (No reference counterpart: s-rack is single-threaded, src/main.rs:59-63.)
/// Rank 0 makes the id; the host carries its 128 bytes to every rank; every rank calls `MixComm::new` with its device selected.
pub struct MixComm {
    raw: *mut c_void,
}

impl MixComm {
    pub fn unique_id() -> Result<[u8; DIST_ID_BYTES], Error> {
        let mut id = [0u8; DIST_ID_BYTES];
        check(unsafe { ffi::srack_dist_unique_id(id.as_mut_ptr()) })?;
        Ok(id)
    }
    pub fn new(id: &[u8; DIST_ID_BYTES], n_ranks: i32, rank: i32) -> Result<Self, Error> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::srack_dist_init(id.as_ptr(), n_ranks, rank, &mut raw) })?;
        Ok(MixComm { raw })
    }
    pub fn count(&self) -> Result<i32, Error> {
        let mut n = 0;
        check(unsafe { ffi::srack_dist_comm_count(self.raw, &mut n) })?;
        Ok(n)
    }
    /// ncclReduce(sum, f32) of the `[channels][n_samples]` partial mix, in place, on the default stream.
    pub fn reduce_mix(&self, mix: &DeviceBuffer, count: usize, root: i32) -> Result<(), Error> {
        check(unsafe { ffi::srack_dist_reduce_mix(self.raw, mix.as_f32(), count, root, std::ptr::null_mut()) }).map(|_| ())
    }
}

impl Drop for MixComm {
    fn drop(&mut self) {
        unsafe { ffi::srack_dist_destroy(self.raw) };
    }
}

#[cfg(test)]
mod tests {
    use super::*;

    /// oscillator::dco_tests::produces_440 (src/synth/oscillator.rs:284-305) through the GPU path.
    #[test]
    fn produces_440() {
        let mut p = Patch::new(440 * 4, 17, 2).unwrap();
        let osc = p.add_module(ModuleType::Oscillator).unwrap();
        let out = p.add_module(ModuleType::Output).unwrap();
        p.set_input(out, 0, osc, 0).unwrap();
        p.configure_voices(1).unwrap();
        let frames = DeviceBuffer::new(17 * 4).unwrap();
        let mut buf = [0f32; 17];
        p.execute_batch(17, Some(&frames), None, 0).unwrap();
        frames.to_host(&mut buf).unwrap();
        assert_eq!(buf[0], 0.0);
        assert!((buf[1] - 1.0).abs() < 0.00001);
        assert!(buf[2].abs() < 0.00001);
        assert!((buf[3] + 1.0).abs() < 0.00001);
        assert!(buf[4].abs() < 0.00001);
        p.execute_batch(17, Some(&frames), None, 0).unwrap();
        frames.to_host(&mut buf).unwrap();
        assert!((buf[0] - 1.0).abs() < 0.00001); // should continue smoothly into next buffer
    }
}
