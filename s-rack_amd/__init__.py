"""srack_amd — host-side binding of the MI355X batch-render path (libsrack_hip.so, C ABI in include/srack_hip.h).

This module is only a ctypes binding plus a thin `Patch` class whose methods carry the reference's
names (`add_module`, `set_input`/`connect`, `plan_execution` -> `plan`, `execute` -> `render`).
All computation happens in the HIP library; there is NO CPU fallback: if the shared library is
missing the import fails, and a render on a host without a GPU returns SRACK_ERR_DEVICE.
"""
import ctypes as C
import os

import numpy as np

from . import workloads  # noqa: F401  (patch builders; pure Python)
from .workloads import *  # noqa: F401,F403  (module / field / port enums)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsrack_hip.so")

OK, ERR_INVALID, ERR_PORT, ERR_NO_OUTPUT, ERR_SELF_LOOP, ERR_STATE, ERR_UNSUPPORTED, ERR_DEVICE, ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6, -7, -8
MAX_BUSES, BUS_NONE = 65536, -1
MAX_VOICE_SLOTS = 4  # srack_voices_set_bus_slots: the most buses a voice can feed
MASTER_RUN, MASTER_BLOCK = 64, 64  # buses per run, runs per block: the order srack_buses_master adds in
MAX_SENDS = 1048576  # srack_buses_set_sends: the longest send list
BUS_FILTER_NPARAMS, BUS_FILTER_NSTATE = 3, 10  # srack_buses_set_filter: FREQ, RES, EXP_AMT per bus; srack_buses_filter_state: VCF_ST_F .. VCF_ST_RES per bus and channel
BUS_FILTER_DEFAULTS = (0.2, 0.5, 0.5)  # MoogFilterModule's three sliders: what set_bus_filter(None) gives every bus
BUS_VCA_NPARAMS, BUS_VCA_NSTATE = 4, 6  # srack_buses_set_vca: ADSR_A_SEC .. ADSR_R_SEC per bus; srack_buses_vca_state: ADSR_PHASE .. ADSR_GATE_LAST per bus
BUS_VCA_OFF, BUS_VCA_CV, BUS_VCA_GATE = 0, 1, 2  # a bus's mode: it passes; its control row is the VCAs' CV; it is the gate of the bus's ADSR
BUS_VCA_DEFAULTS = (0.0, 0.5, 0.25, 0.5)  # ADSRModule's four sliders: what set_bus_vca(None) gives every bus
BUS_OSC_NPARAMS, BUS_OSC_NSTATE = 3, 2  # srack_buses_set_osc: VAL, DEPTH, OFFSET per bus; srack_buses_osc_state: OSC_POS, OSC_SYNC_LAST per bus, as f64
BUS_OSC_VAL, BUS_OSC_DEPTH, BUS_OSC_OFFSET = 0, 1, 2
BUS_OSC_DEFAULTS = (0.0, 1.0, 0.0)  # the oscillator's val, a gain of 1, an offset of 0: what set_bus_osc(None) gives every bus
BUS_SHAPER_NPARAMS = 3  # srack_buses_set_shaper: PRE, EXPONENT, POST per bus
BUS_SHAPER_PRE, BUS_SHAPER_EXPONENT, BUS_SHAPER_POST = 0, 1, 2
BUS_SHAPER_OFF, BUS_SHAPER_CONST, BUS_SHAPER_CV = 0, 1, 2  # a bus's mode: it passes; the exponent is EXPONENT; the exponent is the bus's CV row
BUS_SHAPER_DEFAULTS = (1.0, 1.0, 1.0)  # drive, exponent, make-up gain: what set_bus_shaper(None) gives every bus
BUS_METER_MIN_WINDOW = 64  # srack_buses_meter: the shortest window of a level track, in samples
ADSR_MODE_ATTACK, ADSR_MODE_DECAY, ADSR_MODE_SUSTAIN, ADSR_MODE_RELEASE, ADSR_MODE_NONE = 0, 1, 2, 3, 4  # the values of ADSR_MODE
FREEVERB_DEFAULTS = (0.5, 0.0, 1.0, 0.5, 0.5, 0.0)  # FreeverbModule's six parameters in field order: what set_bus_reverbs(None) gives every bus
WAVE_OWN = -1
SEQ_OWN, MAX_SEQUENCES = -1, 65536
STAT_SUM, STAT_SUM_SQ, STAT_PEAK_POS, STAT_PEAK_NEG, STAT_NONFINITE, STAT_CLIPPED, STAT_COUNT = 0, 1, 2, 3, 4, 5, 6
RENDER_DEFAULT, RENDER_EXACT_OSC, RENDER_NO_FUSION, RENDER_NO_UNIFORM_HOIST, RENDER_NO_CTL_STAGES, RENDER_NO_SPECIALIZE, RENDER_SPECIALIZE, RENDER_KEEP_DEFAULT = 0, 1, 2, 4, 8, 16, 32, 64

# every symbol include/srack_hip.h declares (tests check the library exports exactly these)
ABI_SYMBOLS = [
    "srack_abi_version", "srack_last_error", "srack_patch_create", "srack_patch_destroy", "srack_patch_add_module",
    "srack_patch_num_modules", "srack_patch_module_type", "srack_module_num_inputs", "srack_module_num_outputs",
    "srack_patch_set_field", "srack_patch_get_field", "srack_patch_keep_state", "srack_patch_set_step", "srack_patch_get_step", "srack_patch_set_wave", "srack_patch_get_wave", "srack_patch_load_srk", "srack_patch_save_srk", "srack_patch_module_id",
    "srack_patch_set_module_position", "srack_patch_get_module_position", "srack_patch_set_output_buffer", "srack_patch_get_output_buffer", "srack_patch_set_noise_seed", "srack_patch_connect", "srack_patch_disconnect", "srack_patch_get_input",
    "srack_patch_plan", "srack_patch_plan_list", "srack_patch_removed_edges", "srack_patch_delayed_edges",
    "srack_voices_configure", "srack_voices_set_field_f32", "srack_voices_set_field_f64", "srack_render_planes", "srack_render", "srack_render_stats", "srack_render_reserve",
    "srack_voices_set_buses", "srack_voices_get_buses", "srack_voices_bus_plan", "srack_render_buses",
    "srack_voices_set_bus_slots", "srack_voices_get_bus_slots",
    "srack_buses_set_reverb", "srack_buses_get_reverb", "srack_buses_reset_reverb", "srack_buses_reverb_plan", "srack_buses_reverb",
    "srack_buses_set_master", "srack_buses_get_master", "srack_buses_master",
    "srack_buses_set_sends", "srack_buses_get_sends", "srack_buses_send_plan", "srack_buses_send",
    "srack_buses_set_filter", "srack_buses_get_filter", "srack_buses_reset_filter", "srack_buses_filter_state", "srack_buses_filter",
    "srack_buses_set_vca", "srack_buses_get_vca", "srack_buses_reset_vca", "srack_buses_vca_state", "srack_buses_vca",
    "srack_buses_set_shaper", "srack_buses_get_shaper", "srack_buses_shaper",
    "srack_buses_meter",
    "srack_buses_set_osc", "srack_buses_get_osc", "srack_buses_reset_osc", "srack_buses_osc_state", "srack_buses_osc",
    "srack_patch_set_wave_bank", "srack_patch_get_wave_bank", "srack_patch_get_wave_bank_samples", "srack_voices_set_waves", "srack_voices_get_waves",
    "srack_patch_set_sequence_bank", "srack_patch_get_sequence_bank", "srack_voices_set_sequences", "srack_voices_get_sequences",
    "srack_render_info", "srack_render_kernel_source", "srack_render_kernel_compile", "srack_render_kernel_ms", "srack_voices_get_field", "srack_kernel_cache_set_dir", "srack_kernel_cache_stats", "srack_device_count", "srack_device_set", "srack_device_get",
    "srack_device_alloc", "srack_device_free", "srack_device_to_host", "srack_device_from_host", "srack_device_sync",
    "srack_dist_unique_id", "srack_dist_init", "srack_dist_comm_count", "srack_dist_destroy", "srack_dist_reduce_mix",
]


class KernelCacheInfo(C.Structure):
    """srack_kernel_cache_info (include/srack_hip.h)"""
    _fields_ = [("compiled", C.c_uint64), ("disk_hits", C.c_uint64), ("memory_hits", C.c_uint64), ("modules_loaded", C.c_uint64),
                ("code_evictions", C.c_uint64), ("module_evictions", C.c_uint64), ("resident_code_objects", C.c_uint64),
                ("resident_modules", C.c_uint64), ("compile_ms", C.c_double), ("directory", C.c_char * 512)]


class SrackError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"srack error {code}: {msg}")
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the render path.")
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, dbl, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_double, C.c_size_t
    ip, dp, fp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float)
    L.srack_last_error.restype = C.c_char_p
    L.srack_patch_create.argtypes = [u32, u32, u32, C.POINTER(vp)]
    L.srack_patch_destroy.argtypes = [vp]
    L.srack_patch_add_module.argtypes = [vp, i32]
    L.srack_patch_num_modules.argtypes = [vp]
    L.srack_patch_module_type.argtypes = [vp, i32]
    L.srack_module_num_inputs.argtypes = [vp, i32]
    L.srack_module_num_outputs.argtypes = [vp, i32]
    L.srack_patch_set_field.argtypes = [vp, i32, i32, dbl]
    L.srack_patch_get_field.argtypes = [vp, i32, i32, dp]
    L.srack_patch_set_step.argtypes = [vp, i32, i32, i32, i32, i32]
    L.srack_patch_get_step.argtypes = [vp, i32, i32, i32, ip, ip]
    L.srack_patch_set_wave.argtypes = [vp, i32, fp, u32, C.c_float]
    L.srack_patch_get_wave.argtypes = [vp, i32, fp, u32, fp]
    L.srack_patch_load_srk.argtypes = [C.c_char_p, sz, u32, u32, u32, C.POINTER(vp)]
    L.srack_patch_save_srk.argtypes = [vp, C.c_char_p, sz, C.POINTER(sz)]
    L.srack_patch_module_id.argtypes = [vp, i32, C.c_char_p, sz]
    L.srack_patch_set_module_position.argtypes = [vp, i32, C.c_float, C.c_float]
    L.srack_patch_get_module_position.argtypes = [vp, i32, fp, fp]
    L.srack_patch_set_output_buffer.argtypes = [vp, i32, i32, fp, u32]
    if hasattr(L, "srack_patch_get_output_buffer"):  # (tools/ab.sh alternates older builds of the library under this binding)
        L.srack_patch_get_output_buffer.argtypes = [vp, i32, i32, fp, u32]
    L.srack_patch_set_noise_seed.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.srack_patch_keep_state.argtypes = [vp, i32]
    L.srack_patch_connect.argtypes = [vp, i32, i32, i32, i32]
    L.srack_patch_disconnect.argtypes = [vp, i32, i32]
    L.srack_patch_get_input.argtypes = [vp, i32, i32, ip, ip]
    L.srack_patch_plan.argtypes = [vp, ip, i32]
    L.srack_patch_plan_list.argtypes = [vp, i32, ip, i32, ip, i32]
    L.srack_patch_removed_edges.argtypes = [vp, ip, i32]
    L.srack_patch_delayed_edges.argtypes = [vp, ip, i32]
    L.srack_voices_configure.argtypes = [vp, u32]
    L.srack_voices_set_field_f32.argtypes = [vp, i32, i32, fp]
    L.srack_voices_set_field_f64.argtypes = [vp, i32, i32, dp]
    L.srack_render_planes.argtypes = [vp, ip, i32]
    L.srack_render.argtypes = [vp, u32, vp, vp, u32, vp]
    L.srack_render_stats.argtypes = [vp, u32, vp, vp, vp, u32, vp]
    if hasattr(L, "srack_render_buses"):  # (tools/ alternate older builds of the library under this binding)
        L.srack_voices_set_buses.argtypes = [vp, u32, ip, fp]
        L.srack_voices_get_buses.argtypes = [vp, ip, fp, u32]
        L.srack_voices_bus_plan.argtypes = [vp, ip, u32, ip, u32]
        L.srack_render_buses.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp]
    if hasattr(L, "srack_voices_set_bus_slots"):
        L.srack_voices_set_bus_slots.argtypes = [vp, u32, u32, ip, fp]
        L.srack_voices_get_bus_slots.argtypes = [vp, ip, ip, fp, u32]
    if hasattr(L, "srack_buses_reverb"):
        L.srack_buses_set_reverb.argtypes = [vp, dp, ip]
        L.srack_buses_get_reverb.argtypes = [vp, dp, ip, u32]
        L.srack_buses_reset_reverb.argtypes = [vp]
        L.srack_buses_reverb_plan.argtypes = [vp, ip, ip]
        L.srack_buses_reverb.argtypes = [vp, u32, vp, vp, vp]
    if hasattr(L, "srack_buses_master"):
        L.srack_buses_set_master.argtypes = [vp, fp]
        L.srack_buses_get_master.argtypes = [vp, fp, u32]
        L.srack_buses_master.argtypes = [vp, u32, vp, u32, vp, vp, vp]
    if hasattr(L, "srack_buses_send"):
        L.srack_buses_set_sends.argtypes = [vp, u32, ip, ip, fp, fp]
        L.srack_buses_get_sends.argtypes = [vp, ip, ip, fp, u32, fp, u32]
        L.srack_buses_send_plan.argtypes = [vp, ip, u32, ip, u32]
        L.srack_buses_send.argtypes = [vp, u32, vp, u32, vp, vp]
    if hasattr(L, "srack_buses_filter"):
        L.srack_buses_set_filter.argtypes = [vp, fp, ip, ip]
        L.srack_buses_get_filter.argtypes = [vp, fp, ip, ip, u32]
        L.srack_buses_reset_filter.argtypes = [vp]
        L.srack_buses_filter_state.argtypes = [vp, fp, u32]
        L.srack_buses_filter.argtypes = [vp, u32, vp, u32, vp, vp, vp]
    if hasattr(L, "srack_buses_vca"):
        L.srack_buses_set_vca.argtypes = [vp, fp, ip, ip]
        L.srack_buses_get_vca.argtypes = [vp, fp, ip, ip, u32]
        L.srack_buses_reset_vca.argtypes = [vp]
        L.srack_buses_vca_state.argtypes = [vp, fp, u32]
        L.srack_buses_vca.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp]
    if hasattr(L, "srack_buses_shaper"):
        L.srack_buses_set_shaper.argtypes = [vp, fp, ip]
        L.srack_buses_get_shaper.argtypes = [vp, fp, ip, u32]
        L.srack_buses_shaper.argtypes = [vp, u32, vp, u32, vp, vp, vp]
    if hasattr(L, "srack_buses_meter"):
        L.srack_buses_meter.argtypes = [vp, C.c_uint64, u32, vp, u32, u32, vp, u32, vp, vp]
    if hasattr(L, "srack_buses_osc"):
        L.srack_buses_set_osc.argtypes = [vp, fp, ip, ip, ip]
        L.srack_buses_get_osc.argtypes = [vp, fp, ip, ip, ip, u32]
        L.srack_buses_reset_osc.argtypes = [vp, dp]
        L.srack_buses_osc_state.argtypes = [vp, dp, u32]
        L.srack_buses_osc.argtypes = [vp, u32, vp, vp, vp, vp]
    if hasattr(L, "srack_voices_set_waves"):  # (tools/ alternate older builds of the library under this binding)
        L.srack_patch_set_wave_bank.argtypes = [vp, i32, fp, ip, fp, u32]
        L.srack_patch_get_wave_bank.argtypes = [vp, i32, ip, fp, u32]
        L.srack_patch_get_wave_bank_samples.argtypes = [vp, i32, i32, fp, u32]
        L.srack_voices_set_waves.argtypes = [vp, i32, ip]
        L.srack_voices_get_waves.argtypes = [vp, i32, ip, u32]
    if hasattr(L, "srack_voices_set_sequences"):
        L.srack_patch_set_sequence_bank.argtypes = [vp, i32, vp, vp, ip, u32]
        L.srack_patch_get_sequence_bank.argtypes = [vp, i32, vp, vp, ip, u32]
        L.srack_voices_set_sequences.argtypes = [vp, i32, ip]
        L.srack_voices_get_sequences.argtypes = [vp, i32, ip, u32]
    L.srack_render_reserve.argtypes = [vp, u32, i32, u32]
    L.srack_render_info.argtypes = [vp, C.c_char_p, sz]
    L.srack_render_kernel_ms.argtypes = [vp, dp, ip, i32]
    L.srack_render_kernel_source.argtypes = [vp, u32, C.c_char_p, sz]
    L.srack_render_kernel_compile.argtypes = [vp, u32]
    L.srack_voices_get_field.argtypes = [vp, i32, i32, dp]
    L.srack_kernel_cache_set_dir.argtypes = [C.c_char_p]
    L.srack_kernel_cache_stats.argtypes = [C.POINTER(KernelCacheInfo)]
    L.srack_device_count.argtypes = [ip]
    L.srack_device_set.argtypes = [i32]
    L.srack_device_get.argtypes = [ip, C.c_char_p, sz]
    L.srack_device_alloc.argtypes = [C.POINTER(vp), sz]
    L.srack_device_free.argtypes = [vp]
    L.srack_device_to_host.argtypes = [vp, vp, sz, vp]
    L.srack_device_from_host.argtypes = [vp, vp, sz, vp]
    L.srack_device_sync.argtypes = [vp]
    L.srack_dist_unique_id.argtypes = [C.c_char_p]
    L.srack_dist_init.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
    L.srack_dist_comm_count.argtypes = [vp, ip]
    L.srack_dist_destroy.argtypes = [vp]
    L.srack_dist_reduce_mix.argtypes = [vp, vp, sz, i32, vp]
    return L


lib = _load()


def _check(rc):
    if rc < 0:
        raise SrackError(rc, lib.srack_last_error().decode(errors="replace"))
    return rc


def _opt(a, dtype, shape):
    """An optional array argument -> (the contiguous array of `dtype` or None, its ctypes pointer or None); the shape is asserted.
    The pointer keeps a reference to the array (numpy's data_as), so a caller may hold on to the pointer alone."""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=dtype)
    assert a.shape == shape, a.shape
    return a, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype)))


def _truth(a):
    """an optional array of flags -> where it is not 0, or None"""
    return None if a is None else np.asarray(a) != 0


class DeviceScope:
    """Device buffers for the length of a `with` block (srack_device_*): the one place where a buffer's lifetime is decided.  Addresses
    are plain integers.  Leaving the block normally waits for `stream` and frees everything; leaving it by an exception frees everything
    without a wait.  What srack_device_free says is ignored."""

    def __init__(self, stream=None):
        self.stream, self._owned = stream, []

    def __enter__(self):
        return self

    def alloc(self, nbytes, offset=0):
        """-> the address of nbytes (8 at the least) of device memory, `offset` 4-byte words into an allocation that much larger"""
        d = C.c_void_p()
        _check(lib.srack_device_alloc(C.byref(d), max(8, nbytes) + 4 * offset))
        self._owned.append(d)
        return d.value + 4 * offset

    def upload(self, a, offset=0, stream=None):
        """alloc for the contiguous array `a`, its bytes sent up on `stream` (nothing is sent for 0 bytes) -> the address"""
        d = self.alloc(a.nbytes, offset)
        if a.nbytes:
            _check(lib.srack_device_from_host(d, a.ctypes.data_as(C.c_void_p), a.nbytes, stream))
        return d

    def download(self, a, d):
        """the contiguous array `a` filled from address d on the scope's stream (nothing is fetched for 0 bytes); complete behind the block"""
        if a.nbytes:
            _check(lib.srack_device_to_host(a.ctypes.data_as(C.c_void_p), d, a.nbytes, self.stream))

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None:
                _check(lib.srack_device_sync(self.stream))
        finally:
            for d in self._owned:
                lib.srack_device_free(d)
            self._owned = []
        return False


def device_count():
    n = C.c_int(0)
    lib.srack_device_count(C.byref(n))
    return n.value


def kernel_cache_set_dir(path):
    """The disk level of the specialised-kernel cache: a directory, "off", or None for the default resolution."""
    _check(lib.srack_kernel_cache_set_dir(None if path is None else os.fsencode(path)))


def kernel_cache_stats():
    st = KernelCacheInfo()
    _check(lib.srack_kernel_cache_stats(C.byref(st)))
    d = {k: getattr(st, k) for k, _ in KernelCacheInfo._fields_}
    d["directory"] = st.directory.decode(errors="replace")
    return d


def device_get():
    """(current device of this thread — the one a render launches on —, its PCI bus id)"""
    d, bus = C.c_int(-1), C.create_string_buffer(64)
    _check(lib.srack_device_get(C.byref(d), bus, 64))
    return d.value, bus.value.decode(errors="replace")


DIST_ID_BYTES = 128


class MixComm:
    """The path's one collective behind the C ABI: an RCCL communicator over the ranks that share a render (one process per
    GPU), used for nothing but the sum of the per-rank partial mixes (srack_dist_*).

    Rank 0 calls `MixComm.unique_id()` and hands the 128 bytes to every rank over whatever side channel the host has;
    every rank then constructs `MixComm(id, n_ranks, rank)` with its device already selected (srack_device_set)."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(DIST_ID_BYTES)
        _check(lib.srack_dist_unique_id(buf))
        return buf.raw

    def __init__(self, unique_id, n_ranks, rank):
        assert len(unique_id) == DIST_ID_BYTES
        self.comm = C.c_void_p()
        _check(lib.srack_dist_init(bytes(unique_id), n_ranks, rank, C.byref(self.comm)))
        self.n_ranks, self.rank = n_ranks, rank

    def count(self):
        n = C.c_int()
        _check(lib.srack_dist_comm_count(self.comm, C.byref(n)))
        return n.value

    def reduce_mix(self, d_mix, count, root=0, stream=None):
        """ncclReduce(sum, f32) of `count` floats at device pointer `d_mix`, in place, asynchronous on `stream`."""
        _check(lib.srack_dist_reduce_mix(self.comm, d_mix, count, root, stream))

    def destroy(self):
        if self.comm:
            _check(lib.srack_dist_destroy(self.comm))
            self.comm = C.c_void_p()


class Patch:
    """The workspace's module list + plan + N voices, behind the C ABI.

    Reference API mirrored: `SynthModule::set_input` -> connect, `disconnect_input` -> disconnect,
    `get_input`, `get_num_inputs/outputs`, `plan_execution` -> plan, `execute` (x ceil(T/B) blocks)
    -> render.  Errors the reference reports as `Err(())` / panics raise SrackError(code).
    """

    def __init__(self, sample_rate=48000, buffer_size=1024, channels=2, _handle=None):
        self.sample_rate, self.buffer_size, self.channels = sample_rate, buffer_size, channels
        h = _handle if _handle is not None else C.c_void_p()
        if _handle is None:
            _check(lib.srack_patch_create(sample_rate, buffer_size, channels, C.byref(h)))
        self.h = h
        self.n_voices = 0

    # ---- .srk rack files (FileFormat, ui.rs:578-586) -------------------------------------------------
    @classmethod
    def load_srk(cls, data, sample_rate=48000, buffer_size=1024, channels=2):
        """SynthModuleWorkspaceImpl::deserialize (ui.rs:116-135) against this AudioConfig."""
        h = C.c_void_p()
        data = bytes(data)
        _check(lib.srack_patch_load_srk(data, len(data), sample_rate, buffer_size, channels, C.byref(h)))
        return cls(sample_rate, buffer_size, channels, _handle=h)

    def save_srk(self):
        n = C.c_size_t()
        _check(lib.srack_patch_save_srk(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib.srack_patch_save_srk(self.h, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    def module_id(self, module):
        buf = C.create_string_buffer(64)
        _check(lib.srack_patch_module_id(self.h, module, buf, 64))
        return buf.value.decode()

    def set_module_position(self, module, x, y):
        _check(lib.srack_patch_set_module_position(self.h, module, x, y))

    def get_module_position(self, module):
        x, y = C.c_float(), C.c_float()
        return (x.value, y.value) if _check(lib.srack_patch_get_module_position(self.h, module, C.byref(x), C.byref(y))) else None

    def set_output_buffer(self, module, port, samples):
        a = np.ascontiguousarray(samples, dtype=np.float32)
        _check(lib.srack_patch_set_output_buffer(self.h, module, port, a.ctypes.data_as(C.POINTER(C.c_float)), a.size))

    def get_output_buffer(self, module, port):
        """The block the patch holds for this port before the first tick (a loaded file's, or set_output_buffer's); empty: fresh zeros."""
        n = _check(lib.srack_patch_get_output_buffer(self.h, module, port, None, 0))
        a = np.zeros(n, dtype=np.float32)
        if n:
            _check(lib.srack_patch_get_output_buffer(self.h, module, port, a.ctypes.data_as(C.POINTER(C.c_float)), n))
        return a

    def keep_state(self, keep=True):
        """Edits between renders no longer restart the voices: the modules' device state is carried into the re-flattened program."""
        _check(lib.srack_patch_keep_state(self.h, 1 if keep else 0))

    def set_noise_seed(self, seed, first_voice=0):
        """Noise modules: stream = (seed, module, first_voice + voice); a rank owning global voices [r*V, (r+1)*V) passes r*V."""
        _check(lib.srack_patch_set_noise_seed(self.h, seed, first_voice))

    def __del__(self):
        if getattr(self, "h", None) and lib is not None:  # `lib` is already gone at interpreter shutdown
            lib.srack_patch_destroy(self.h)
            self.h = None

    # ---- graph ------------------------------------------------------------------------------
    def add_module(self, module_type):
        return _check(lib.srack_patch_add_module(self.h, module_type))

    def num_modules(self):
        return _check(lib.srack_patch_num_modules(self.h))

    def module_type(self, module):
        return _check(lib.srack_patch_module_type(self.h, module))

    def get_num_inputs(self, module):
        return _check(lib.srack_module_num_inputs(self.h, module))

    def get_num_outputs(self, module):
        return _check(lib.srack_module_num_outputs(self.h, module))

    def set_field(self, module, field, value):
        _check(lib.srack_patch_set_field(self.h, module, field, float(value)))

    def get_field(self, module, field):
        v = C.c_double()
        _check(lib.srack_patch_get_field(self.h, module, field, C.byref(v)))
        return v.value

    def set_step(self, module, channel, step, state, value=0):
        _check(lib.srack_patch_set_step(self.h, module, channel, step, state, value))

    def get_step(self, module, channel, step):
        st, v = C.c_int(), C.c_int()
        _check(lib.srack_patch_get_step(self.h, module, channel, step, C.byref(st), C.byref(v)))
        return st.value, v.value

    def set_wave(self, module, samples, sample_rate):
        """WaveBox::load's result for a SampleModule: first-channel f32 samples + the file's sample rate."""
        a = np.ascontiguousarray(samples, dtype=np.float32)
        _check(lib.srack_patch_set_wave(self.h, module, a.ctypes.data_as(C.POINTER(C.c_float)), a.size, float(sample_rate)))

    def get_wave(self, module):
        sr = C.c_float()
        n = _check(lib.srack_patch_get_wave(self.h, module, None, 0, C.byref(sr)))
        a = np.zeros(n, dtype=np.float32)
        _check(lib.srack_patch_get_wave(self.h, module, a.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(sr)))
        return a, sr.value

    def set_wave_bank(self, module, waves, rates):
        """A bank of waves for a SampleModule (srack_patch_set_wave_bank): `waves` a list of f32 arrays (any lengths, 0 included), `rates`
        their sample rates.  An empty list removes the bank.  Inert until set_voice_waves assigns voices to it."""
        waves = [np.ascontiguousarray(w, dtype=np.float32).ravel() for w in waves]
        assert len(waves) == len(rates)
        flat = np.concatenate(waves) if waves else np.zeros(0, dtype=np.float32)
        lengths = np.array([w.size for w in waves], dtype=np.intc)
        sr = np.ascontiguousarray(rates, dtype=np.float32)
        _check(lib.srack_patch_set_wave_bank(self.h, module, flat.ctypes.data_as(C.POINTER(C.c_float)), lengths.ctypes.data_as(C.POINTER(C.c_int)),
                                             sr.ctypes.data_as(C.POINTER(C.c_float)), len(waves)))

    def get_wave_bank(self, module):
        """-> (list of f32 arrays, f32 array of rates); ([], empty) without a bank"""
        n = _check(lib.srack_patch_get_wave_bank(self.h, module, None, None, 0))
        lengths, sr = np.zeros(n, dtype=np.intc), np.zeros(n, dtype=np.float32)
        _check(lib.srack_patch_get_wave_bank(self.h, module, lengths.ctypes.data_as(C.POINTER(C.c_int)), sr.ctypes.data_as(C.POINTER(C.c_float)), n))
        waves = []
        for k in range(n):
            a = np.zeros(int(lengths[k]), dtype=np.float32)
            _check(lib.srack_patch_get_wave_bank_samples(self.h, module, k, a.ctypes.data_as(C.POINTER(C.c_float)), a.size))
            waves.append(a)
        return waves, sr

    def set_voice_waves(self, module, idx):
        """Which wave of the bank every voice plays (srack_voices_set_waves): idx[v] in [0, n_waves) or WAVE_OWN; None clears."""
        _, a = _opt(idx, np.intc, (self.n_voices,))
        _check(lib.srack_voices_set_waves(self.h, module, a))

    def get_voice_waves(self, module):
        """-> int32 [V], or None when no assignment is set"""
        n = _check(lib.srack_voices_get_waves(self.h, module, None, 0))
        if n == 0:
            return None
        a = np.empty(n, dtype=np.intc)
        _check(lib.srack_voices_get_waves(self.h, module, a.ctypes.data_as(C.POINTER(C.c_int)), n))
        return a

    def set_sequence_bank(self, module, states, values=None, lengths=None):
        """A bank of sequences for a sequencer (srack_patch_set_sequence_bank): `states` u8 [n][64] for a grid sequencer or [n][8][64] for a
        pattern sequencer (STEP_NONE / _ON / _HOLD), `values` the grid's u16 [n][64] note indices (None: all 0), `lengths` [n] in 1..64
        (None: all 64).  An empty `states` removes the bank.  Inert until set_voice_sequences assigns voices to it."""
        st = np.ascontiguousarray(states, dtype=np.uint8)
        n = st.shape[0] if st.ndim > 1 else 0
        assert n == 0 or st.shape[-1] == 64, st.shape
        vals = None if values is None else np.ascontiguousarray(values, dtype=np.uint16)
        assert vals is None or vals.shape == (n, 64), vals.shape
        ln = np.full(n, 64, dtype=np.intc) if lengths is None else np.ascontiguousarray(lengths, dtype=np.intc)
        assert ln.shape == (n,), ln.shape
        _check(lib.srack_patch_set_sequence_bank(self.h, module, st.ctypes.data if n else None, None if vals is None or n == 0 else vals.ctypes.data,
                                                 ln.ctypes.data_as(C.POINTER(C.c_int)), n))

    def get_sequence_bank(self, module, channels=1):
        """-> (states u8 [n][channels][64], values u16 [n][64], lengths int32 [n]); channels: 1 for a grid, 8 for a pattern sequencer"""
        n = _check(lib.srack_patch_get_sequence_bank(self.h, module, None, None, None, 0))
        st, vals, ln = np.zeros((n, channels, 64), dtype=np.uint8), np.zeros((n, 64), dtype=np.uint16), np.zeros(n, dtype=np.intc)
        if n:
            _check(lib.srack_patch_get_sequence_bank(self.h, module, st.ctypes.data, vals.ctypes.data, ln.ctypes.data_as(C.POINTER(C.c_int)), n))
        return st, vals, ln

    def set_voice_sequences(self, module, idx):
        """Which sequence of the bank every voice plays (srack_voices_set_sequences): idx[v] in [0, n_sequences) or SEQ_OWN; None clears."""
        _, a = _opt(idx, np.intc, (self.n_voices,))
        _check(lib.srack_voices_set_sequences(self.h, module, a))

    def get_voice_sequences(self, module):
        """-> int32 [V], or None when no assignment is set"""
        n = _check(lib.srack_voices_get_sequences(self.h, module, None, 0))
        if n == 0:
            return None
        a = np.empty(n, dtype=np.intc)
        _check(lib.srack_voices_get_sequences(self.h, module, a.ctypes.data_as(C.POINTER(C.c_int)), n))
        return a

    def connect(self, src, src_port, sink, sink_port):
        _check(lib.srack_patch_connect(self.h, src, src_port, sink, sink_port))

    def disconnect(self, sink, sink_port):
        _check(lib.srack_patch_disconnect(self.h, sink, sink_port))

    def get_input(self, sink, sink_port):
        m, p = C.c_int(), C.c_int()
        _check(lib.srack_patch_get_input(self.h, sink, sink_port, C.byref(m), C.byref(p)))
        return None if m.value < 0 else (m.value, p.value)

    def plan(self, output=None, all_modules=None):
        buf = (C.c_int * 1024)()
        if output is None and all_modules is None:
            n = _check(lib.srack_patch_plan(self.h, buf, 1024))
        else:
            if all_modules is None:
                all_modules = list(range(self.num_modules()))
            arr = (C.c_int * len(all_modules))(*all_modules)
            n = _check(lib.srack_patch_plan_list(self.h, output, arr, len(all_modules), buf, 1024))
        return list(buf[:n])

    def removed_edges(self):
        buf = (C.c_int * 512)()
        n = _check(lib.srack_patch_removed_edges(self.h, buf, 256))
        return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]

    def delayed_edges(self):
        buf = (C.c_int * 1024)()
        n = _check(lib.srack_patch_delayed_edges(self.h, buf, 256))
        return [tuple(buf[4 * i:4 * i + 4]) for i in range(n)]

    # ---- voices -----------------------------------------------------------------------------
    def configure_voices(self, n_voices):
        _check(lib.srack_voices_configure(self.h, n_voices))
        self.n_voices = n_voices

    def set_voice_field(self, module, field, values):
        values = np.asarray(values)
        assert values.shape == (self.n_voices,)
        if values.dtype == np.float64:
            a = np.ascontiguousarray(values)
            _check(lib.srack_voices_set_field_f64(self.h, module, field, a.ctypes.data_as(C.POINTER(C.c_double))))
        else:
            a = np.ascontiguousarray(values, dtype=np.float32)
            _check(lib.srack_voices_set_field_f32(self.h, module, field, a.ctypes.data_as(C.POINTER(C.c_float))))

    def set_buses(self, n_buses, bus=None, gain=None):
        """The mix table (srack_voices_set_buses): bus[v] in [0, n_buses) or BUS_NONE (None: every voice in bus 0), gain[v] any f32
        (None: 1.0).  Not part of the program: changing it between renders restarts nothing."""
        _, b = _opt(bus, np.intc, (self.n_voices,))
        _, g = _opt(gain, np.float32, (self.n_voices,))
        _check(lib.srack_voices_set_buses(self.h, n_buses, b, g))

    def n_buses(self):
        """The number of mix buses of the table set with set_buses; 0 when none is set."""
        return _check(lib.srack_voices_get_buses(self.h, None, None, 0))

    def get_buses(self):
        """-> (n_buses, bus int32 [V], gain f32 [V]); (0, None, None) when no table is set"""
        n = self.n_buses()
        if n == 0:
            return 0, None, None
        b, g = np.empty(self.n_voices, dtype=np.intc), np.empty(self.n_voices, dtype=np.float32)
        _check(lib.srack_voices_get_buses(self.h, b.ctypes.data_as(C.POINTER(C.c_int)), g.ctypes.data_as(C.POINTER(C.c_float)), self.n_voices))
        return n, b, g

    def set_bus_slots(self, n_buses, bus, gain=None):
        """The mix table with up to MAX_VOICE_SLOTS buses per voice and a gain per channel (srack_voices_set_bus_slots): bus int [V][K],
        entries in [0, n_buses) or BUS_NONE (None: slot 0 is bus 0, the other slots none; K then comes from gain, or is 1), gain f32
        [V][K][channels], any f32 (None: 1.0).  Replaces a table set with set_buses, and is replaced by it.  Not part of the program."""
        k = np.shape(bus)[1] if bus is not None and np.ndim(bus) == 2 else np.shape(gain)[1] if gain is not None and np.ndim(gain) == 3 else 1
        _, b = _opt(bus, np.intc, (self.n_voices, k))
        _, g = _opt(gain, np.float32, (self.n_voices, k, self.channels))
        _check(lib.srack_voices_set_bus_slots(self.h, n_buses, k, b, g))

    def get_bus_slots(self):
        """-> (n_buses, bus int32 [V][K], gain f32 [V][K][channels]); a table set with set_buses comes back with K = 1 and its gain repeated
        per channel; (0, None, None) when no table is set"""
        k = C.c_int(0)
        n = _check(lib.srack_voices_get_bus_slots(self.h, C.byref(k), None, None, 0))
        if n == 0:
            return 0, None, None
        b, g = np.empty((self.n_voices, k.value), dtype=np.intc), np.empty((self.n_voices, k.value, self.channels), dtype=np.float32)
        _check(lib.srack_voices_get_bus_slots(self.h, C.byref(k), b.ctypes.data_as(C.POINTER(C.c_int)), g.ctypes.data_as(C.POINTER(C.c_float)), self.n_voices))
        return n, b, g

    def bus_plan(self):
        """How the table is laid out for the bus fold (srack_voices_bus_plan) -> (segments int [S][4]: tile (a slot table: the group
        tile * K + slot), bus, scratch row or -1, voices; order: the voices segment after segment)"""
        n = _check(lib.srack_voices_bus_plan(self.h, None, 0, None, 0))
        seg = np.zeros((n, 4), dtype=np.intc)
        _check(lib.srack_voices_bus_plan(self.h, seg.ctypes.data_as(C.POINTER(C.c_int)), n, None, 0))
        m = int(seg[:, 3].sum())
        order = np.zeros(max(1, m), dtype=np.intc)
        _check(lib.srack_voices_bus_plan(self.h, seg.ctypes.data_as(C.POINTER(C.c_int)), n, order.ctypes.data_as(C.POINTER(C.c_int)), m))
        return seg, order[:m]

    # ---- bus reverbs: a Freeverb per mix bus, behind the mixer ---------------------------------------
    def set_bus_reverbs(self, params=None, enabled=None):
        """srack_buses_set_reverb: params f64 [n_buses][6] in FreeverbModule's field order (FREEVERB_DAMPENING, _FREEZE, _WET, _WIDTH,
        _ROOM_SIZE, _DRY; None: the module's defaults), enabled [n_buses] (None: every bus).  Calling it again is the slider: the
        coefficients change, the tails stay.  Not part of the program: restarts nothing."""
        n_buses = self.n_buses()
        _, a = _opt(params, np.float64, (n_buses, 6))
        _, e = _opt(_truth(enabled), np.intc, (n_buses,))
        _check(lib.srack_buses_set_reverb(self.h, a, e))

    def get_bus_reverbs(self):
        """-> (n_buses, params f64 [n_buses][6], enabled int32 [n_buses]); (0, None, None) when no reverbs are set"""
        n = _check(lib.srack_buses_get_reverb(self.h, None, None, 0))
        if n == 0:
            return 0, None, None
        a, e = np.empty((n, 6), dtype=np.float64), np.empty(n, dtype=np.intc)
        _check(lib.srack_buses_get_reverb(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), e.ctypes.data_as(C.POINTER(C.c_int)), n))
        return n, a, e

    def reset_bus_reverbs(self):
        """Delay lines and filter states to zero, the sample counter to 0; the parameters stay (srack_buses_reset_reverb)."""
        _check(lib.srack_buses_reset_reverb(self.h))

    def bus_reverb_plan(self):
        """-> (the 24 line lengths at this sample rate, line = 2 * unit + channel, combs then allpasses; samples the kernel takes at a time)"""
        ln, blk = np.zeros(24, dtype=np.intc), C.c_int(0)
        _check(lib.srack_buses_reverb_plan(self.h, ln.ctypes.data_as(C.POINTER(C.c_int)), C.byref(blk)))
        return ln, blk.value

    def bus_reverb_raw(self, n_samples, d_bus_mix, d_bus_fx, stream=None):
        """Device pointers in; asynchronous on `stream` (srack_buses_reverb): d_bus_mix f32 [n_buses][channels][n], d_bus_fx f32 [n_buses][2][n]."""
        _check(lib.srack_buses_reverb(self.h, n_samples, d_bus_mix, d_bus_fx, stream))

    def bus_reverb(self, bus_mix):
        """Convenience for tests: bus_mix f32 [n_buses][channels][T] from the host through the reverbs -> fx f32 [n_buses][2][T]."""
        bm = np.ascontiguousarray(bus_mix, dtype=np.float32)
        n_buses = self.n_buses()
        assert bm.shape[:2] == (n_buses, self.channels), bm.shape
        T = bm.shape[2]
        fx = np.empty((n_buses, 2, T), dtype=np.float32)
        with DeviceScope() as dev:
            d_in, d_out = dev.upload(bm), dev.alloc(fx.nbytes)
            self.bus_reverb_raw(T, d_in, d_out, None)
            dev.download(fx, d_out)
        return fx

    # ---- master section: a gain per bus and channel, the buses summed to one stereo pair ---------------
    def set_master(self, gain=None):
        """srack_buses_set_master: gain f32 [n_buses][2], any f32 (None: 1.0 everywhere).  Not part of the program: restarts nothing."""
        g = None if gain is None else _opt(gain, np.float32, (self.n_buses(), 2))[1]
        _check(lib.srack_buses_set_master(self.h, g))

    def get_master(self):
        """-> gain f32 [n_buses][2], or None when no gains are set"""
        n = _check(lib.srack_buses_get_master(self.h, None, 0))
        if n == 0:
            return None
        g = np.empty((n, 2), dtype=np.float32)
        _check(lib.srack_buses_get_master(self.h, g.ctypes.data_as(C.POINTER(C.c_float)), n))
        return g

    def master_raw(self, n_samples, d_rows, row_channels, d_master, d_master_stats=None, stream=None):
        """Device pointers in; asynchronous on `stream` (srack_buses_master): d_rows f32 [n_buses][row_channels][n], d_master f32 [2][n],
        d_master_stats f64 [2][STAT_COUNT] (added to) or None."""
        _check(lib.srack_buses_master(self.h, n_samples, d_rows, row_channels, d_master, d_master_stats, stream))

    def master(self, rows, stats=None):
        """Convenience for tests: rows f32 [n_buses][row_channels][T] from the host through the master -> (master f32 [2][T], stats).
        stats: f64 [2][STAT_COUNT] to continue from (a copy comes back), or None for no statistics."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        assert x.ndim == 3 and x.shape[0] == self.n_buses(), x.shape
        T = x.shape[2]
        out = np.empty((2, T), dtype=np.float32)
        st = None if stats is None else np.array(stats, dtype=np.float64).reshape(2, STAT_COUNT)
        with DeviceScope() as dev:
            d_in, d_out = dev.upload(x), dev.alloc(out.nbytes)
            d_st = None if st is None else dev.upload(st)
            self.master_raw(T, d_in, x.shape[1], d_out, d_st, None)
            dev.download(out, d_out)
            if st is not None:
                dev.download(st, d_st)
        return out, st

    # ---- bus sends: aux sends from bus to bus, a gather-sum per destination bus -------------------------
    def set_sends(self, src, dst, gain=None, through=None):
        """srack_buses_set_sends: src, dst int [n_sends], gain f32 [n_sends][2] (None: 1.0), through f32 [n_buses][2] (None: 1.0); any
        f32.  An empty list removes the sends.  Not part of the program: restarts nothing."""
        s, d = np.ascontiguousarray(src, dtype=np.intc), np.ascontiguousarray(dst, dtype=np.intc)
        assert s.ndim == 1 and s.shape == d.shape, (s.shape, d.shape)
        _, g = _opt(gain, np.float32, (len(s), 2))
        t = None if through is None else _opt(through, np.float32, (self.n_buses(), 2))[1]
        ip = C.POINTER(C.c_int)
        _check(lib.srack_buses_set_sends(self.h, len(s), s.ctypes.data_as(ip), d.ctypes.data_as(ip), g, t))

    def get_sends(self):
        """-> (src int32 [n_sends], dst int32 [n_sends], gain f32 [n_sends][2], through f32 [n_buses][2]), or None when no sends are set"""
        n = _check(lib.srack_buses_get_sends(self.h, None, None, None, 0, None, 0))
        if n == 0:
            return None
        n_buses = self.n_buses()
        s, d = np.empty(n, dtype=np.intc), np.empty(n, dtype=np.intc)
        g, t = np.empty((n, 2), dtype=np.float32), np.empty((n_buses, 2), dtype=np.float32)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        _check(lib.srack_buses_get_sends(self.h, s.ctypes.data_as(ip), d.ctypes.data_as(ip), g.ctypes.data_as(fp), n, t.ctypes.data_as(fp), n_buses))
        return s, d, g, t

    def send_plan(self):
        """How the list is laid out (srack_buses_send_plan) -> (n_terms int32 [n_buses], through term included; order: the send indices
        grouped by destination ascending; the number of runs), or None when no sends are set"""
        n = _check(lib.srack_buses_get_sends(self.h, None, None, None, 0, None, 0))
        if n == 0:
            return None
        n_buses = self.n_buses()
        nt, order = np.zeros(n_buses, dtype=np.intc), np.zeros(n, dtype=np.intc)
        ip = C.POINTER(C.c_int)
        runs = _check(lib.srack_buses_send_plan(self.h, nt.ctypes.data_as(ip), n_buses, order.ctypes.data_as(ip), n))
        return nt, order, runs

    def send_raw(self, n_samples, d_rows, row_channels, d_out, stream=None):
        """Device pointers in; asynchronous on `stream` (srack_buses_send): d_rows and d_out f32 [n_buses][row_channels][n]."""
        _check(lib.srack_buses_send(self.h, n_samples, d_rows, row_channels, d_out, stream))

    def send(self, rows):
        """Convenience for tests: rows f32 [n_buses][row_channels][T] from the host through the sends -> f32 of the same shape
        (channels beyond the second are not written: they come back as zeros, which is what the output buffer is filled with)."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        assert x.ndim == 3 and x.shape[0] == self.n_buses(), x.shape
        out = np.zeros_like(x)
        with DeviceScope() as dev:
            d_in, d_out = dev.upload(x), dev.upload(out)
            self.send_raw(x.shape[2], d_in, x.shape[1], d_out, None)
            dev.download(out, d_out)
        return out

    # ---- bus filters: a Moog ladder per mix bus, behind the mixer -----------------------------------------
    def set_bus_filter(self, params=None, port=None, enabled=None):
        """srack_buses_set_filter: params f32 [n_buses][3] = FREQ, RES, EXP_AMT, any f32 (None: the module's defaults), port int [n_buses]
        VCF_OUT_* (None: lowpass), enabled [n_buses] (None: every bus).  Calling it again is the slider: parameters change, state stays.
        Not part of the program: restarts nothing."""
        n_buses = self.n_buses()
        _, a = _opt(params, np.float32, (n_buses, BUS_FILTER_NPARAMS))
        _, po = _opt(port, np.intc, (n_buses,))
        _, e = _opt(_truth(enabled), np.intc, (n_buses,))
        _check(lib.srack_buses_set_filter(self.h, a, po, e))

    def get_bus_filter(self):
        """-> (n_buses, params f32 [n_buses][3], port int32 [n_buses], enabled int32 [n_buses]); (0, None, None, None) when no filters are set"""
        n = _check(lib.srack_buses_get_filter(self.h, None, None, None, 0))
        if n == 0:
            return 0, None, None, None
        a, po, e = np.empty((n, BUS_FILTER_NPARAMS), dtype=np.float32), np.empty(n, dtype=np.intc), np.empty(n, dtype=np.intc)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        _check(lib.srack_buses_get_filter(self.h, a.ctypes.data_as(fp), po.ctypes.data_as(ip), e.ctypes.data_as(ip), n))
        return n, a, po, e

    def reset_bus_filter(self):
        """Every filter's state to zero; the parameters stay (srack_buses_reset_filter)."""
        _check(lib.srack_buses_reset_filter(self.h))

    def bus_filter_state(self):
        """-> f32 [n_buses][2][BUS_FILTER_NSTATE]: VCF_ST_F .. VCF_ST_RES per bus and channel behind the last filter call, a disabled bus as
        zeros (srack_buses_filter_state)"""
        n = _check(lib.srack_buses_filter_state(self.h, None, 0))
        st = np.zeros((n, 2, BUS_FILTER_NSTATE), dtype=np.float32)
        _check(lib.srack_buses_filter_state(self.h, st.ctypes.data_as(C.POINTER(C.c_float)), n))
        return st

    def bus_filter_raw(self, n_samples, d_rows, row_channels, d_cv, d_out, stream=None):
        """Device pointers in; asynchronous on `stream` (srack_buses_filter): d_rows and d_out f32 [n_buses][row_channels][n] (d_out may be
        d_rows), d_cv f32 [n_buses][n] or None."""
        _check(lib.srack_buses_filter(self.h, n_samples, d_rows, row_channels, d_cv, d_out, stream))

    def bus_filter(self, rows, cv=None, in_place=False):
        """Convenience for tests: rows f32 [n_buses][row_channels][T] (and cv f32 [n_buses][T]) from the host through the filters -> f32 of
        the shape of rows.  Out of place the output buffer starts as zeros, which is what channels beyond the second come back as; in
        place they come back as they went in."""
        return self._bus_stage(self.bus_filter_raw, rows, cv, in_place)[0]

    def _bus_stage(self, raw, rows, side, in_place, env=None):
        """The filters', the VCAs' and the shapers' convenience call: rows, the optional `side` row (a CV, a control) and, where env is
        not None, the stage's extra output row (fetched when env is true) through `raw` -> (out, the extra row or None).  Both outputs
        start as zeros on the device."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        n_buses = self.n_buses()
        assert x.ndim == 3 and x.shape[0] == n_buses, x.shape
        T = x.shape[2]
        c, _ = _opt(side, np.float32, (n_buses, T))
        out = np.zeros_like(x)
        extra = np.zeros((n_buses, T), dtype=np.float32) if env else None
        with DeviceScope() as dev:
            d_in = dev.upload(x)
            d_out = d_in if in_place else dev.upload(out)
            d_side = None if c is None else dev.upload(c)
            d_extra = None if extra is None else dev.upload(extra)
            tail = () if env is None else (d_extra,)
            raw(T, d_in, x.shape[1], d_side, d_out, *tail, None)
            dev.download(out, d_out)
            if extra is not None:
                dev.download(extra, d_extra)
        return out, extra

    # ---- bus VCAs: an ADSR and a VCA per mix bus, behind the mixer ------------------------------------------
    def set_bus_vca(self, params=None, mode=None, negative=None):
        """srack_buses_set_vca: params f32 [n_buses][4] = A_SEC, D_SEC, S_VAL, R_SEC, any f32 (None: the module's defaults), mode int
        [n_buses] BUS_VCA_OFF / _CV / _GATE (None: every bus GATE), negative [n_buses] (None: false).  Calling it again is the slider:
        sliders change, state stays; a bus that becomes GATE starts fresh.  Not part of the program: restarts nothing."""
        n_buses = self.n_buses()
        _, a = _opt(params, np.float32, (n_buses, BUS_VCA_NPARAMS))
        _, mo = _opt(mode, np.intc, (n_buses,))
        _, ng = _opt(_truth(negative), np.intc, (n_buses,))
        _check(lib.srack_buses_set_vca(self.h, a, mo, ng))

    def get_bus_vca(self):
        """-> (n_buses, params f32 [n_buses][4], mode int32 [n_buses], negative int32 [n_buses]); (0, None, None, None) when no VCAs are set"""
        n = _check(lib.srack_buses_get_vca(self.h, None, None, None, 0))
        if n == 0:
            return 0, None, None, None
        a, mo, ng = np.empty((n, BUS_VCA_NPARAMS), dtype=np.float32), np.empty(n, dtype=np.intc), np.empty(n, dtype=np.intc)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        _check(lib.srack_buses_get_vca(self.h, a.ctypes.data_as(fp), mo.ctypes.data_as(ip), ng.ctypes.data_as(ip), n))
        return n, a, mo, ng

    def reset_bus_vca(self):
        """Every envelope's state fresh; the setting stays (srack_buses_reset_vca)."""
        _check(lib.srack_buses_reset_vca(self.h))

    def bus_vca_state(self):
        """-> f32 [n_buses][BUS_VCA_NSTATE]: ADSR_PHASE .. ADSR_GATE_LAST per bus behind the last call, a bus that is not GATE as the fresh
        state (0, 4, 0, 0, rate, 1) (srack_buses_vca_state)"""
        n = _check(lib.srack_buses_vca_state(self.h, None, 0))
        st = np.zeros((n, BUS_VCA_NSTATE), dtype=np.float32)
        _check(lib.srack_buses_vca_state(self.h, st.ctypes.data_as(C.POINTER(C.c_float)), n))
        return st

    def bus_vca_raw(self, n_samples, d_rows, row_channels, d_ctl, d_out, d_env=None, stream=None):
        """Device pointers in; asynchronous on `stream` (srack_buses_vca): d_rows and d_out f32 [n_buses][row_channels][n] (d_out may be
        d_rows), d_ctl and d_env f32 [n_buses][n] or None."""
        _check(lib.srack_buses_vca(self.h, n_samples, d_rows, row_channels, d_ctl, d_out, d_env, stream))

    def bus_vca(self, rows, ctl=None, in_place=False, want_env=False):
        """Convenience for tests: rows f32 [n_buses][row_channels][T] (and ctl f32 [n_buses][T]) from the host through the VCAs -> f32 of
        the shape of rows, or (that, env f32 [n_buses][T]) when want_env.  Out of place the output buffer starts as zeros, which is what
        channels beyond the second come back as; in place they come back as they went in."""
        out, env = self._bus_stage(self.bus_vca_raw, rows, ctl, in_place, env=bool(want_env))
        return (out, env) if want_env else out

    # ---- bus oscillators: an LFO per mix bus writes the console's control rows ------------------------------
    def set_bus_osc(self, params=None, port=None, antialiasing=None, enabled=None):
        """srack_buses_set_osc: params f32 [n_buses][3] = VAL, DEPTH, OFFSET, any f32 (None: 0, 1, 0), port int [n_buses] OSC_OUT_*
        (None: sine), antialiasing [n_buses] (None: true), enabled [n_buses] (None: every bus).  Calling it again is the slider:
        parameters, ports and flags change, state stays; a bus that becomes enabled starts fresh.  Not part of the program: restarts nothing."""
        n_buses = self.n_buses()
        _, a = _opt(params, np.float32, (n_buses, BUS_OSC_NPARAMS))
        _, po = _opt(port, np.intc, (n_buses,))
        _, aa = _opt(_truth(antialiasing), np.intc, (n_buses,))
        _, e = _opt(_truth(enabled), np.intc, (n_buses,))
        _check(lib.srack_buses_set_osc(self.h, a, po, aa, e))

    def get_bus_osc(self):
        """-> (n_buses, params f32 [n_buses][3], port int32 [n_buses], antialiasing int32 [n_buses], enabled int32 [n_buses]);
        (0, None, None, None, None) when no oscillators are set"""
        n = _check(lib.srack_buses_get_osc(self.h, None, None, None, None, 0))
        if n == 0:
            return 0, None, None, None, None
        a, po, aa, e = np.empty((n, BUS_OSC_NPARAMS), dtype=np.float32), np.empty(n, dtype=np.intc), np.empty(n, dtype=np.intc), np.empty(n, dtype=np.intc)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        _check(lib.srack_buses_get_osc(self.h, a.ctypes.data_as(fp), po.ctypes.data_as(ip), aa.ctypes.data_as(ip), e.ctypes.data_as(ip), n))
        return n, a, po, aa, e

    def reset_bus_osc(self, pos=None):
        """Every oscillator's state fresh — phase 0.0, last true — or, with pos f64 [n_buses], each in [0, 1) and not -0.0, bus b at phase
        pos[b]; the setting stays (srack_buses_reset_osc)."""
        _, ph = _opt(pos, np.float64, (self.n_buses(),))
        _check(lib.srack_buses_reset_osc(self.h, ph))

    def bus_osc_state(self):
        """-> f64 [n_buses][BUS_OSC_NSTATE]: OSC_POS and OSC_SYNC_LAST (0.0 / 1.0) per bus behind the last call, a disabled bus as the fresh
        state (0.0, 1.0) (srack_buses_osc_state)"""
        n = _check(lib.srack_buses_osc_state(self.h, None, 0))
        st = np.zeros((n, BUS_OSC_NSTATE), dtype=np.float64)
        _check(lib.srack_buses_osc_state(self.h, st.ctypes.data_as(C.POINTER(C.c_double)), n))
        return st

    def bus_osc_raw(self, n_samples, d_cv, d_sync, d_out, stream=None):
        """Device pointers in; asynchronous on `stream` (srack_buses_osc): d_cv and d_sync f32 [n_buses][n] or None, d_out f32 [n_buses][n]."""
        _check(lib.srack_buses_osc(self.h, n_samples, d_cv, d_sync, d_out, stream))

    def bus_osc(self, n_samples, cv=None, sync=None):
        """Convenience for tests: n_samples of every bus's oscillator (cv and sync f32 [n_buses][n_samples] from the host, or None: the
        port is unconnected) -> f32 [n_buses][n_samples]."""
        n_buses = self.n_buses()
        c, _ = _opt(cv, np.float32, (n_buses, n_samples))
        g, _ = _opt(sync, np.float32, (n_buses, n_samples))
        out = np.zeros((n_buses, n_samples), dtype=np.float32)
        if n_samples == 0:
            return out
        with DeviceScope() as dev:
            d_cv, d_sync = (None if x is None else dev.upload(x) for x in (c, g))
            d_out = dev.upload(out)
            self.bus_osc_raw(n_samples, d_cv, d_sync, d_out, None)
            dev.download(out, d_out)
        return out

    # ---- bus shapers: a drive, a waveshaper and a make-up gain per mix bus, behind the mixer ----------------
    def set_bus_shaper(self, params=None, mode=None):
        """srack_buses_set_shaper: params f32 [n_buses][3] = PRE, EXPONENT, POST, any f32 (None: 1, 1, 1), mode int [n_buses]
        BUS_SHAPER_OFF / _CONST / _CV (None: every bus CONST).  Calling it again is the slider; there is no state.  Not part of the
        program: restarts nothing."""
        n_buses = self.n_buses()
        _, a = _opt(params, np.float32, (n_buses, BUS_SHAPER_NPARAMS))
        _, mo = _opt(mode, np.intc, (n_buses,))
        _check(lib.srack_buses_set_shaper(self.h, a, mo))

    def get_bus_shaper(self):
        """-> (n_buses, params f32 [n_buses][3], mode int32 [n_buses]); (0, None, None) when no shapers are set"""
        n = _check(lib.srack_buses_get_shaper(self.h, None, None, 0))
        if n == 0:
            return 0, None, None
        a, mo = np.empty((n, BUS_SHAPER_NPARAMS), dtype=np.float32), np.empty(n, dtype=np.intc)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        _check(lib.srack_buses_get_shaper(self.h, a.ctypes.data_as(fp), mo.ctypes.data_as(ip), n))
        return n, a, mo

    def bus_shaper_raw(self, n_samples, d_rows, row_channels, d_cv, d_out, stream=None):
        """Device pointers in; asynchronous on `stream` (srack_buses_shaper): d_rows and d_out f32 [n_buses][row_channels][n] (d_out may be
        d_rows), d_cv f32 [n_buses][n] or None."""
        _check(lib.srack_buses_shaper(self.h, n_samples, d_rows, row_channels, d_cv, d_out, stream))

    def bus_shaper(self, rows, cv=None, in_place=False):
        """Convenience for tests: rows f32 [n_buses][row_channels][T] (and cv f32 [n_buses][T]) from the host through the shapers -> f32 of
        the shape of rows.  Out of place the output buffer starts as zeros, which is what channels beyond the second come back as; in
        place they come back as they went in."""
        return self._bus_stage(self.bus_shaper_raw, rows, cv, in_place)[0]

    # ---- bus meters: windowed level tracks and totals per mix bus, a read-only tap on bus rows ---------------
    def bus_meter_raw(self, first_sample, n_samples, d_rows, row_channels, window, d_levels, n_windows, d_totals, stream=None):
        """Device pointers in; asynchronous on `stream` (srack_buses_meter): d_rows f32 [n_buses][row_channels][n] (read only), d_levels
        f64 [n_windows][STAT_COUNT][n_buses][2] or None, d_totals f64 [STAT_COUNT][n_buses][2] or None; both are added to."""
        _check(lib.srack_buses_meter(self.h, first_sample, n_samples, d_rows, row_channels, window, d_levels, n_windows, d_totals, stream))

    def bus_meter(self, rows, window=None, first_sample=0, levels=None, totals=None):
        """Convenience for tests: rows f32 [n_buses][row_channels][T] from the host through the meters -> (levels, totals), the updated
        arrays.  window None: no level track (levels comes back None); otherwise levels f64 [n_windows][STAT_COUNT][n_buses][2] to
        continue from (a copy comes back), None for zeros over ceil((first_sample + T) / window) windows.  totals f64
        [STAT_COUNT][n_buses][2] to continue from, None for zeros, False for no totals (None comes back)."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        n_buses = self.n_buses()
        assert x.ndim == 3 and x.shape[0] == n_buses, x.shape
        T = x.shape[2]
        lv = tt = None
        if window is not None:
            if levels is None:
                levels = np.zeros((max(1, -(-(first_sample + T) // max(1, window))), STAT_COUNT, n_buses, 2))
            lv = np.array(levels, dtype=np.float64, order="C", copy=True)
            assert lv.ndim == 4 and lv.shape[1:] == (STAT_COUNT, n_buses, 2), lv.shape
        if totals is not False:
            tt = np.zeros((STAT_COUNT, n_buses, 2)) if totals is None else np.array(totals, dtype=np.float64, order="C", copy=True)
            assert tt.shape == (STAT_COUNT, n_buses, 2), tt.shape
        with DeviceScope() as dev:
            d_in = dev.upload(x)
            d_lv, d_tt = (None if a is None else dev.upload(a) for a in (lv, tt))
            self.bus_meter_raw(first_sample, T, d_in, x.shape[1], 0 if lv is None else window, d_lv, 0 if lv is None else lv.shape[0], d_tt, None)
            for a, d in ((lv, d_lv), (tt, d_tt)):
                if a is not None:
                    dev.download(a, d)
        return lv, tt

    def get_voice_field(self, module, field):
        out = np.empty(self.n_voices, dtype=np.float64)
        _check(lib.srack_voices_get_field(self.h, module, field, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    # ---- render -----------------------------------------------------------------------------
    def planes(self):
        buf = (C.c_int * 8)()
        n = _check(lib.srack_render_planes(self.h, buf, 8))
        return n, list(buf[:self.channels])

    def reserve(self, n_samples, want_mix=True, flags=0):
        """First-use set-up (flatten, upload, scratch buffers) ahead of the first render."""
        _check(lib.srack_render_reserve(self.h, n_samples, 1 if want_mix else 0, flags))

    def render_buses_raw(self, n_samples, d_bus_mix, d_frames=None, d_mix=None, d_stats=None, flags=0, stream=None):
        """render_raw plus d_bus_mix: device, f32 [n_buses][channels][n_samples], written (srack_render_buses)."""
        _check(lib.srack_render_buses(self.h, n_samples, d_frames, d_mix, d_stats, d_bus_mix, flags, stream))

    def render_raw(self, n_samples, d_frames=None, d_mix=None, flags=0, stream=None, d_stats=None):
        """Device pointers (ints) in; asynchronous on `stream`.  d_stats: per-voice statistics, f64 [planes][STAT_COUNT][V],
        folded into what the buffer holds (srack_render_stats)."""
        if d_stats is None:
            _check(lib.srack_render(self.h, n_samples, d_frames, d_mix, flags, stream))
        else:
            _check(lib.srack_render_stats(self.h, n_samples, d_frames, d_mix, d_stats, flags, stream))

    def info(self):
        n = _check(lib.srack_render_info(self.h, None, 0))   # (the length: a description names every control unit and may pass any fixed size)
        buf = C.create_string_buffer(n + 1)
        _check(lib.srack_render_info(self.h, buf, n + 1))
        return buf.value.decode()

    def kernel_source(self, flags=0):
        """The HIP source of the voice kernel specialised for this patch (SrackError(ERR_UNSUPPORTED) if the generator cannot express it)."""
        n = _check(lib.srack_render_kernel_source(self.h, flags, None, 0))
        buf = C.create_string_buffer(n + 1)
        _check(lib.srack_render_kernel_source(self.h, flags, buf, n + 1))
        return buf.value.decode()

    def kernel_compile(self, flags=0):
        """Compile that source for gfx950 with hiprtc (no GPU needed)."""
        _check(lib.srack_render_kernel_compile(self.h, flags))

    def kernel_ms(self, reset=True):
        ms, n = C.c_double(), C.c_int()
        _check(lib.srack_render_kernel_ms(self.h, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def render(self, n_samples, frames=True, mix=True, flags=0):
        """Convenience for tests: allocates device buffers through the C ABI's device helpers,
        renders, copies back.  -> (frames [planes][T][V] f32 or None, mix [C][T] f32 or None)."""
        if self.n_voices == 0:
            self.configure_voices(1)
        return self._render(n_samples, frames, mix, flags)[:2]

    def _render(self, n_samples, frames, mix, flags, st=None, bm=None):
        """render, render_stats and render_buses: the frames and the mix where asked for, the statistics `st` to continue from (they are
        written) and the bus mixes into `bm`, each where given -> (frames or None, mix or None, st, bm)"""
        n_planes, _ = self.planes()
        V, T, Cn = self.n_voices, n_samples, self.channels
        fr = np.zeros((n_planes, T, V), dtype=np.float32) if frames else None
        mx = np.empty((Cn, T), dtype=np.float32) if mix else None
        with DeviceScope() as dev:
            d_fr = dev.alloc(fr.nbytes) if frames and n_planes > 0 else None   # (without planes there is nothing to write: zeros come back)
            d_mx = dev.alloc(mx.nbytes) if mix else None
            d_st = None if st is None else dev.upload(st)
            d_bm = None if bm is None else dev.alloc(bm.nbytes)
            if bm is None:
                self.render_raw(T, d_fr, d_mx, flags, None, d_st)
            else:
                self.render_buses_raw(T, d_bm, d_fr, d_mx, d_st, flags, None)
            for a, d in ((fr, d_fr), (mx, d_mx), (st, d_st), (bm, d_bm)):
                if d is not None:
                    dev.download(a, d)
        return fr, mx, st, bm

    def render_stats(self, n_samples, frames=False, mix=False, flags=0, stats=None):
        """render() plus per-voice statistics of every plane -> (frames or None, mix or None, stats f64 [planes][STAT_COUNT][V]).
        `stats`: an earlier call's result to continue from (None: zeros).  Fields: STAT_SUM, STAT_SUM_SQ, STAT_PEAK_POS, STAT_PEAK_NEG,
        STAT_NONFINITE, STAT_CLIPPED (include/srack_hip.h)."""
        if self.n_voices == 0:
            self.configure_voices(1)
        shape = (self.planes()[0], STAT_COUNT, self.n_voices)
        st = np.zeros(shape) if stats is None else np.array(stats, dtype=np.float64, order="C", copy=True)
        assert st.shape == shape, st.shape
        return self._render(n_samples, frames, mix, flags, st)[:3]

    def render_buses(self, n_samples, frames=False, mix=False, stats=False, flags=0):
        """render_stats() plus the bus mixes of the table set with set_buses -> (frames or None, mix or None, stats or None — from zeros —,
        bus_mix f32 [n_buses][channels][T])."""
        n_buses = self.n_buses()
        if n_buses == 0:
            raise SrackError(ERR_STATE, "render_buses: no mix table set (set_buses)")
        st = np.zeros((self.planes()[0], STAT_COUNT, self.n_voices)) if stats else None
        return self._render(n_samples, frames, mix, flags, st, np.empty((n_buses, self.channels, n_samples), dtype=np.float32))

    def render_channels(self, n_samples, flags=0):
        """-> [channels][T][V] f32 (planes expanded to channels, silence for unconnected ones)."""
        fr, _ = self.render(n_samples, frames=True, mix=False, flags=flags)
        _, cp = self.planes()
        out = np.zeros((self.channels, n_samples, self.n_voices), dtype=np.float32)
        for c, p in enumerate(cp):
            if p >= 0:
                out[c] = fr[p]
        return out
