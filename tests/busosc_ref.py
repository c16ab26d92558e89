"""The bus oscillators' reference (srack_buses_osc): the ORACLE'S OWN modules, row by row — OscillatorModule (oscillator.rs:108-157),
MathModule(Multiply) by DEPTH, MathModule(Add) of OFFSET (math.rs:150-155), as oracle/srack_oracle.c ticks them.

Nothing of the oscillator is restated here: NumPy's sin and exp2 are not the host libm's.  Per row an OraclePatch with buffer_size = T;
two source modules have their output buffers set to the row's CV and sync slices (set_output_buffer), then module_calc runs the
oscillator and the two Math modules once, and get_output / get_field read the result and the state.  tests/test_bus_osc_host.py holds
this file to the reference's own unit test and to a planned render of the same three modules; the GPU tests hold the device to this file."""
import numpy as np

import srack_pkg
from oracle import oracle as O

F32 = np.float32
NSTATE = 2       # pos, sync_last: SRACK_OSC_POS, SRACK_OSC_SYNC_LAST as f64
NPARAMS = 3      # VAL, DEPTH, OFFSET
SINE, SQUARE, SAW = 0, 1, 2   # SRACK_OSC_OUT_*
DEFAULTS = (0.0, 1.0, 0.0)


def same_bits(a, b):
    """elementwise: the same f32 words, any NaN matching any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def same_state(a, b):
    """elementwise: the same f64 words, any NaN matching any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def fresh(n):
    """OscillatorModule::new's state for n oscillators, f64 [n][NSTATE]: pos 0.0, TransitionDetector.last TRUE"""
    return np.tile(np.array([0.0, 1.0]), (n, 1))


def _chain(S, T, rate, cv_connected, sync_connected):
    """-> (patch, cv source, sync source, oscillator, multiply, add); the sources are never ticked: their output buffers are set"""
    o = O.OraclePatch(int(rate), T, 1)
    src_cv, src_sync, osc, mul, add = (o.add_module(m) for m in (S.MOD_MATH, S.MOD_MATH, S.MOD_OSCILLATOR, S.MOD_MATH, S.MOD_MATH))
    if cv_connected:
        o.connect(src_cv, 0, osc, 0)     # SRACK_OSC_IN_CV
    if sync_connected:
        o.connect(src_sync, 0, osc, 1)   # SRACK_OSC_IN_SYNC
    o.set_field(mul, S.MATH_OPERATION, S.MATH_MULTIPLY)
    o.set_field(add, S.MATH_OPERATION, S.MATH_ADD)
    o.connect(mul, 0, add, 0)
    return o, src_cv, src_sync, osc, mul, add


def bus_osc(cv, sync, params, port, aa, enabled, rate, state=None, n=None):
    """What srack_buses_osc writes: cv, sync f32 [R][T] or None (the port is unconnected; with both None, n is the sample count);
    params f32 [R][3] = VAL, DEPTH, OFFSET; port int [R]; aa, enabled [R] (None: all true); rate the patch's sample rate;
    state f64 [R][NSTATE] to continue from (None: fresh)
    -> (out f32 [R][T], a disabled row +0.0; state f64 [R][NSTATE] as srack_buses_osc_state reads: a disabled bus fresh)"""
    S = srack_pkg.load()
    params = np.ascontiguousarray(params, dtype=F32)
    R = params.shape[0]
    params = params.reshape(R, NPARAMS)
    cv = None if cv is None else np.ascontiguousarray(cv, dtype=F32).reshape(R, -1)
    sync = None if sync is None else np.ascontiguousarray(sync, dtype=F32).reshape(R, -1)
    T = cv.shape[1] if cv is not None else sync.shape[1] if sync is not None else int(n)
    assert (cv is None or cv.shape == (R, T)) and (sync is None or sync.shape == (R, T))
    port = np.zeros(R, dtype=np.int64) if port is None else np.asarray(port).reshape(R)
    aa = np.ones(R, dtype=bool) if aa is None else np.asarray(aa).reshape(R) != 0
    enabled = np.ones(R, dtype=bool) if enabled is None else np.asarray(enabled).reshape(R) != 0
    st = fresh(R) if state is None else np.array(state, dtype=np.float64).reshape(R, NSTATE)
    out = np.zeros((R, T), dtype=F32)
    if T == 0:
        return out, st
    o, src_cv, src_sync, osc, mul, add = _chain(S, T, rate, cv is not None, sync is not None)
    wired = None  # the oscillator's port on the multiplier's In1
    for r in range(R):
        if not enabled[r]:
            st[r] = (0.0, 1.0)
            continue
        if cv is not None:
            o.set_output_buffer(src_cv, 0, cv[r])
        if sync is not None:
            o.set_output_buffer(src_sync, 0, sync[r])
        o.set_field(osc, S.OSC_VAL, params[r, 0])
        o.set_field(osc, S.OSC_ANTIALIASING, 1.0 if aa[r] else 0.0)
        o.set_field(osc, S.OSC_POS, st[r, 0])
        o.set_field(osc, S.OSC_SYNC_LAST, 1.0 if st[r, 1] != 0 else 0.0)
        o.set_field(mul, S.MATH_CONSTANT, params[r, 1])
        o.set_field(add, S.MATH_CONSTANT, params[r, 2])
        if wired != int(port[r]):
            if wired is not None:
                o.disconnect(mul, 0)
            wired = int(port[r])
            o.connect(osc, wired, mul, 0)
        for m in (osc, mul, add):
            o.module_calc(m)
        out[r] = o.get_output(add, 0)
        st[r] = (o.get_field(osc, S.OSC_POS), o.get_field(osc, S.OSC_SYNC_LAST))
    return out, st
