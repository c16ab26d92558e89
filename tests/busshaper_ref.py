"""The bus shapers' reference (srack_buses_shaper): MathModule(Multiply) -> NonLinearModule (math.rs:203-205) -> MathModule(Multiply) in
NumPy f32 around the HOST libm's powf.

The two products are one NumPy f32 multiplication each, so one IEEE rounding.  The power is `powf` of the libm this host runs — the
function Rust's f32::powf and the oracle call — reached through ctypes, element by element: it is a 0.82-ulp function, and its
misroundings are part of the reference.  The two arms are math.rs:204's: `if a > 0.0 { a.powf(b) } else { -(-a).powf(b) }` — both
zeros and NaN take the second.  tests/test_bus_shaper_host.py holds this file to the oracle's three modules and to the transliteration
of the device's arithmetic (tests/libm_powf.py) bit for bit; the GPU tests hold the device to this file."""
import ctypes
import ctypes.util

import numpy as np

F32 = np.float32
NPARAMS = 3
PRE, EXPONENT, POST = 0, 1, 2          # SRACK_BUS_SHAPER_PRE / _EXPONENT / _POST
OFF, CONST, CV = 0, 1, 2               # SRACK_BUS_SHAPER_*
DEFAULTS = (1.0, 1.0, 1.0)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def same_bits(a, b):
    """elementwise: the same f32 bits, any NaN matching any NaN whatever its sign or payload (busvca_ref.same_bits)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def powf(x, y):
    """the host libm's powf, elementwise over two f32 arrays of one shape -> f32"""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=F32), np.asarray(y, dtype=F32))
    f = _libm.powf
    out = np.array([f(a, b) for a, b in zip(x.ravel().tolist(), y.ravel().tolist())], dtype=np.float64)
    with np.errstate(all="ignore"):
        return out.astype(F32).reshape(x.shape)   # (a c_float result is an f32 already: the conversion back is exact)


def nonlinear(a, b):
    """NonLinearModule on f32 arrays: a > 0 ? a.powf(b) : -(-a).powf(b)"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=F32), np.asarray(b, dtype=F32))
    pos = a > 0
    r = powf(np.where(pos, a, -a), b)
    return np.where(pos, r, -r).astype(F32)


def shape(x, pre, exponent, post):
    """One channel row or many: x f32 [..., T]; pre, exponent, post f32 broadcastable against it (the exponent a constant or a CV row)"""
    with np.errstate(all="ignore"):
        driven = (np.asarray(x, dtype=F32) * np.asarray(pre, dtype=F32)).astype(F32)
        return (nonlinear(driven, exponent) * np.asarray(post, dtype=F32)).astype(F32)


def bus_shaper(rows, cv, params, mode):
    """What srack_buses_shaper writes out of place into a zeroed buffer: rows f32 [n_buses][row_channels][T], cv f32 [n_buses][T] or None,
    params f32 [n_buses][3] = PRE, EXPONENT, POST, mode int [n_buses] (OFF / CONST / CV)
    -> out of rows' shape: channels 0 and 1 processed, an OFF bus's copied, channels beyond the second zero.  A CV bus without a cv row
    has In2 unconnected: its exponent is EXPONENT."""
    rows = np.ascontiguousarray(rows, dtype=F32)
    n_buses, rc, T = rows.shape
    used = min(rc, 2)
    params = np.asarray(params, dtype=F32).reshape(n_buses, NPARAMS)
    mode = np.asarray(mode).reshape(n_buses)
    out = np.zeros_like(rows)
    out[:, :used] = rows[:, :used]
    on = np.flatnonzero(mode != OFF)
    if len(on) == 0 or T == 0:
        return out
    expo = np.repeat(params[on, EXPONENT][:, None], T, axis=1)
    if cv is not None:
        by_cv = mode[on] == CV
        expo[by_cv] = np.asarray(cv, dtype=F32)[on][by_cv]
    out[on, :used] = shape(rows[on, :used], params[on, PRE][:, None, None], expo[:, None, :], params[on, POST][:, None, None])
    return out
