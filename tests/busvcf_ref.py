"""The bus filters' reference (srack_buses_filter): MoogFilterModule's ladder (filter.rs:58-92 and 182-221; oracle/srack_oracle.c:764-807)
in NumPy f32, vectorised across rows with a Python loop over time.

Every operation is one NumPy f32 operation, so one IEEE rounding, in the reference's order.  The clamps are np.fmin / np.fmax — the
reference's x.min(hi).max(lo) and C's fminf / fmaxf: a NaN loses against the number —, the coefficient update is np.where on
(frequency != sfreq) | (res != sres).  tests/test_bus_filter_host.py holds this file to the oracle bit for bit; the GPU tests hold
the device to this file."""
import numpy as np

F32 = np.float32
NSTATE = 10  # f, p, q, b0 .. b4, freq, res: SRACK_VCF_ST_F .. SRACK_VCF_ST_RES
_ONE, _ZERO, _P9, _P8, _TWO, _HALF, _5P6, _SIXTH, _THREE = (F32(1.0), F32(0.0), F32(0.9), F32(0.8), F32(2.0), F32(0.5), F32(5.6), F32(0.166667), F32(3.0))


def same_bits(a, b):
    """elementwise: the same f32 bits, any NaN matching any NaN (the sends' and the master's convention)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ladder(x, cv, freq, res, exp_amt, port, state=None):
    """x f32 [R][T] audio, cv f32 [R][T] or None (the CV port unconnected: 0.0f, the arithmetic still carried out), freq / res / exp_amt
    f32 [R] the sliders, port int [R] (0 lowpass, 1 bandpass, 2 highpass), state f32 [R][NSTATE] to continue from (None: zeros)
    -> (out f32 [R][T], state f32 [R][NSTATE])"""
    x = np.ascontiguousarray(x, dtype=F32)
    R, T = x.shape
    freq, res, exp_amt = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=F32), (R,))) for a in (freq, res, exp_amt))
    port = np.broadcast_to(np.asarray(port), (R,))
    st = np.zeros((R, NSTATE), dtype=F32) if state is None else np.array(state, dtype=F32).reshape(R, NSTATE)
    f, p, q, b0, b1, b2, b3, b4, sfreq, sres = (st[:, k].copy() for k in range(NSTATE))
    out = np.empty((R, T), dtype=F32)
    zero_cv = np.zeros(R, dtype=F32)
    with np.errstate(all="ignore"):
        rs = np.fmin(np.fmax(res, _ZERO), _ONE)                       # self.res.max(0.0).min(1.0)
        for t in range(T):
            c = zero_cv if cv is None else cv[:, t]
            fr = np.fmin(np.fmax(freq + c * exp_amt, _ZERO), _P9)     # (self.freq + cv * self.exp_amt).max(0.0).min(0.9)
            ch = (fr != sfreq) | (rs != sres)
            q1 = _ONE - fr
            pn = fr + _P8 * fr * q1
            fn = pn * _TWO - _ONE
            qn = rs * (_ONE + _HALF * q1 * (_ONE - q1 + _5P6 * q1 * q1))
            sfreq, sres = np.where(ch, fr, sfreq), np.where(ch, rs, sres)
            p, f, q = np.where(ch, pn, p), np.where(ch, fn, f), np.where(ch, qn, q)
            inp = x[:, t] - (q * b4)
            t1 = b1
            b1 = (inp + b0) * p - b1 * f
            t2 = b2
            b2 = (b1 + t1) * p - b2 * f
            t1 = b3
            b3 = (b2 + t2) * p - b3 * f
            b4 = (b3 + t1) * p - b4 * f
            b4 = b4 - (b4 * b4 * b4) * _SIXTH
            b0 = inp
            b0, b1, b2, b3, b4 = (np.fmax(np.fmin(b, _ONE), -_ONE) for b in (b0, b1, b2, b3, b4))   # clamp_buffers
            lp, hp, bp = b4, inp - b4, _THREE * (b3 - b4)
            out[:, t] = np.where(port == 0, lp, np.where(port == 1, bp, hp))
    return out, np.stack([f, p, q, b0, b1, b2, b3, b4, sfreq, sres], axis=1).astype(F32)


def bus_filter(rows, cv, params, port, enabled, state=None):
    """What srack_buses_filter writes out of place into a zeroed buffer: rows f32 [n_buses][row_channels][T], cv f32 [n_buses][T] or None,
    params f32 [n_buses][3], port int [n_buses], enabled [n_buses], state f32 [n_buses][2][NSTATE] or None
    -> (out of rows' shape — channels 0 and 1 filtered, a disabled bus's copied, channels beyond the second zero —, state [n_buses][2][NSTATE]:
    a disabled bus's zeros, as srack_buses_filter_state reads)"""
    rows = np.ascontiguousarray(rows, dtype=F32)
    n_buses, rc, T = rows.shape
    used = min(rc, 2)
    params = np.asarray(params, dtype=F32).reshape(n_buses, 3)
    port, enabled = np.asarray(port).reshape(n_buses), np.asarray(enabled).reshape(n_buses) != 0
    st = np.zeros((n_buses, 2, NSTATE), dtype=F32) if state is None else np.array(state, dtype=F32).reshape(n_buses, 2, NSTATE)
    out = np.zeros_like(rows)
    out[:, :used] = rows[:, :used]
    on = np.flatnonzero(enabled)
    for c in range(used):
        if len(on):
            y, s = ladder(rows[on, c], None if cv is None else np.asarray(cv, dtype=F32)[on], params[on, 0], params[on, 1], params[on, 2], port[on], st[on, c])
            out[on, c] = y
            st[on, c] = s
    st[~enabled] = 0
    return out, st
