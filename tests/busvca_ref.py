"""The bus VCAs' reference (srack_buses_vca): ADSRModule (adsr.rs:134-217; oracle/srack_oracle.c) and VCAModule (vca.rs:117-148) in
NumPy f32, vectorised across buses with a Python loop over time.

Every operation is one NumPy f32 operation, so one IEEE rounding, in the reference's order; the state machine is np.where on the mode
the sample began in.  The gate's tests are spelled as the reference spells them: `> 0.0` for high and for the TransitionDetector,
`<= 0.0` for Sustain's low — a NaN gate is neither.  tests/test_bus_vca_host.py holds this file to the oracle bit for bit; the GPU
tests hold the device to this file."""
import numpy as np

F32 = np.float32
NSTATE = 6  # phase, mode, r_val, from_a_val, sample rate, gate_last: SRACK_ADSR_PHASE .. SRACK_ADSR_GATE_LAST
ATTACK, DECAY, SUSTAIN, RELEASE, NONE = 0, 1, 2, 3, 4   # SRACK_ADSR_MODE_*
OFF, CV, GATE = 0, 1, 2                                 # SRACK_BUS_VCA_*
DEFAULTS = (0.0, 0.5, 0.25, 0.5)
_ONE, _ZERO = F32(1.0), F32(0.0)


def same_bits(a, b):
    """elementwise: the same f32 bits, any NaN matching any NaN (the sends' and the master's convention)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def fresh(n, rate):
    """ADSRModule::new's state for n envelopes, f32 [n][NSTATE]: TransitionDetector.last starts TRUE"""
    return np.tile(np.array([0.0, NONE, 0.0, 0.0, F32(rate), 1.0], dtype=F32), (n, 1))


def envelope(gate, params, rate, state=None, n=None):
    """gate f32 [R][T], or None: the Gate port unconnected (then n is the sample count); params f32 [R][4] = a_sec, d_sec, s_val, r_sec;
    rate the f32 sample rate the modules carry; state f32 [R][NSTATE] to continue from (None: fresh)
    -> (env f32 [R][T], state f32 [R][NSTATE], mode int8 [R][T]: the mode each sample ENDED in)"""
    params = np.ascontiguousarray(params, dtype=F32)
    R = params.shape[0]
    has_gate = gate is not None
    if has_gate:
        gate = np.ascontiguousarray(gate, dtype=F32)
        assert gate.shape[0] == R, gate.shape
        n = gate.shape[1]
    st = fresh(R, rate) if state is None else np.array(state, dtype=F32).reshape(R, NSTATE)
    phase, r_val, from_a = st[:, 0].copy(), st[:, 2].copy(), st[:, 3].copy()
    mode, last = st[:, 1].astype(np.int64), st[:, 5] != 0
    rate = F32(rate)
    env, track = np.empty((R, n), dtype=F32), np.empty((R, n), dtype=np.int8)
    no_gate = np.zeros(R, dtype=F32)
    never = np.zeros(R, dtype=bool)
    with np.errstate(all="ignore"):
        a_sec, d_sec, s_val, r_sec = (params[:, k] for k in range(4))
        inc_a, inc_d, inc_r = _ONE / (rate * a_sec), _ONE / (rate * d_sec), _ONE / (rate * r_sec)   # a_sec = 0: +inf
        for t in range(n):
            g = gate[:, t] if has_gate else no_gate     # None => &0.0
            above = g > _ZERO
            trans = above & ~last                       # TransitionDetector::is_transition
            last = above
            high = above if has_gate else never         # gate_in_buf.is_some() && gate > 0.0
            low = (g <= _ZERO) if has_gate else ~never  # gate_in_buf.is_none() || gate <= 0.0
            is_n, is_a, is_d, is_s, is_r = (mode == m for m in (NONE, ATTACK, DECAY, SUSTAIN, RELEASE))
            ph, md = phase, mode
            # Attack
            ph_a = phase + inc_a
            a_over = is_a & (ph_a >= _ONE)
            a_tr = is_a & ~a_over & trans
            ph = np.where(is_a, np.where(a_over | a_tr, _ZERO, ph_a), ph)
            md = np.where(a_over, DECAY, md)
            r_val = np.where(a_tr, from_a, r_val)
            # Decay
            ph_d = phase + inc_d
            d_over, d_tr = is_d & (ph_d >= _ONE), is_d & trans
            ph = np.where(is_d, np.where(d_over | d_tr, _ZERO, ph_d), ph)
            md = np.where(d_tr, ATTACK, np.where(d_over, SUSTAIN, md))
            # Sustain
            s_low, s_tr = is_s & low, is_s & trans
            ph = np.where(s_low | s_tr, _ZERO, ph)
            md = np.where(s_tr, ATTACK, np.where(s_low, RELEASE, md))
            # Release: the phase advances right after a switch to Attack as well
            r_high = is_r & high
            ph_r = np.where(r_high, _ZERO, phase) + inc_r
            r_over = is_r & (ph_r >= _ONE)
            ph = np.where(is_r, np.where(r_over, _ZERO, ph_r), ph)
            r_val = np.where(r_over, _ZERO, r_val)
            md = np.where(r_over, NONE, np.where(r_high, ATTACK, md))
            # None
            n_high = is_n & high
            ph = np.where(n_high, _ZERO, ph)
            md = np.where(n_high, ATTACK, md)
            phase, mode = ph.astype(F32), md
            out = np.where(mode == NONE, _ZERO,
                           np.where(mode == ATTACK, r_val + (_ONE - r_val) * phase,
                                    np.where(mode == DECAY, s_val + (_ONE - s_val) * (_ONE - phase),
                                             np.where(mode == SUSTAIN, s_val, s_val * (_ONE - phase))))).astype(F32)
            r_val = np.where(mode != ATTACK, out, r_val)
            from_a = np.where(mode == ATTACK, out, from_a)
            env[:, t], track[:, t] = out, mode
    state = np.stack([phase, mode.astype(F32), r_val, from_a, np.full(R, rate, dtype=F32), last.astype(F32)], axis=1).astype(F32)
    return env, state, track


def vca(audio, cv, negative):
    """VCAModule with both ports connected: audio f32 [R][T], cv f32 [R][T], negative bool [R] -> f32 [R][T]"""
    audio, cv = np.asarray(audio, dtype=F32), np.asarray(cv, dtype=F32)
    with np.errstate(all="ignore"):
        open_ = np.asarray(negative, dtype=bool)[:, None] | (cv > _ZERO)
        return np.where(open_, audio * cv, _ZERO).astype(F32)


def retriggers(track, gate, mode0=NONE, last0=True):
    """How often a gate started an attack from inside each mode, over all rows: {ATTACK: .., DECAY: .., SUSTAIN: .., RELEASE: ..} —
    a rising edge on a sample that began in Attack, Decay or Sustain; a high gate on a sample that began in Release."""
    track, gate = np.asarray(track), np.asarray(gate, dtype=F32)
    above = gate > 0
    before_above = np.concatenate([np.broadcast_to(np.asarray(last0, dtype=bool), (gate.shape[0],))[:, None], above[:, :-1]], axis=1)
    began = np.concatenate([np.broadcast_to(np.asarray(mode0), (gate.shape[0],))[:, None], track[:, :-1]], axis=1)
    edge = above & ~before_above
    out = {m: int(np.count_nonzero(edge & (began == m))) for m in (ATTACK, DECAY, SUSTAIN)}
    out[RELEASE] = int(np.count_nonzero(above & (began == RELEASE)))
    return out


def bus_vca(rows, ctl, params, mode, negative, rate, state=None):
    """What srack_buses_vca writes out of place into a zeroed buffer: rows f32 [n_buses][row_channels][T], ctl f32 [n_buses][T] or None,
    params f32 [n_buses][4], mode int [n_buses] (OFF / CV / GATE), negative [n_buses], state f32 [n_buses][NSTATE] or None
    -> (out of rows' shape — channels 0 and 1 processed, an OFF bus's copied, channels beyond the second zero —, env f32 [n_buses][T] as
    d_env gets it, state [n_buses][NSTATE] as srack_buses_vca_state reads: a bus that is not GATE fresh, track int8 [n_buses][T]: the
    gated buses' modes, -1 elsewhere)"""
    rows = np.ascontiguousarray(rows, dtype=F32)
    n_buses, rc, T = rows.shape
    used = min(rc, 2)
    params = np.asarray(params, dtype=F32).reshape(n_buses, 4)
    mode, negative = np.asarray(mode).reshape(n_buses), np.asarray(negative).reshape(n_buses) != 0
    st = fresh(n_buses, rate) if state is None else np.array(state, dtype=F32).reshape(n_buses, NSTATE)
    out = np.zeros_like(rows)
    out[:, :used] = rows[:, :used]
    env = np.zeros((n_buses, T), dtype=F32)
    track = np.full((n_buses, T), -1, dtype=np.int8)
    gated, direct = np.flatnonzero(mode == GATE), np.flatnonzero(mode == CV)
    if len(gated):
        env[gated], st[gated], track[gated] = envelope(None if ctl is None else np.asarray(ctl, dtype=F32)[gated], params[gated], rate, st[gated], T)
    if len(direct) and ctl is not None:
        env[direct] = np.asarray(ctl, dtype=F32)[direct]
    for c in range(used):
        if len(gated):
            out[gated, c] = vca(rows[gated, c], env[gated], negative[gated])
        if len(direct):
            out[direct, c] = vca(rows[direct, c], env[direct], negative[direct]) if ctl is not None else _ZERO   # the CV port unconnected: output.fill(0.0)
    st[mode != GATE] = fresh(1, rate)[0]
    return out, env, st, track
