"""Bus meters (srack_buses_meter): the C ABI surface, the bindings and every argument rule without a GPU — all of them are decided
before anything reaches the device — and tests/busmeter_ref.py, the reference the GPU tests compare with: held to the per-voice
definitions (tests/test_gpu_voice_stats.ref_stats) on special values, and shown to tell orders of addition apart on the GPU tests'
case inputs."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from tests import busmeter_ref as R
from tests.test_gpu_voice_stats import ref_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "srack_buses_meter"
PARAMS = ["p", "first_sample", "n_samples", "d_rows", "row_channels", "window", "d_levels", "n_windows", "d_totals", "stream"]
_CTYPES = {"srack_patch*": ctypes.c_void_p, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "const float*": ctypes.c_void_p,
           "double*": ctypes.c_void_p, "void*": ctypes.c_void_p}  # (device addresses travel as integers: c_void_p)


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def _prototype(hdr, name):
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    args = re.search(r"int %s\((.*?)\);" % name, hdr, flags=re.S).group(1)
    out = []
    for a in [x.strip() for x in args.replace("\n", " ").split(",")]:
        m = re.match(r"(.*?)(\w+)$", a)
        out.append((re.sub(r"\s+", " ", m.group(1)).strip().replace(" *", "*"), m.group(2)))
    return out


def _patch(S, channels=2, voices=6, n_buses=3, rate=48000):
    p = S.Patch(rate, 64, channels)
    p.ids = S.build_p1(p)
    if voices:
        p.configure_voices(voices)
        if n_buses:
            p.set_buses(n_buses, np.arange(voices, dtype=np.intc) % n_buses)
    return p


def test_symbol_prototype_constant_and_no_state_calls(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2 and S.lib.srack_abi_version() == 2
    assert re.search(r"#define SRACK_ABI_VERSION 2\b", hdr)
    assert re.search(r"#define SRACK_BUS_METER_MIN_WINDOW 64\b", hdr)
    assert S.BUS_METER_MIN_WINDOW == 64 == R.MIN_WINDOW and S.STAT_COUNT == 6 == R.STAT_COUNT
    assert hdr.index("int srack_buses_shaper(") < hdr.index("int srack_buses_meter(") < hdr.index("int srack_render_reserve(")  # behind the shapers
    assert len(set(S.ABI_SYMBOLS)) == len(S.ABI_SYMBOLS)
    assert NAME in S.ABI_SYMBOLS and hasattr(L, NAME)
    proto = _prototype(hdr, NAME)
    assert [n for _, n in proto] == PARAMS
    argtypes = getattr(S.lib, NAME).argtypes
    assert len(argtypes) == len(proto)
    for (ctype, pname), at in zip(proto, argtypes):
        assert at is _CTYPES[ctype], f"{pname} is {at}, the header says {ctype}"
    for gone in ("srack_buses_reset_meter", "srack_buses_meter_state", "srack_buses_set_meter", "srack_buses_get_meter"):  # there is no state
        assert gone not in hdr and not hasattr(L, gone), gone
    assert not [s for s in S.ABI_SYMBOLS if "meter" in s and s != NAME]


def test_python_wrappers(S):
    assert list(inspect.signature(S.Patch.bus_meter_raw).parameters) == ["self", "first_sample", "n_samples", "d_rows", "row_channels", "window", "d_levels",
                                                                         "n_windows", "d_totals", "stream"]
    assert list(inspect.signature(S.Patch.bus_meter).parameters) == ["self", "rows", "window", "first_sample", "levels", "totals"]
    d = {k: v.default for k, v in inspect.signature(S.Patch.bus_meter).parameters.items()}
    assert (d["window"], d["first_sample"], d["levels"], d["totals"]) == (None, 0, None, None)


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    assert re.search(r"pub fn %s\(" % NAME, src) and "ffi::%s(" % NAME in src and re.search(r"pub fn bus_meter\(", src)
    assert NAME + "(" in hpp and re.search(r"\bbus_meter\(", hpp)
    for path, what in (("INTEGRATION.md", NAME), ("README.md", NAME), ("DESIGN.md", "busmeter.hip.h"), ("DESIGN.md", NAME), ("NOTES.md", "notes/r25.md"),
                       ("tools/README.md", "busmeter_timing.py"), ("profiles/README.md", "r25_busmeter.json"), ("notes/r25.md", NAME),
                       ("s-rack_amd/csrc/Makefile", "busmeter.hip"), ("tools/busmeter_timing.py", NAME)):
        assert what in open(os.path.join(ROOT, path)).read(), (path, what)
    limits = open(os.path.join(ROOT, "DESIGN.md")).read()
    for what in ("bus selection", "zero crossings"):  # what the meters do not have
        assert what in limits, what


def test_error_codes_in_their_order_without_a_device(S):
    lib = S.lib
    err = lambda: lib.srack_last_error().decode()
    ROWS, LV, TT = 1 << 20, 1 << 24, 1 << 28   # far apart: nothing overlaps unless a case moves them
    good = lambda h: lib.srack_buses_meter(h, 0, 16, ROWS, 2, 64, LV, 1, TT, None)
    assert good(None) == S.ERR_INVALID  # a null handle
    p = _patch(S, voices=0)
    assert good(p.h) == S.ERR_STATE and err() == "buses_meter: call srack_voices_configure first"
    assert lib.srack_buses_meter(p.h, 0, 0, None, 99, 0, None, 0, None, None) == S.ERR_STATE  # before any look at the call's own arguments
    p.configure_voices(6)
    assert good(p.h) == S.ERR_STATE and err() == "buses_meter: no mix table set: call srack_voices_set_buses first"
    assert lib.srack_buses_meter(p.h, 0, 0, None, 99, 0, None, 0, None, None) == S.ERR_STATE
    p.set_buses(3, np.arange(6, dtype=np.intc) % 3)
    info = p.info()
    # zero samples is nothing to do, whatever else is wrong
    assert lib.srack_buses_meter(p.h, 0, 0, None, 99, 0, None, 0, None, None) == S.OK
    assert lib.srack_buses_meter(p.h, 1 << 63, 0, 3, 0, 1, 5, 0, 7, None) == S.OK

    def refused(text, *args):
        assert lib.srack_buses_meter(p.h, *args, None) == S.ERR_INVALID, args
        assert err() == "buses_meter: " + text, (args, err())

    refused("d_rows must be given", 0, 16, None, 99, 0, None, 0, None)  # the first of several faults is the one reported
    for rc in (0, 9, 1 << 20):
        refused("row_channels must be 1 .. 8", 0, 16, ROWS, rc, 0, None, 0, None)
    refused("d_levels or d_totals must be given", 0, 16, ROWS, 2, 0, None, 0, None)
    refused("d_levels or d_totals must be given", 0, 16, ROWS, 2, 64, None, 1, None)
    for off in (1, 4, 7):
        refused("d_levels must be 8-byte aligned", 0, 16, ROWS, 2, 0, LV + off, 0, TT + off)
        refused("d_totals must be 8-byte aligned", 0, 16, ROWS, 2, 0, LV, 0, TT + off)
        refused("d_totals must be 8-byte aligned", 0, 16, ROWS, 2, 0, None, 0, TT + off)
    for w in (0, 1, 63):
        refused("window must be at least SRACK_BUS_METER_MIN_WINDOW (64) samples", 0, 16, ROWS, 2, w, LV, 0, TT)
    refused("n_windows must be at least 1", 0, 16, ROWS, 2, 64, LV, 0, TT)
    # the span: first_sample + n_samples <= n_windows * window holds at exactly the product and fails one above
    span = "first_sample + n_samples exceeds n_windows * window"
    far = 1 << 36  # (rows of 2^16 samples need room: the buffers of these cases lie further apart)
    for window, n_windows in ((64, 1), (100, 8), (65, 3), (4096, 1 << 28)):   # (4096 * 2^28 = 2^40)
        total = window * n_windows
        for n in (1, 16, min(total, 1 << 16)):
            # exactly at the product the span passes: the call gets as far as the next check, an overlap put there for it (nothing may
            # reach a device from here: the addresses are numbers)
            refused("d_totals overlaps d_rows", total - n, n, ROWS, 2, window, far, n_windows, ROWS)
            refused(span, total - n + 1, n, ROWS, 2, window, far, n_windows, 2 * far)
            refused(span, total - n, n + 1, ROWS, 2, window, far, n_windows, 2 * far)
    near = (1 << 40) - 5
    refused("d_totals overlaps d_rows", near, 5, ROWS, 2, 4096, far, 1 << 28, ROWS)   # first_sample near 2^40: exactly at the product
    refused(span, near, 6, ROWS, 2, 4096, far, 1 << 28, 2 * far)      # first_sample near 2^40: one above
    refused(span, near + 6, 1, ROWS, 2, 4096, far, 1 << 28, 2 * far)  # first_sample past the span
    refused(span, (1 << 64) - 8, 16, ROWS, 2, 64, far, 1, 2 * far)    # a sum that would wrap
    # with d_levels NULL, window, n_windows and first_sample are ignored: the next fault is reported (here: an overlap)
    refused("d_totals overlaps d_rows", (1 << 64) - 8, 16, ROWS, 2, 0, None, 0, ROWS + 8)
    # overlaps: rows are 3 * 2 * 16 * 4 = 384 bytes, a frame of totals 6 * 3 * 2 * 8 = 288, levels n_windows frames
    rows_bytes, frame = 3 * 2 * 16 * 4, R.STAT_COUNT * 3 * 2 * 8
    for lv in (ROWS, ROWS + rows_bytes - 8, ROWS - 2 * frame + 8):
        refused("d_levels overlaps d_rows", 0, 16, ROWS, 2, 64, lv, 2, TT)
    for tt in (ROWS, ROWS + rows_bytes - 8, ROWS - frame + 8):
        refused("d_totals overlaps d_rows", 0, 16, ROWS, 2, 64, LV, 2, tt)
        refused("d_totals overlaps d_rows", 0, 16, ROWS, 2, 0, None, 0, tt)
    for tt in (LV, LV + 2 * frame - 8, LV - frame + 8):
        refused("d_levels overlaps d_totals", 0, 16, ROWS, 2, 64, LV, 2, tt)
    # such calls leave no trace in the description
    assert p.info() == info and "meter" not in info


# ---- tests/busmeter_ref.py against the per-voice definitions --------------------------------------------------------------------------
ONE_UP = np.nextafter(np.float32(1), np.float32(2))
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, ONE_UP, -ONE_UP, 1e-45, -1e-45, 1.1754942e-38, -5e-40, 0.5, -0.25, 3.0, -7.5, 2.0 ** -30],
                    dtype=np.float32)


def _as_frames(rows):
    """rows [n_buses][2][T] -> the per-voice frames [1][T][n_buses * 2]: a (bus, channel) row is a voice"""
    n_buses, rc, T = rows.shape
    return np.ascontiguousarray(rows.reshape(n_buses * rc, T).T)[None]


def _special_rows(n_buses=5, T=300, seed=3):
    rng = np.random.default_rng(seed)
    rows = R.case_rows(n_buses, T, seed)
    at = rng.random(rows.shape) < 0.2
    rows[at] = rng.choice(SPECIALS, int(at.sum()))
    rows[1, 0] = np.nan           # a row that is entirely non-finite
    rows[1, 1, ::2] = np.inf
    rows[1, 1, 1::2] = -np.inf
    rows[2, 0, :len(SPECIALS)] = SPECIALS
    return rows


def test_reference_is_the_per_voice_definitions_on_special_values():
    rows = _special_rows()
    n_buses, _, T = rows.shape
    rng = np.random.default_rng(11)
    for init in (None, "nonzero"):
        start = None
        if init:
            start = np.zeros((1, 6, n_buses * 2))
            start[0, 0], start[0, 1] = rng.uniform(-3, 3, n_buses * 2), rng.uniform(0, 9, n_buses * 2)
            start[0, 2], start[0, 3] = np.float32(0.75), np.float32(2.5)   # a peak the samples pass, and one that few do
            start[0, 4], start[0, 5] = rng.integers(0, 9, n_buses * 2), rng.integers(0, 9, n_buses * 2)
        want = ref_stats(_as_frames(rows), start)[0].reshape(6, n_buses, 2)
        _, tt = R.bus_meter(rows, totals=None if start is None else start[0].reshape(6, n_buses, 2))
        assert R.same_bits64(tt, want).all()
        # window by window: each record is the definitions on its stretch
        for window, first in ((64, 0), (100, 37), (65, 64)):
            lv, tt2 = R.bus_meter(rows, window, first)
            assert R.same_bits64(tt2, R.bus_meter(rows)[1]).all()
            assert lv.shape[0] == -(-(first + T) // window)
            for k in range(lv.shape[0]):
                lo, hi = max(k * window - first, 0), min((k + 1) * window - first, T)
                if hi <= lo:
                    assert (lv[k] == 0).all() and not np.signbit(lv[k]).any()   # untouched
                    continue
                assert R.same_bits64(lv[k], ref_stats(_as_frames(rows[:, :, lo:hi]))[0].reshape(6, n_buses, 2)).all(), (window, first, k)
    # the values one by one
    one = lambda v: R.bus_meter(np.full((1, 1, 1), v, dtype=np.float32))[1][:, 0, 0].tolist()
    for v in (np.nan, np.inf, -np.inf):
        assert one(v) == [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        assert not np.signbit(R.bus_meter(np.full((1, 1, 1), v, dtype=np.float32))[1][:4, 0, 0]).any()   # -0.0 enters, +0.0 stays
    assert one(1.0) == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0] and one(-1.0) == [-1.0, 1.0, 0.0, 1.0, 0.0, 0.0]   # exactly +-1.0 does not clip
    up = float(ONE_UP)
    assert one(ONE_UP) == [up, up * up, up, 0.0, 0.0, 1.0] and one(-ONE_UP) == [-up, up * up, 0.0, up, 0.0, 1.0]
    tiny = float(np.float32(1e-45))
    assert one(1e-45) == [tiny, tiny * tiny, tiny, 0.0, 0.0, 0.0] and tiny * tiny > 0   # a denormal counts, and its square is an f64
    z = R.bus_meter(np.full((1, 1, 1), -0.0, dtype=np.float32))[1][:, 0, 0]
    assert z.tolist() == [0.0] * 6 and not np.signbit(z).any()   # a peak of nothing is +0.0, and +0.0 + -0.0 is +0.0
    # a stored peak does not move down, a row of channel 1 is left alone for one row channel, a third channel is never read
    tt = np.full((6, 1, 2), 5.0)
    got = R.bus_meter(np.full((1, 1, 4), 0.5, dtype=np.float32), totals=tt)[1]
    assert got[:, 0, 0].tolist() == [7.0, 6.0, 5.0, 5.0, 5.0, 5.0] and (got[:, 0, 1] == 5.0).all()
    three = np.concatenate([rows, np.full((n_buses, 1, T), np.nan, dtype=np.float32)], axis=1)
    assert R.same_bits64(R.bus_meter(three)[1], R.bus_meter(rows)[1]).all()


@pytest.mark.parametrize("seed", [7, 8, 9])
def test_case_inputs_tell_the_orders_apart(seed):
    """The GPU tests' case — NB = 130, T = 777, window 100 — on the reference alone: bit equality with the sequential loop means
    something only if another order of the same additions gives other bits, and if the clip counts are not all zero."""
    rows = R.case_rows(130, 777, seed)
    lv, _ = R.bus_meter(rows, 100, totals=False)
    n = lv.shape[0] * 130 * 2
    assert n == 2080
    rev, _ = R.bus_meter(rows, 100, totals=False, row_fn=R.row_reversed)
    til, _ = R.bus_meter(rows, 100, totals=False, row_fn=R.row_tiled)
    diff = lambda a, k: int(np.count_nonzero(~R.same_bits64(a[:, k], lv[:, k])))
    counts = {"reversed SUM": diff(rev, R.STAT_SUM), "reversed SUM_SQ": diff(rev, R.STAT_SUM_SQ), "tiled SUM": diff(til, R.STAT_SUM),
              "tiled SUM_SQ": diff(til, R.STAT_SUM_SQ)}
    clipped = int(np.count_nonzero(lv[:, R.STAT_CLIPPED] > 0))
    print(seed, counts, "records with a clipped sample:", clipped)
    for what, c in counts.items():
        assert c > n // 4, (what, c)
    assert clipped > n // 2, clipped
    for a in (rev, til):   # the other four fields do not depend on the order
        for k in (R.STAT_PEAK_POS, R.STAT_PEAK_NEG, R.STAT_NONFINITE, R.STAT_CLIPPED):
            assert R.same_bits64(a[:, k], lv[:, k]).all()
