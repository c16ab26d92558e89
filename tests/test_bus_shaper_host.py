"""Bus shapers (srack_buses_set_shaper / _get_shaper / srack_buses_shaper): the C ABI surface, the bindings, the argument and lifetime
rules without a GPU — and tests/busshaper_ref.py, the reference the GPU tests compare with, held bit for bit to the oracle's MathModule ->
NonLinearModule -> MathModule chain and to the transliteration of the device's powf with the device header's tables."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import srack_pkg
from oracle import oracle as O
from tests import busshaper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srack_buses_set_shaper", "srack_buses_get_shaper", "srack_buses_shaper"]

_CTYPES = {"srack_patch*": ctypes.c_void_p, "const srack_patch*": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int,
           "const int*": ctypes.POINTER(ctypes.c_int), "int*": ctypes.POINTER(ctypes.c_int), "const float*": ctypes.POINTER(ctypes.c_float),
           "float*": ctypes.POINTER(ctypes.c_float), "void*": ctypes.c_void_p}
_DEVICE_POINTERS = {"d_rows", "d_cv", "d_out"}  # (device addresses travel as integers: c_void_p)
DEFAULTS = [1.0, 1.0, 1.0]


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


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _patch(S, channels=2, voices=6, n_buses=3, rate=48000):
    p = S.Patch(rate, 64, channels)
    p.ids = S.build_p1(p)
    if voices:
        p.configure_voices(voices)
        if n_buses:
            p.set_buses(n_buses, np.arange(voices, dtype=np.intc) % n_buses)
    return p


def test_symbols_prototypes_and_argtypes(S):
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    L = ctypes.CDLL(S.LIB_PATH)
    assert L.srack_abi_version() == 2 and S.lib.srack_abi_version() == 2
    assert re.search(r"#define SRACK_ABI_VERSION 2\b", hdr)
    assert re.search(r"#define SRACK_BUS_SHAPER_NPARAMS 3\b", hdr)
    assert re.search(r"enum \{ SRACK_BUS_SHAPER_PRE = 0, SRACK_BUS_SHAPER_EXPONENT = 1, SRACK_BUS_SHAPER_POST = 2 \};", hdr)
    assert re.search(r"enum \{ SRACK_BUS_SHAPER_OFF = 0, SRACK_BUS_SHAPER_CONST = 1, SRACK_BUS_SHAPER_CV = 2 \};", hdr)
    assert hdr.index("int srack_buses_vca(") < hdr.index("int srack_buses_set_shaper(") < hdr.index("int srack_render_reserve(")   # behind the VCAs
    assert len(set(S.ABI_SYMBOLS)) == len(S.ABI_SYMBOLS)
    for name in NAMES:
        assert name in S.ABI_SYMBOLS and hasattr(L, name), name
        proto = _prototype(hdr, name)
        argtypes = getattr(S.lib, name).argtypes
        assert len(argtypes) == len(proto), name
        for (ctype, pname), at in zip(proto, argtypes):
            want = ctypes.c_void_p if pname in _DEVICE_POINTERS else _CTYPES[ctype]
            assert at is want, f"{name}: {pname} is {at}, the header says {ctype}"
    assert [n for _, n in _prototype(hdr, "srack_buses_set_shaper")] == ["p", "params", "mode"]
    assert [n for _, n in _prototype(hdr, "srack_buses_get_shaper")] == ["p", "params", "mode", "cap"]
    assert [n for _, n in _prototype(hdr, "srack_buses_shaper")] == ["p", "n_samples", "d_rows", "row_channels", "d_cv", "d_out", "stream"]
    for gone in ("srack_buses_reset_shaper", "srack_buses_shaper_state"):   # there is no state
        assert gone not in hdr and not hasattr(L, gone), gone


def test_python_wrappers_and_constants(S):
    assert list(inspect.signature(S.Patch.set_bus_shaper).parameters) == ["self", "params", "mode"]
    assert list(inspect.signature(S.Patch.get_bus_shaper).parameters) == ["self"]
    assert list(inspect.signature(S.Patch.bus_shaper_raw).parameters) == ["self", "n_samples", "d_rows", "row_channels", "d_cv", "d_out", "stream"]
    assert list(inspect.signature(S.Patch.bus_shaper).parameters) == ["self", "rows", "cv", "in_place"]
    assert S.BUS_SHAPER_NPARAMS == 3 == R.NPARAMS and tuple(S.BUS_SHAPER_DEFAULTS) == tuple(DEFAULTS) == tuple(R.DEFAULTS)
    assert (S.BUS_SHAPER_PRE, S.BUS_SHAPER_EXPONENT, S.BUS_SHAPER_POST) == (0, 1, 2) == (R.PRE, R.EXPONENT, R.POST)
    assert (S.BUS_SHAPER_OFF, S.BUS_SHAPER_CONST, S.BUS_SHAPER_CV) == (0, 1, 2) == (R.OFF, R.CONST, R.CV)


def test_rust_and_cpp_bindings_and_documents():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "srack.hpp")).read()
    for name in NAMES:
        assert re.search(r"pub fn %s\(" % name, src), name
        assert "ffi::%s(" % name in src, name
        assert name in doc, name
        assert name + "(" in hpp, name
    for fn in ("set_bus_shaper", "get_bus_shaper", "bus_shaper"):
        assert re.search(r"pub fn %s\(" % fn, src), fn
        assert re.search(r"\b%s\(" % fn, hpp), fn
    for path, what in (("README.md", "srack_buses_shaper"), ("DESIGN.md", "busshape.hip.h"), ("NOTES.md", "notes/r24.md"), ("tools/README.md", "busshape_timing.py"),
                       ("profiles/README.md", "r24_busshape.json"), ("notes/r24.md", "srack_buses_shaper"), ("s-rack_amd/csrc/Makefile", "busshape.hip")):
        assert what in open(os.path.join(ROOT, path)).read(), (path, what)


def test_error_codes_in_their_order_without_a_device(S):
    par = np.tile(np.array(DEFAULTS, dtype=np.float32), (3, 1))
    mo = np.full(3, 2, dtype=np.intc)
    calls = {
        "set": lambda h: S.lib.srack_buses_set_shaper(h, _fp(par), _ip(mo)),
        "get": lambda h: S.lib.srack_buses_get_shaper(h, None, None, 0),
        "run": lambda h: S.lib.srack_buses_shaper(h, 16, 4096, 2, None, 8192, None),
    }
    err = lambda: S.lib.srack_last_error().decode()
    for name, call in calls.items():  # a null handle
        assert call(None) == S.ERR_INVALID, name
    p = _patch(S, voices=0)
    for name, call in calls.items():  # before srack_voices_configure
        assert call(p.h) == S.ERR_STATE, name
        assert err() == {"set": "buses_set_shaper", "get": "buses_get_shaper", "run": "buses_shaper"}[name] + ": call srack_voices_configure first", name
    p.configure_voices(6)
    for name, call in calls.items():  # before a bus table exists
        assert call(p.h) == S.ERR_STATE, name
        assert err() == {"set": "buses_set_shaper", "get": "buses_get_shaper", "run": "buses_shaper"}[name] + ": no mix table set: call srack_voices_set_buses first", name
    p.set_buses(3, np.arange(6, dtype=np.intc) % 3)
    assert calls["get"](p.h) == 0  # none set
    assert p.get_bus_shaper() == (0, None, None)
    assert calls["run"](p.h) == S.ERR_STATE  # without shapers set — before any look at the call's own arguments
    assert err() == "buses_shaper: no shapers set: call srack_buses_set_shaper first"
    assert S.lib.srack_buses_shaper(p.h, 0, None, 2, None, None, None) == S.ERR_STATE
    assert S.lib.srack_buses_shaper(p.h, 16, None, 99, None, None, None) == S.ERR_STATE
    assert calls["set"](p.h) == S.OK
    assert calls["get"](p.h) == 3
    # srack_buses_shaper's own arguments, refused before anything reaches the device (this host has none); zero samples is nothing to do
    assert S.lib.srack_buses_shaper(p.h, 0, None, 99, None, None, None) == S.OK
    assert S.lib.srack_buses_shaper(p.h, 16, None, 2, None, 8192, None) == S.ERR_INVALID
    assert err() == "buses_shaper: d_rows and d_out must be given"
    assert S.lib.srack_buses_shaper(p.h, 16, 4096, 2, None, None, None) == S.ERR_INVALID
    assert err() == "buses_shaper: d_rows and d_out must be given"
    for rc in (0, 9, 1 << 20):
        assert S.lib.srack_buses_shaper(p.h, 16, 4096, rc, None, 1 << 20, None) == S.ERR_INVALID, rc
        assert err() == "buses_shaper: row_channels must be 1 .. 8"
    nbytes, rowbytes, base, far = 3 * 2 * 16 * 4, 3 * 16 * 4, 1 << 20, 1 << 24
    for d_in, d_out in ((base, base + 4), (base, base + nbytes - 4), (base + nbytes - 4, base), (base + 64, base)):  # a partial overlap
        assert S.lib.srack_buses_shaper(p.h, 16, d_in, 2, None, d_out, None) == S.ERR_INVALID, (d_in, d_out)
        assert err() == "buses_shaper: d_out overlaps d_rows in part: it must be d_rows itself or disjoint from it"
    for d_cv in (base, base + nbytes - 4, base - rowbytes + 4):  # d_cv on d_out, in place and out of place
        for d_in in (base, far):
            assert S.lib.srack_buses_shaper(p.h, 16, d_in, 2, d_cv, base, None) == S.ERR_INVALID, (d_cv, d_in)
            assert err() == "buses_shaper: d_cv overlaps d_out"
    # ... and such calls leave the setting in place and add nothing to the description
    n, a, m = p.get_bus_shaper()
    assert n == 3 and (a == par).all() and (m == 2).all()
    assert "busshp" not in p.info()


def test_round_trip_defaults_odd_values_and_a_bad_mode(S):
    p = _patch(S, n_buses=4, voices=8)
    p.set_bus_shaper()  # NULL, NULL: 1, 1, 1 and every bus CONST
    n, a, m = p.get_bus_shaper()
    assert n == 4 and a.tolist() == [DEFAULTS] * 4 and m.tolist() == [1] * 4
    odd = np.array([[0.1, 1.0, 0.25], [np.nan, -0.0, np.inf], [-np.inf, 1e-45, 3.4028235e38], [-np.nan, 1.7, -3.0]], dtype=np.float32)
    odd.view(np.uint32)[3, 0] = 0xFFC12345  # a NaN with a payload
    mo = np.array([2, 1, 0, 2], dtype=np.intc)
    p.set_bus_shaper(odd, mo)
    n, a, m = p.get_bus_shaper()
    assert n == 4 and m.tolist() == [2, 1, 0, 2]
    np.testing.assert_array_equal(a.view(np.uint32), odd.view(np.uint32))  # bit for bit, NaN payloads and signed zeros included
    # the raw call with a NULL mode keeps params and makes every bus CONST; NULL params with modes gives 1, 1, 1; a short read copies `cap` buses
    assert S.lib.srack_buses_set_shaper(p.h, _fp(odd), None) == S.OK
    a2, m2 = np.full((4, 3), 77.0, dtype=np.float32), np.full(4, 77, dtype=np.intc)
    assert S.lib.srack_buses_get_shaper(p.h, _fp(a2), _ip(m2), 2) == 4
    np.testing.assert_array_equal(a2[:2].view(np.uint32), odd[:2].view(np.uint32))
    assert (a2[2:] == 77.0).all() and m2.tolist() == [1, 1, 77, 77]
    assert S.lib.srack_buses_set_shaper(p.h, None, _ip(mo)) == S.OK
    n, a, m = p.get_bus_shaper()
    assert a.tolist() == [DEFAULTS] * 4 and m.tolist() == [2, 1, 0, 2]
    assert S.lib.srack_buses_get_shaper(p.h, None, None, 4) == 4   # any pointer may be NULL
    # a mode outside 0..2 is refused and leaves the earlier setting in place
    p.set_bus_shaper(odd, mo)
    for bad in (3, -1, 1 << 30):
        bm = mo.copy()
        bm[2] = bad
        assert S.lib.srack_buses_set_shaper(p.h, None, _ip(bm)) == S.ERR_INVALID, bad
        assert S.lib.srack_last_error().decode() == f"buses_set_shaper: bus 2 asks for mode {bad}: a bus shaper is off (0), constant (1) or CV (2)"
    n, a, m = p.get_bus_shaper()
    np.testing.assert_array_equal(a.view(np.uint32), odd.view(np.uint32))
    assert m.tolist() == [2, 1, 0, 2]


def test_lifetime_with_the_bus_table_and_the_voices(S):
    p = _patch(S, n_buses=3, voices=6)
    par = (1 + np.arange(9, dtype=np.float32).reshape(3, 3) / 7).astype(np.float32)
    p.set_bus_shaper(par, [2, 1, 0])
    info = p.info()
    assert "busshp" not in info  # no call has run
    twin = _patch(S, n_buses=3, voices=6)
    assert twin.info() == info   # a handle that never heard of shapers says the same
    # the same n_buses, another table: the shapers stay
    p.set_buses(3, np.array([2, 2, 1, 1, 0, -1], dtype=np.intc), np.linspace(0, 1, 6).astype(np.float32))
    n, a, m = p.get_bus_shaper()
    assert n == 3 and (a == par).all() and m.tolist() == [2, 1, 0]
    # not part of the program: the description of the patch is what it was, a field edit (a re-flatten) keeps them
    assert p.info() == info
    p.set_field(p.ids["vcf"], S.VCF_RES, 0.3)
    n, a, m = p.get_bus_shaper()
    assert n == 3 and (a == par).all() and m.tolist() == [2, 1, 0]
    # a bad table is refused and drops nothing
    assert S.lib.srack_voices_set_buses(p.h, 2, _ip(np.full(6, 5, dtype=np.intc)), None) == S.ERR_INVALID
    assert p.get_bus_shaper()[0] == 3
    # the VCAs, the filters and the shapers do not know of each other
    p.set_bus_filter()
    p.set_bus_vca()
    assert p.get_bus_shaper()[0] == 3 and p.get_bus_filter()[0] == 3 and p.get_bus_vca()[0] == 3
    # another n_buses drops them
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_shaper() == (0, None, None)
    assert S.lib.srack_buses_shaper(p.h, 16, 4096, 2, None, 1 << 20, None) == S.ERR_STATE
    p.set_bus_shaper()
    assert p.get_bus_shaper()[0] == 4
    # srack_voices_configure drops the table and with it the shapers
    p.configure_voices(6)
    assert S.lib.srack_buses_get_shaper(p.h, None, None, 0) == S.ERR_STATE
    p.set_buses(4, np.arange(6, dtype=np.intc) % 4)
    assert p.get_bus_shaper() == (0, None, None)


# ---- tests/busshaper_ref.py against the oracle's MathModule -> NonLinearModule -> MathModule, bit for bit -----------------------------------
BUF, NBUF = 37, 108
T = BUF * NBUF   # 3 996


def _oracle_chain(S, pre, exponent, post, cv):
    """saw -> Math(Multiply, PRE) -> NonLinear (constant EXPONENT; In2 <- sine LFO * 0.7 + 1.3 when cv) -> Math(Multiply, POST);
    3 output channels: the chain's out, the saw, the CV row.  -> f32 [3][T]"""
    o = O.OraclePatch(48000, BUF, 3)
    osc, lfo, drive, shp, gain, scale, lift, out = (o.add_module(m) for m in (S.MOD_OSCILLATOR, S.MOD_OSCILLATOR, S.MOD_MATH, S.MOD_NONLINEAR, S.MOD_MATH,
                                                                                S.MOD_MATH, S.MOD_MATH, S.MOD_OUTPUT))
    o.set_field(osc, S.OSC_VAL, -1.0)
    o.set_field(lfo, S.OSC_VAL, -2.3)
    for m, op, c in ((drive, S.MATH_MULTIPLY, pre), (gain, S.MATH_MULTIPLY, post), (scale, S.MATH_MULTIPLY, 0.7), (lift, S.MATH_ADD, 1.3)):
        o.set_field(m, S.MATH_OPERATION, op)
        o.set_field(m, S.MATH_CONSTANT, c)
    o.set_field(shp, S.NONLIN_CONSTANT, exponent)
    o.connect(osc, S.OSC_OUT_SAW, drive, 0)
    o.connect(drive, 0, shp, 0)
    o.connect(lfo, S.OSC_OUT_SINE, scale, 0)
    o.connect(scale, 0, lift, 0)
    if cv:
        o.connect(lift, 0, shp, 1)
    o.connect(shp, 0, gain, 0)
    o.connect(gain, 0, out, 0)
    o.connect(osc, S.OSC_OUT_SAW, out, 1)
    o.connect(lift, 0, out, 2)
    return o.render(T)


def _assert_bits(got, ref, what):
    ok = R.same_bits(got, ref)
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} of {ok.size} differ, first at {tuple(np.argwhere(~ok)[0])}"


@pytest.mark.parametrize("pre,exponent,post", [(1.7, 0.6, 0.8), (0.5, 1.9, 1.5), (3.0, -1.0, 0.25), (1.0, 1.0, 1.0)])
@pytest.mark.parametrize("how", ["const", "cv", "cv_unconnected"])
def test_busshaper_ref_is_the_oracles_modules(S, how, pre, exponent, post):
    y, saw, cv = _oracle_chain(S, pre, exponent, post, cv=how == "cv")
    assert np.isfinite(saw).all() and np.abs(saw).max() > 0.5 and (saw > 0).any() and (saw < 0).any() and 0.55 < cv.min() < 0.7 and 1.9 < cv.max() < 2.05
    if exponent > 0:
        assert np.isfinite(y).all()
    assert np.count_nonzero(y) > T // 2
    par = np.array([[pre, exponent, post]], dtype=np.float32)
    rows = np.stack([saw, saw])[None]
    mode = {"const": R.CONST, "cv": R.CV, "cv_unconnected": R.CV}[how]
    got = R.bus_shaper(rows, None if how == "cv_unconnected" else cv[None], par, [mode])
    _assert_bits(got[0, 0], y, f"bus_shaper {how}, channel 0")
    _assert_bits(got[0, 1], y, f"bus_shaper {how}, channel 1")
    if how == "cv":   # the CV is meant to show; an OFF bus passes; row_channels 1 and 3
        assert np.count_nonzero(~R.same_bits(R.bus_shaper(rows, None, par, [R.CV])[0, 0], y)) > T // 2
        _assert_bits(R.bus_shaper(rows, cv[None], par, [R.OFF]), rows, "an OFF bus")
        three = np.stack([saw, saw, saw])[None]
        out3 = R.bus_shaper(three, cv[None], par, [R.CV])
        _assert_bits(out3[0, 0], y, "three channels")
        assert (out3[0, 2] == 0).all()
        _assert_bits(R.bus_shaper(rows[:, :1], cv[None], par, [R.CV])[0, 0], y, "one channel")
    elif (pre, exponent, post) != (1.0, 1.0, 1.0):
        assert np.count_nonzero(~R.same_bits(y, saw)) > T // 2, "the shaper is meant to show"


def test_busshaper_ref_takes_the_arms_as_the_reference_does():
    """math.rs:204: a sample that is not > 0 goes through -(-a).powf(b): both zeros and NaN"""
    x = np.array([0.0, -0.0, np.nan, -2.0, 2.0, np.inf, -np.inf], dtype=np.float32)
    with np.errstate(all="ignore"):
        # (+0.0 is not > 0: -(-0.0).powf(-1) = -(-inf) = +inf, the pole of an odd power keeps the zero's sign; -0.0 gives -(+inf))
        assert R.nonlinear(x, np.float32(-1.0)).tolist()[:2] == [np.inf, -np.inf]
        assert R.nonlinear(x, np.float32(-1.0)).tolist()[3:] == [-0.5, 0.5, 0.0, -0.0]
        r = R.nonlinear(x, np.float32(0.0))   # powf(anything, 0) is 1, NaN included: the second arm gives -1
        assert r.tolist() == [-1.0, -1.0, -1.0, -1.0, 1.0, 1.0, -1.0]
        assert np.isnan(R.nonlinear(x, np.float32(2.0))[2]) and R.nonlinear(x, np.float32(2.0)).view(np.uint32)[1] == 0x80000000
    assert R.same_bits(np.array([np.nan], dtype=np.float32), -np.array([np.nan], dtype=np.float32)).all()
    assert not R.same_bits(np.float32(0.0), np.float32(-0.0)).any()


def test_busshaper_ref_is_the_devices_transliteration():
    """the power inside busshaper_ref is the host's powf; the device's is powf_libm_plain with the header's tables (tests/libm_powf.py):
    the same bits on waveshaper-like arguments — a drive in [0.25, 4] on samples in (0, 2), exponents in [0.5, 2] — and wider ones"""
    import platform
    from tests import libm_powf as L
    if platform.machine() != "x86_64" or platform.libc_ver()[0] != "glibc":
        pytest.skip("the port follows glibc's x86-64 FMA build of powf")
    if "fma" not in open("/proc/cpuinfo").read().split("flags", 1)[-1].split("\n", 1)[0].split():
        pytest.skip("a host without FMA runs glibc's other build of powf")
    log2_tab, exp2f_tab = L.header_tables()
    rng = np.random.default_rng(24)
    n = 2500
    xs = np.concatenate([(rng.uniform(0, 2, n).astype(np.float32) * rng.uniform(0.25, 4, n).astype(np.float32)), 10.0 ** rng.uniform(-38, 38, n // 2),
                         rng.uniform(0, 1e-39, n // 10), [1.0, 1e-40, 1e-20, 1e30, 1e-30]]).astype(np.float32)
    ys = np.concatenate([rng.uniform(0.5, 2, n), rng.uniform(-4, 4, n // 2), rng.uniform(-2, 2, n // 10), [2.0, 0.5, -1.0, 3.0, 3.0]]).astype(np.float32)
    keep = (xs > 0) & np.isfinite(xs) & (ys != 0)
    xs, ys = xs[keep], ys[keep]
    assert len(xs) > 3000
    want = R.powf(xs, ys)
    got = np.array([L.powf_libm(float(x), float(y), log2_tab, exp2f_tab) for x, y in zip(xs, ys)]).astype(np.float32)
    _assert_bits(got, want, "powf_libm against the host's powf")
    assert (want == 0).any() and np.isinf(want).any() and ((want != 0) & (np.abs(want) < 1.1754944e-38)).any(), "underflow, overflow and a subnormal result"
