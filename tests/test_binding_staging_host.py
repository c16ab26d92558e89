"""The staging contract of the binding's ten convenience calls — Patch.bus_reverb, master, send, bus_filter, bus_vca, bus_shaper,
bus_meter, render, render_stats, render_buses — without a GPU and without the library: the module's `lib` is replaced by a fake that
records every call.  srack_device_alloc hands out addresses 1 MiB apart, so an address names its allocation; a download fills the host
array with the byte 0xAB, so a result that came down is told from one that did not.  Patches stand on a fake handle.

What every run is held to: every allocation is freed exactly once and behind the sync; a stage call that fails raises SrackError, frees
what was allocated exactly once and downloads nothing; no copy of 0 bytes is issued; the stage call gets n_samples and row_channels from
the array's shape, None for an absent row and, in place, d_rows for d_out with no second allocation; every download reads from the
address the stage call was given, for the array's byte count; outputs a stage does not fully write go up as zeros; what a call
continues from goes up as given and comes back as a copy; the results have the types and shapes the docstrings give."""
import ctypes as C

import numpy as np
import pytest

import srack_pkg

NB, V, CH = 2, 3, 2        # buses, voices, channels of the fake patch
STEP = 1 << 20             # between two fake allocations
FILL = 0xAB                # what a download leaves in every byte
HANDLE = 0xBEE0


def _int(x):
    return x.value if hasattr(x, "value") else x


class FakeLib:
    """Records (name, arguments as plain integers); see the module's docstring."""

    def __init__(self, n_buses=NB, n_planes=1, fail=None):
        self.n_buses, self.n_planes, self.fail = n_buses, n_planes, fail
        self.log, self.sizes, self.up = [], {}, {}   # calls; allocation -> bytes asked for; upload address -> the bytes that went up

    def __getattr__(self, name):
        if not name.startswith("srack_"):
            raise AttributeError(name)

        def call(*args):
            args = tuple(_int(a) for a in args)
            self.log.append((name,) + args)
            if name == self.fail:
                return -1   # ERR_INVALID
            return getattr(self, "_" + name, lambda *a: 0)(*args)
        return call

    def srack_last_error(self):
        return b"fake: refused"

    def srack_device_alloc(self, ref, size):
        base = STEP * (len(self.sizes) + 1)
        ref._obj.value = base
        self.sizes[base] = size
        self.log.append(("srack_device_alloc", base, size))
        return 0

    def _srack_device_from_host(self, dst, src, nbytes, stream):
        self.up[dst] = C.string_at(src, nbytes)
        return 0

    def _srack_device_to_host(self, dst, src, nbytes, stream):
        C.memset(dst, FILL, nbytes)
        return 0

    def _srack_voices_get_buses(self, h, bus, gain, cap):
        return self.n_buses

    def srack_render_planes(self, h, buf, cap):
        for c in range(CH):
            buf[c] = c if c < self.n_planes else -1
        return self.n_planes

    def calls(self, name):
        return [c for c in self.log if c[0] == name]

    def stage(self):
        """the one stage or render call of the run"""
        st = [c for c in self.log if c[0].startswith(("srack_buses_", "srack_render")) and c[0] != "srack_render_planes"]
        assert len(st) == 1, st
        return st[0]


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


@pytest.fixture
def rig(S, monkeypatch):
    """rig(**fake's arguments) -> (fake, a Patch on a fake handle with V voices)"""
    made = []

    def make(**kw):
        fake = FakeLib(**kw)
        monkeypatch.setattr(S, "lib", fake)
        p = S.Patch(48000, 64, CH, _handle=C.c_void_p(HANDLE))
        p.n_voices = V
        made.append(p)
        return fake, p
    yield make
    for p in made:
        p.h = None   # (nothing for __del__ to hand to the real library)


def filled(a):
    return a.nbytes == 0 or (a.view(np.uint8) == FILL).all()


def check_lifetimes(fake, failed=False):
    """frees, the sync, zero-byte copies; on a failure: nothing came down"""
    names = [c[0] for c in fake.log]
    freed = [c[1] for c in fake.calls("srack_device_free")]
    assert sorted(freed) == sorted(fake.sizes), "every allocation is freed exactly once"
    for c in fake.calls("srack_device_from_host") + fake.calls("srack_device_to_host"):
        assert c[3] > 0, f"a copy of 0 bytes: {c}"
    if failed:
        assert not fake.calls("srack_device_to_host"), "nothing is downloaded behind a failed call"
        return
    assert names.count("srack_device_sync") == 1
    sync = names.index("srack_device_sync")
    assert fake.log[sync][1] is None
    assert all(i > sync for i, n in enumerate(names) if n == "srack_device_free"), "frees come behind the sync"
    stage = fake.log.index(fake.stage())
    assert all(i < stage for i, n in enumerate(names) if n == "srack_device_from_host"), "uploads come ahead of the stage call"
    assert all(stage < i < sync for i, n in enumerate(names) if n == "srack_device_to_host"), "downloads lie between the call and the sync"


def check_up(fake, addr, a):
    """`a` went up to addr as it is (nothing goes up for 0 bytes)"""
    assert addr in fake.sizes, "the address is an allocation's"
    if a.nbytes:
        assert fake.up[addr] == a.tobytes()
    else:
        assert addr not in fake.up


def check_down(fake, addr, got, shape, dtype=np.float32):
    """`got` has the shape and type, and came down from addr in one copy of its byte count (no copy for 0 bytes)"""
    assert isinstance(got, np.ndarray) and got.shape == shape and got.dtype == dtype, (got.shape, got.dtype)
    down = [c for c in fake.calls("srack_device_to_host") if c[2] == addr]
    if got.nbytes:
        assert [(c[2], c[3]) for c in down] == [(addr, got.nbytes)] and down[0][1] == got.ctypes.data and filled(got)
    else:
        assert not down


def check_downloads(fake, n):
    assert len(fake.calls("srack_device_to_host")) == n and len({c[2] for c in fake.calls("srack_device_to_host")}) == n


def rows_of(rc, T, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (NB, rc, T)).astype(np.float32)


def expect_refusal(S, fake, call):
    with pytest.raises(S.SrackError) as e:
        call()
    assert e.value.code == S.ERR_INVALID and "fake: refused" in str(e.value)
    assert fake.sizes, "the call failed behind its allocations"
    check_lifetimes(fake, failed=True)


SHAPES = [(1, 5), (3, 5), (1, 0), (3, 0)]   # row_channels, T


# ---- the reverbs, the master, the sends ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc,T", [(CH, 5), (CH, 0)])
def test_bus_reverb(S, rig, rc, T):
    fake, p = rig()
    x = rows_of(rc, T)
    fx = p.bus_reverb(x)
    name, h, n, d_in, d_out, stream = fake.stage()
    assert (name, h, n, stream) == ("srack_buses_reverb", HANDLE, T, None) and len(fake.sizes) == 2
    check_up(fake, d_in, x)
    assert d_out not in fake.up
    check_down(fake, d_out, fx, (NB, 2, T))
    check_downloads(fake, 1 if T else 0)
    check_lifetimes(fake)


@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("rc,T", SHAPES)
def test_master(S, rig, rc, T, with_stats):
    fake, p = rig()
    x = rows_of(rc, T)
    stats = np.arange(2.0 * S.STAT_COUNT).reshape(2, S.STAT_COUNT) if with_stats else None
    keep = None if stats is None else stats.copy()
    out, st = p.master(x, stats)
    name, h, n, d_in, row_channels, d_out, d_st, stream = fake.stage()
    assert (name, h, n, row_channels, stream) == ("srack_buses_master", HANDLE, T, rc, None)
    check_up(fake, d_in, x)
    check_down(fake, d_out, out, (2, T))
    if with_stats:
        assert len(fake.sizes) == 3
        check_up(fake, d_st, keep)
        check_down(fake, d_st, st, (2, S.STAT_COUNT), np.float64)
        assert st is not stats and (stats == keep).all(), "the caller's statistics are not written"
    else:
        assert d_st is None and st is None and len(fake.sizes) == 2
    check_downloads(fake, (1 if T else 0) + with_stats)
    check_lifetimes(fake)


@pytest.mark.parametrize("rc,T", SHAPES)
def test_send(S, rig, rc, T):
    fake, p = rig()
    x = rows_of(rc, T)
    out = p.send(x)
    name, h, n, d_in, row_channels, d_out, stream = fake.stage()
    assert (name, h, n, row_channels, stream) == ("srack_buses_send", HANDLE, T, rc, None) and len(fake.sizes) == 2
    check_up(fake, d_in, x)
    check_up(fake, d_out, np.zeros_like(x))
    check_down(fake, d_out, out, x.shape)
    check_downloads(fake, 1 if T else 0)
    check_lifetimes(fake)


# ---- the three in-place stages ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_side", [False, True])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("rc,T", SHAPES)
@pytest.mark.parametrize("stage,want_env", [("filter", False), ("vca", False), ("vca", True), ("shaper", False)])
def test_in_place_stages(S, rig, stage, rc, T, in_place, with_side, want_env):
    fake, p = rig()
    x = rows_of(rc, T)
    side = np.random.default_rng(1).uniform(-1, 1, (NB, T)).astype(np.float32) if with_side else None
    kw = dict(in_place=in_place)
    if stage == "vca":
        got = p.bus_vca(x, side, want_env=want_env, **kw)
        name, h, n, d_in, row_channels, d_side, d_out, d_env, stream = fake.stage()
        if want_env:
            assert isinstance(got, tuple) and len(got) == 2
            out, env = got
            check_up(fake, d_env, np.zeros((NB, T), dtype=np.float32))
            check_down(fake, d_env, env, (NB, T))
        else:
            out = got
            assert d_env is None
    else:
        out = getattr(p, "bus_" + stage)(x, side, **kw)
        name, h, n, d_in, row_channels, d_side, d_out, stream = fake.stage()
    assert (name, h, n, row_channels, stream) == ("srack_buses_" + stage, HANDLE, T, rc, None)
    check_up(fake, d_in, x)
    if in_place:
        assert d_out == d_in
    else:
        assert d_out != d_in
        check_up(fake, d_out, np.zeros_like(x))
    if with_side:
        check_up(fake, d_side, side)
    else:
        assert d_side is None
    assert len(fake.sizes) == 1 + (not in_place) + with_side + want_env, "one allocation per buffer, none for an absent one"
    check_down(fake, d_out, out, x.shape)
    check_downloads(fake, (1 + want_env) if T else 0)
    check_lifetimes(fake)


# ---- the meters ------------------------------------------------------------------------------------------------------------------------------------
# (levels and totals both off is left out: the library refuses a call that asks for neither, and nothing of the staging is different)
@pytest.mark.parametrize("levels,totals", [(lv, tt) for lv in ("off", "zeros", "given") for tt in ("zeros", "given", "off") if (lv, tt) != ("off", "off")])
@pytest.mark.parametrize("rc,T", SHAPES)
def test_bus_meter(S, rig, rc, T, levels, totals):
    fake, p = rig()
    x = rows_of(rc, T)
    first = 100
    n_windows = 3 if levels == "given" else -(-(first + T) // 64)
    lv_in = np.arange(1.0 * n_windows * S.STAT_COUNT * NB * 2).reshape(n_windows, S.STAT_COUNT, NB, 2) if levels == "given" else None
    tt_in = {"zeros": None, "off": False, "given": np.arange(1.0 * S.STAT_COUNT * NB * 2).reshape(S.STAT_COUNT, NB, 2)}[totals]
    lv_keep, tt_keep = (None if a is None or a is False else a.copy() for a in (lv_in, tt_in))
    lv, tt = p.bus_meter(x, window=None if levels == "off" else 64, first_sample=first, levels=lv_in, totals=tt_in)
    name, h, first_sample, n, d_in, row_channels, window, d_lv, nw, d_tt, stream = fake.stage()
    assert (name, h, first_sample, n, row_channels, stream) == ("srack_buses_meter", HANDLE, first, T, rc, None)
    check_up(fake, d_in, x)
    if levels == "off":
        assert (window, d_lv, nw) == (0, None, 0) and lv is None
    else:
        assert (window, nw) == (64, n_windows)
        check_up(fake, d_lv, np.zeros((n_windows, S.STAT_COUNT, NB, 2)) if lv_in is None else lv_keep)
        check_down(fake, d_lv, lv, (n_windows, S.STAT_COUNT, NB, 2), np.float64)
        assert lv_in is None or (lv is not lv_in and (lv_in == lv_keep).all()), "the caller's levels are not written"
    if totals == "off":
        assert d_tt is None and tt is None
    else:
        check_up(fake, d_tt, np.zeros((S.STAT_COUNT, NB, 2)) if tt_in is None else tt_keep)
        check_down(fake, d_tt, tt, (S.STAT_COUNT, NB, 2), np.float64)
        assert tt_in is None or (tt is not tt_in and (tt_in == tt_keep).all()), "the caller's totals are not written"
    assert len(fake.sizes) == 1 + (levels != "off") + (totals != "off")
    check_downloads(fake, (levels != "off") + (totals != "off"))
    check_lifetimes(fake)


# ---- the three renders ---------------------------------------------------------------------------------------------------------------------------
def check_render_outputs(fake, n_planes, T, frames, mix, fr, mx, d_fr, d_mx):
    if frames:
        if n_planes:
            check_down(fake, d_fr, fr, (n_planes, T, V))
        else:
            assert d_fr is None and fr.shape == (0, T, V) and fr.dtype == np.float32, "no planes: no buffer, frames of no planes"
    else:
        assert d_fr is None and fr is None
    if mix:
        check_down(fake, d_mx, mx, (CH, T))
    else:
        assert d_mx is None and mx is None
    for d in (d_fr, d_mx):
        assert d is None or d not in fake.up, "nothing goes up to a buffer the render writes in full"


RENDERS = [(n_planes, T, frames, mix) for n_planes in (1, 0) for T in (5, 0) for frames in (True, False) for mix in (True, False)]


@pytest.mark.parametrize("n_planes,T,frames,mix", RENDERS)
def test_render(S, rig, n_planes, T, frames, mix):
    fake, p = rig(n_planes=n_planes)
    got = p.render(T, frames=frames, mix=mix, flags=S.RENDER_NO_FUSION)
    assert isinstance(got, tuple) and len(got) == 2
    name, h, n, d_fr, d_mx, flags, stream = fake.stage()
    assert (name, h, n, flags, stream) == ("srack_render", HANDLE, T, S.RENDER_NO_FUSION, None)
    check_render_outputs(fake, n_planes, T, frames, mix, got[0], got[1], d_fr, d_mx)
    assert len(fake.sizes) == bool(frames and n_planes) + mix
    check_downloads(fake, (bool(frames and n_planes) + mix) if T else 0)
    check_lifetimes(fake)


@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("n_planes,T,frames,mix", RENDERS)
def test_render_stats(S, rig, n_planes, T, frames, mix, with_stats):
    fake, p = rig(n_planes=n_planes)
    stats = np.arange(1.0 * n_planes * S.STAT_COUNT * V).reshape(n_planes, S.STAT_COUNT, V) if with_stats else None
    keep = None if stats is None else stats.copy()
    got = p.render_stats(T, frames=frames, mix=mix, stats=stats)
    assert isinstance(got, tuple) and len(got) == 3
    name, h, n, d_fr, d_mx, d_st, flags, stream = fake.stage()
    assert (name, h, n, flags, stream) == ("srack_render_stats", HANDLE, T, 0, None)
    check_render_outputs(fake, n_planes, T, frames, mix, got[0], got[1], d_fr, d_mx)
    check_up(fake, d_st, np.zeros((n_planes, S.STAT_COUNT, V)) if stats is None else keep)
    check_down(fake, d_st, got[2], (n_planes, S.STAT_COUNT, V), np.float64)
    assert stats is None or (got[2] is not stats and (stats == keep).all()), "the caller's statistics are not written"
    assert len(fake.sizes) == bool(frames and n_planes) + mix + 1
    check_downloads(fake, ((bool(frames and n_planes) + mix) if T else 0) + bool(n_planes))
    check_lifetimes(fake)


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("n_planes,T,frames,mix", RENDERS)
def test_render_buses(S, rig, n_planes, T, frames, mix, stats):
    fake, p = rig(n_planes=n_planes)
    got = p.render_buses(T, frames=frames, mix=mix, stats=stats)
    assert isinstance(got, tuple) and len(got) == 4
    name, h, n, d_fr, d_mx, d_st, d_bm, flags, stream = fake.stage()
    assert (name, h, n, flags, stream) == ("srack_render_buses", HANDLE, T, 0, None)
    check_render_outputs(fake, n_planes, T, frames, mix, got[0], got[1], d_fr, d_mx)
    if stats:
        check_up(fake, d_st, np.zeros((n_planes, S.STAT_COUNT, V)))
        check_down(fake, d_st, got[2], (n_planes, S.STAT_COUNT, V), np.float64)
    else:
        assert d_st is None and got[2] is None
    assert d_bm not in fake.up
    check_down(fake, d_bm, got[3], (NB, CH, T))
    assert len(fake.sizes) == bool(frames and n_planes) + mix + stats + 1
    check_downloads(fake, ((bool(frames and n_planes) + mix + 1) if T else 0) + bool(stats and n_planes))
    check_lifetimes(fake)


def test_render_buses_without_a_table(S, rig):
    fake, p = rig(n_buses=0)
    with pytest.raises(S.SrackError) as e:
        p.render_buses(5)
    assert e.value.code == S.ERR_STATE and not fake.sizes


def test_render_configures_one_voice_where_there_is_none(S, rig):
    for call in (lambda p: p.render(5), lambda p: p.render_stats(5)):
        fake, p = rig()
        p.n_voices = 0
        got = call(p)
        assert fake.calls("srack_voices_configure") == [("srack_voices_configure", HANDLE, 1)] and got[0 if len(got) == 2 else 2].shape[-1] == 1
        check_lifetimes(fake)


# ---- a stage call that fails ---------------------------------------------------------------------------------------------------------------------
FAILURES = [
    ("srack_buses_reverb", lambda S, p: p.bus_reverb(rows_of(CH, 5))),
    ("srack_buses_master", lambda S, p: p.master(rows_of(3, 5), np.zeros((2, S.STAT_COUNT)))),
    ("srack_buses_send", lambda S, p: p.send(rows_of(3, 5))),
    ("srack_buses_filter", lambda S, p: p.bus_filter(rows_of(3, 5), np.zeros((NB, 5)))),
    ("srack_buses_filter", lambda S, p: p.bus_filter(rows_of(1, 5), in_place=True)),
    ("srack_buses_vca", lambda S, p: p.bus_vca(rows_of(3, 5), np.zeros((NB, 5)), want_env=True)),
    ("srack_buses_vca", lambda S, p: p.bus_vca(rows_of(1, 5), in_place=True)),
    ("srack_buses_shaper", lambda S, p: p.bus_shaper(rows_of(3, 5), np.zeros((NB, 5)))),
    ("srack_buses_shaper", lambda S, p: p.bus_shaper(rows_of(1, 5), in_place=True)),
    ("srack_buses_meter", lambda S, p: p.bus_meter(rows_of(3, 5), window=64)),
    ("srack_render", lambda S, p: p.render(5)),
    ("srack_render_stats", lambda S, p: p.render_stats(5, frames=True, mix=True)),
    ("srack_render_buses", lambda S, p: p.render_buses(5, frames=True, mix=True, stats=True)),
]


@pytest.mark.parametrize("k", range(len(FAILURES)))
def test_a_failed_stage_call(S, rig, k):
    name, call = FAILURES[k]
    fake, p = rig(fail=name)
    expect_refusal(S, fake, lambda: call(S, p))
    assert fake.stage()[0] == name and not fake.calls("srack_device_sync")
