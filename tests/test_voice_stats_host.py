"""Per-voice output statistics (srack_render_stats): the C ABI surface and the bindings, without a GPU."""
import ctypes
import inspect
import os
import re

import pytest

import srack_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def test_symbol_and_stat_fields(S):
    assert "srack_render_stats" in S.ABI_SYMBOLS and "srack_device_from_host" in S.ABI_SYMBOLS
    L = ctypes.CDLL(S.LIB_PATH)
    assert hasattr(L, "srack_render_stats") and hasattr(L, "srack_device_from_host")
    assert L.srack_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "srack_hip.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"SRACK_STAT_([A-Z_]+)\s*=\s*(\d+)", hdr))
    assert enum == {"SUM": 0, "SUM_SQ": 1, "PEAK_POS": 2, "PEAK_NEG": 3, "NONFINITE": 4, "CLIPPED": 5, "COUNT": 6}
    assert (S.STAT_SUM, S.STAT_SUM_SQ, S.STAT_PEAK_POS, S.STAT_PEAK_NEG, S.STAT_NONFINITE, S.STAT_CLIPPED, S.STAT_COUNT) == (0, 1, 2, 3, 4, 5, 6)
    proto = re.search(r"int srack_render_stats\((.*?)\);", hdr, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ["p", "n_samples", "d_frames", "d_mix", "d_stats", "flags", "stream"]


def test_python_wrappers_argument_order(S):
    assert list(inspect.signature(S.Patch.render_raw).parameters)[-1] == "d_stats"
    assert list(inspect.signature(S.Patch.render_raw).parameters)[:6] == ["self", "n_samples", "d_frames", "d_mix", "flags", "stream"]
    assert list(inspect.signature(S.Patch.render_stats).parameters) == ["self", "n_samples", "frames", "mix", "flags", "stats"]
    assert list(inspect.signature(S.Patch.render).parameters) == ["self", "n_samples", "frames", "mix", "flags"]


def test_errors_without_a_gpu(S):
    # a null handle
    assert S.lib.srack_render_stats(None, 16, None, None, None, 0, None) == S.ERR_INVALID
    p = S.Patch(48000, 1024, 2)
    S.build_p1(p)
    # no voices configured
    buf = (ctypes.c_double * 64)()
    assert S.lib.srack_render_stats(p.h, 16, None, None, ctypes.addressof(buf), 0, None) == S.ERR_STATE
    assert "voices_configure" in S.lib.srack_last_error().decode()
    # a misaligned statistics buffer: refused before anything reaches the device (this host has none)
    p.configure_voices(4)
    assert S.lib.srack_render_stats(p.h, 16, None, None, ctypes.addressof(buf) + 4, 0, None) == S.ERR_INVALID
    assert "aligned" in S.lib.srack_last_error().decode()
    assert S.lib.srack_render_stats(None, 16, None, None, ctypes.addressof(buf) + 4, 0, None) == S.ERR_INVALID
    # the host-to-device copy refuses null pointers
    assert S.lib.srack_device_from_host(None, ctypes.addressof(buf), 8, None) == S.ERR_INVALID


def test_rust_binding_declares_and_wraps_it():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert re.search(r"pub fn srack_render_stats\(", src)
    assert "ffi::srack_render_stats(" in src
    assert "srack_render_stats" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
