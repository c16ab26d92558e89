"""The wave census (tools/wave_census.py, a tools-only build with -DSRK_WAVE_CENSUS): the default library carries none of it, and the
tool's arithmetic on hand-made records.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import srack_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("wave_census", os.path.join(ROOT, "tools", "wave_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_library_has_no_census():
    import ctypes
    S = srack_pkg.load()
    L = ctypes.CDLL(S.LIB_PATH)
    assert not hasattr(L, "srack_census_begin") and not hasattr(L, "srack_census_read")


def record(t0, t1, simd, cu, xcc=0, ctl=False, wave=0):
    return [t0 & 0xFFFFFFFF, t0 >> 32, t1 & 0xFFFFFFFF, t1 >> 32, (cu << 8) | (simd << 4), xcc, 3 if ctl else 1, 0xFFFFFFFF if ctl else wave]


def test_census_analysis_of_hand_made_records(census):
    base = 1 << 33   # (the 64-bit clock: a value past 32 bits)
    recs = []
    # CU 0: SIMD 0 holds two waves at once, ending at 60 and 100; SIMD 1 one wave 0 .. 80
    recs.append(record(base + 0, base + 60, 0, 0, wave=0))
    recs.append(record(base + 0, base + 100, 0, 0, wave=1))
    recs.append(record(base + 0, base + 80, 1, 0, wave=2))
    # the same CU and SIMD numbers on another XCC are another SIMD
    recs.append(record(base + 10, base + 90, 0, 0, xcc=1, wave=3))
    recs.append([0] * 8)                                   # a slot nobody wrote
    recs.append(record(base + 0, base + 50, 2, 0, ctl=True))
    out = census.analyse(np.array(recs, dtype=np.uint32))
    assert out["span_ticks_10ns"] == 100 and out["voice_waves"] == 4 and out["control_block"]
    assert out["simds"] == 3 and out["cus"] == 2 and out["xccs"] == [0, 1]
    assert out["waves_per_simd"] == {"1": 2, "2": 1}
    assert out["peak_resident_per_simd"] == {"1": 2, "2": 1}
    assert out["end_spread_within_simd_pct"]["max"] == 40.0
    assert out["simd_last_end_spread_pct"] == 20.0                       # last ends at 80, 90, 100
    assert out["voice_lifetime_over_launch"] == pytest.approx((60 + 100 + 80 + 80) / 4 / 100)
    assert out["control"]["end_pct"] == 50.0 and out["control"]["end_minus_last_voice_pct"] == -50.0
    assert census.analyse(np.zeros((3, 8), np.uint32)) is None
