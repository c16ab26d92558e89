"""The pacing groups as tools/wave_census.py reports them (wave.hip.h pace_key; notes/r10.md), on hand-made records.  No GPU.
(The SRACK_PACE knob itself is read inside the library and not reachable from the bindings: tests/test_gpu_pace.py runs both settings.)"""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def census():
    spec = importlib.util.spec_from_file_location("wave_census", os.path.join(ROOT, "tools", "wave_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hw_id(simd, cu, sh=0, se=0, pipe=0, slot=0):
    return slot | (simd << 4) | (pipe << 6) | (cu << 8) | (sh << 12) | (se << 13)


def key_of(simd, cu, sh=0, se=0, xcc=0):
    return (xcc << 10) | ((cu | (sh << 4) | (se << 5)) << 2) | simd


def record(simd, cu, xcc=0, sh=0, se=0, pipe=0, slot=0, lead=None, steps=0, key=None, ctl=False, t0=100, t1=200):
    """One census record (fused.hip.h census_begin / census_end); lead = None: a wave of a launch that was not paced."""
    flags = 3 if ctl else 1
    if lead is not None:
        k = key_of(simd, cu, sh, se, xcc) if key is None else key
        flags |= 4 | (k << 3) | (lead << 16) | (steps << 24)
    return [t0, 0, t1, 0, hw_id(simd, cu, sh, se, pipe, slot), xcc, flags, 0xFFFFFFFF if ctl else 0]


def test_pace_key_leaves_out_the_pipe_and_the_wave_slot(census):
    assert int(census.pace_key(hw_id(2, 5, sh=1, se=3, pipe=3, slot=9), 6)) == key_of(2, 5, sh=1, se=3, xcc=6)
    assert int(census.pace_key(hw_id(2, 5, sh=1, se=3), 6)) == key_of(2, 5, sh=1, se=3, xcc=6)
    assert key_of(3, 15, sh=1, se=7, xcc=7) == 8191   # the table has 8 192 words per slice
    # the XCC's upper bits are not part of the key
    assert int(census.pace_key(hw_id(1, 1), 0x13)) == key_of(1, 1, xcc=3)


def test_group_report_of_hand_made_records(census):
    recs = []
    # a full group: SIMD 1 of CU 3 on XCC 0, four waves in four wave slots, 32 steps each, leads 0 .. 3
    recs += [record(1, 3, slot=s, lead=s, steps=32) for s in range(4)]
    # the same CU and SIMD numbers on XCC 1: another group, of five (a late joiner, far behind when it joined: lead 96)
    recs += [record(1, 3, xcc=1, slot=s, lead=1, steps=32) for s in range(4)]
    recs.append(record(1, 3, xcc=1, slot=4, lead=96, steps=32))
    recs.append([0] * 8)                          # a slot nobody wrote
    recs.append(record(0, 0, ctl=True))           # the control block is in no group
    out = census.pace_groups(np.array(recs, dtype=np.uint32))
    assert out["keys"] == 2 and out["keys_with_four"] == 1
    assert out["members_per_key"] == {"4": 1, "5": 1}
    assert out["paced_waves"] == 9 and out["key_mismatches"] == 0
    assert out["largest_lead"] == 96
    assert out["steps"] == {"min": 32, "max": 32}
    # analyse() carries the report
    assert census.analyse(np.array(recs, dtype=np.uint32))["pace"] == out


def test_group_report_without_pacing_and_with_a_wrong_key(census):
    # a launch that was not paced (the ramp): the groups by the decode of HW_ID alone
    recs = [record(0, 0, slot=s) for s in range(4)] + [record(1, 0, slot=s) for s in range(3)]
    out = census.pace_groups(np.array(recs, dtype=np.uint32))
    assert out == {"keys": 2, "keys_with_four": 1, "members_per_key": {"3": 1, "4": 1}, "paced_waves": 0}
    # a wave whose recorded key is not the decode of its HW_ID is counted
    recs = [record(0, 0, slot=s, lead=0, steps=1) for s in range(3)] + [record(0, 0, slot=3, lead=0, steps=1, key=5)]
    assert census.pace_groups(np.array(recs, dtype=np.uint32))["key_mismatches"] == 1
    assert census.pace_groups(np.zeros((3, 8), np.uint32)) is None
