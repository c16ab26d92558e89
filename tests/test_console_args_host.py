"""What the five calls of the bus console — srack_buses_send, _reverb, _vca, _filter, _master — say about their arguments, without a
GPU: every check here is made before anything reaches the device, so device addresses are plain integers (as in
tests/test_bus_vca_host.py).  One table: (the handle's state, the call, its arguments, the code, the exact text of srack_last_error).
The texts are those of the library as it stood before the checks were gathered into shared helpers (csrc/capi.cpp: console_preamble,
need_set, need_rows, meet); the table passed against that library unchanged.

The handle has 3 buses and 2 channels and every call is of 16 samples, so a block of rows is 384 bytes, a control or envelope row block
192, the master's pair 128.  Overlaps are tried at both ends, four bytes deep: the intervals are half open.  Where several arguments are
wrong the table says which one is reported."""
import numpy as np
import pytest

import srack_pkg

N, ROWS, ROW, PAIR = 16, 4 * 3 * 2 * 16, 4 * 3 * 16, 4 * 2 * 16
A, FAR, FARTHER = 1 << 20, 1 << 24, 1 << 25

# the calls' arguments behind the handle, the stream left out: it is None throughout
FN = {"send": "srack_buses_send",        # n, d_rows, row_channels, d_out
      "reverb": "srack_buses_reverb",    # n, d_bus_mix, d_bus_fx
      "vca": "srack_buses_vca",          # n, d_rows, row_channels, d_ctl, d_out, d_env
      "filter": "srack_buses_filter",    # n, d_rows, row_channels, d_cv, d_out
      "master": "srack_buses_master",    # n, d_rows, row_channels, d_master, d_master_stats
      "reset_reverb": "srack_buses_reset_reverb", "reset_filter": "srack_buses_reset_filter", "filter_state": "srack_buses_filter_state",
      "reset_vca": "srack_buses_reset_vca", "vca_state": "srack_buses_vca_state"}
GOOD = {"send": (N, A, 2, FAR), "reverb": (N, A, FAR), "vca": (N, A, 2, None, FAR, None), "filter": (N, A, 2, None, FAR),
        "master": (N, A, 2, FAR, None)}
WHO = {k: v[len("srack_"):] for k, v in FN.items()}
NOT_SET = {"send": "no sends set: call srack_buses_set_sends first", "reverb": "no reverbs set: call srack_buses_set_reverb first",
           "reset_reverb": "no reverbs set: call srack_buses_set_reverb first", "vca": "no VCAs set: call srack_buses_set_vca first",
           "reset_vca": "no VCAs set: call srack_buses_set_vca first", "vca_state": "no VCAs set: call srack_buses_set_vca first",
           "filter": "no filters set: call srack_buses_set_filter first", "reset_filter": "no filters set: call srack_buses_set_filter first",
           "filter_state": "no filters set: call srack_buses_set_filter first"}
IN_PART = ": d_out overlaps d_rows in part: it must be d_rows itself or disjoint from it"

CASES = []


def case(state, call, args, code, text=None):
    CASES.append(pytest.param(state, call, args, code, None if text is None else WHO[call] + text, id=f"{state}-{call}-{len(CASES)}"))


for c in GOOD:
    case("no voices", c, GOOD[c], "ERR_STATE", ": call srack_voices_configure first")
    case("no table", c, GOOD[c], "ERR_STATE", ": no mix table set: call srack_voices_set_buses first")
    case("no voices", c, (0,) + GOOD[c][1:], "ERR_STATE", ": call srack_voices_configure first")   # (zero samples is no excuse)
for c in ("reset_reverb", "reset_filter", "reset_vca"):
    case("no voices", c, (), "ERR_STATE", ": call srack_voices_configure first")
    case("no table", c, (), "ERR_STATE", ": no mix table set: call srack_voices_set_buses first")
    case("nothing set", c, (), "ERR_STATE", ": " + NOT_SET[c])
for c in ("filter_state", "vca_state"):
    case("nothing set", c, (None, 0), "ERR_STATE", ": " + NOT_SET[c])
# the stage is not set: said before any look at the call's own arguments, zero samples included (the master needs no setting)
for c in ("send", "reverb", "vca", "filter"):
    case("nothing set", c, GOOD[c], "ERR_STATE", ": " + NOT_SET[c])
    case("nothing set", c, (0,) + tuple(99 if x == 2 else None for x in GOOD[c][1:]), "ERR_STATE", ": " + NOT_SET[c])
case("nothing set", "master", (0, None, 99, None, 4), "OK")
case("nothing set", "master", (N, None, 2, FAR, None), "ERR_INVALID", ": d_rows and d_master must be given")
# zero samples: nothing to do, ahead of the pointer and row_channels checks
case("all set", "send", (0, None, 99, None), "OK")
case("all set", "reverb", (0, None, None), "OK")
case("all set", "vca", (0, None, 99, None, None, None), "OK")
case("all set", "filter", (0, None, 99, None, None), "OK")
case("all set", "master", (0, None, 99, None, 4), "OK")
# null pointers; with a bad row_channels besides, the pointers are reported
case("all set", "reverb", (N, None, FAR), "ERR_INVALID", ": d_bus_mix and d_bus_fx must be given")
case("all set", "reverb", (N, A, None), "ERR_INVALID", ": d_bus_mix and d_bus_fx must be given")
for c, out in (("send", "d_out"), ("vca", "d_out"), ("filter", "d_out"), ("master", "d_master")):
    tail = {"send": (), "vca": (None,), "filter": (), "master": (None,)}[c]
    mid = {"send": (), "vca": (None,), "filter": (None,), "master": ()}[c]
    text = f": d_rows and {out} must be given"
    case("all set", c, (N, None, 2) + mid + (FAR,) + tail, "ERR_INVALID", text)
    case("all set", c, (N, A, 2) + mid + (None,) + tail, "ERR_INVALID", text)
    case("all set", c, (N, None, 0) + mid + (None,) + tail, "ERR_INVALID", text)
    # row_channels 0 and 9; with an overlap besides, row_channels is reported
    for rc in (0, 9):
        case("all set", c, (N, A, rc) + mid + (FAR,) + tail, "ERR_INVALID", ": row_channels must be 1 .. 8")
    case("all set", c, (N, A, 9) + mid + (A + 4,) + tail, "ERR_INVALID", ": row_channels must be 1 .. 8")
# the master's statistics: behind row_channels, ahead of the overlap
case("all set", "master", (N, A, 2, FAR, 4), "ERR_INVALID", ": d_master_stats must be 8-byte aligned")
case("all set", "master", (N, A, 0, FAR, 4), "ERR_INVALID", ": row_channels must be 1 .. 8")
case("all set", "master", (N, A, 2, A, 4), "ERR_INVALID", ": d_master_stats must be 8-byte aligned")
# overlaps: the reverb, the master and the sends are out of place only
for d_in, d_out in ((A, A), (A, A + ROWS - 4), (A + ROWS - 4, A)):
    case("all set", "reverb", (N, d_in, d_out), "ERR_INVALID", ": d_bus_fx overlaps d_bus_mix")
    case("all set", "send", (N, d_in, 2, d_out), "ERR_INVALID", ": d_out overlaps d_rows")
for d_in, d_out in ((A, A), (A, A + ROWS - 4), (A + PAIR - 4, A), (A, A + 64)):
    case("all set", "master", (N, d_in, 2, d_out, None), "ERR_INVALID", ": d_master overlaps d_rows")
# ... the filters and the VCAs in place or out of place, not in between
for d_in, d_out in ((A, A + 4), (A, A + ROWS - 4), (A + ROWS - 4, A), (A + 64, A)):
    case("all set", "filter", (N, d_in, 2, None, d_out), "ERR_INVALID", IN_PART)
    case("all set", "vca", (N, d_in, 2, None, d_out, None), "ERR_INVALID", IN_PART)
    case("all set", "filter", (N, d_in, 2, d_out, d_out), "ERR_INVALID", IN_PART)         # (... ahead of d_cv on d_out)
    case("all set", "vca", (N, d_in, 2, d_out, d_out, d_out), "ERR_INVALID", IN_PART)     # (... ahead of d_ctl and d_env on d_out)
for d_x in (A, A + ROWS - 4, A - ROW + 4):
    for d_in in (A, FAR):   # in place and out of place
        case("all set", "filter", (N, d_in, 2, d_x, A), "ERR_INVALID", ": d_cv overlaps d_out")
        case("all set", "vca", (N, d_in, 2, d_x, A, None), "ERR_INVALID", ": d_ctl overlaps d_out")
        case("all set", "vca", (N, d_in, 2, None, A, d_x), "ERR_INVALID", ": d_env overlaps d_out")
        case("all set", "vca", (N, d_in, 2, d_x, A, d_x), "ERR_INVALID", ": d_ctl overlaps d_out")   # (d_ctl ahead of d_env)
    case("all set", "vca", (N, A, 2, None, FAR, d_x), "ERR_INVALID", ": d_env overlaps d_rows")
    case("all set", "vca", (N, A, 2, d_x, FAR, d_x), "ERR_INVALID", ": d_env overlaps d_rows")       # (... ahead of d_env on d_ctl)
for d_env in (FARTHER, FARTHER + ROW - 4, FARTHER - ROW + 4):
    case("all set", "vca", (N, A, 2, FARTHER, FAR, d_env), "ERR_INVALID", ": d_env overlaps d_ctl")
    case("all set", "vca", (N, A, 2, FARTHER, A, d_env), "ERR_INVALID", ": d_env overlaps d_ctl")    # in place


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


@pytest.fixture(scope="module")
def handles(S):
    def patch(voices, n_buses, stages):
        p = S.Patch(48000, 64, 2)
        S.build_p1(p)
        if voices:
            p.configure_voices(voices)
        if n_buses:
            p.set_buses(n_buses, np.arange(voices, dtype=np.intc) % n_buses)
        if stages:
            p.set_sends([0, 1], [2, 2])
            p.set_bus_reverbs()
            p.set_bus_vca()
            p.set_bus_filter()
            p.set_master()
        return p
    return {"no voices": patch(0, 0, False), "no table": patch(6, 0, False), "nothing set": patch(6, 3, False), "all set": patch(6, 3, True)}


@pytest.mark.parametrize("state,call,args,code,text", CASES)
def test_what_the_call_says(S, handles, state, call, args, code, text):
    p = handles[state]
    before = p.info() if state != "no voices" else None   # (without voices there is no program to describe)
    stream = () if call not in GOOD else (None,)
    rc = getattr(S.lib, FN[call])(p.h, *args, *stream)
    said = S.lib.srack_last_error().decode()
    assert rc == getattr(S, code), (rc, said)
    if text is not None:
        assert said == text
    assert before is None or p.info() == before, "a refused call, or one of no samples, leaves no note"


def test_the_table_covers_every_stage_and_message():
    texts = {c.values[4] for c in CASES}
    for c in GOOD:
        for state in ("no voices", "no table", "nothing set", "all set"):
            assert any(x.values[0] == state and x.values[1] == c for x in CASES), (state, c)
        assert any(x.values[1] == c and x.values[3] == "OK" for x in CASES), c
        assert sum(x.values[1] == c and "overlaps" in (x.values[4] or "") for x in CASES) >= 3, c
    for t in ("buses_vca: d_ctl overlaps d_out", "buses_vca: d_env overlaps d_out", "buses_vca: d_env overlaps d_rows", "buses_vca: d_env overlaps d_ctl",
              "buses_vca" + IN_PART, "buses_filter" + IN_PART, "buses_filter: d_cv overlaps d_out", "buses_send: d_out overlaps d_rows",
              "buses_master: d_master overlaps d_rows", "buses_reverb: d_bus_fx overlaps d_bus_mix"):
        assert t in texts, t
    for who in ("buses_send", "buses_vca", "buses_filter", "buses_master"):
        assert who + ": row_channels must be 1 .. 8" in texts
