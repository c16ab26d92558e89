"""What the seven calls of the bus console — srack_buses_send, _reverb, _vca, _filter, _shaper, _master, _meter — say about their arguments, without a
GPU: every check here is made before anything reaches the device, so device addresses are plain integers (as in
tests/test_bus_vca_host.py).  One table: (the handle's state, the call, its arguments, the code, the exact text of srack_last_error).
The texts are those of the library as it stood before the checks were gathered into shared helpers (csrc/capi.cpp: console_preamble,
need_set, need_rows, meet); the table passed against that library unchanged.

The handle has 3 buses and 2 channels and every call is of 16 samples, so a block of rows is 384 bytes, a control or envelope row block
192, the master's pair 128, the meters' totals 288 and their levels 288 a window.  Overlaps are tried at both ends, four bytes deep: the
intervals are half open (the meters' levels on their totals eight bytes deep: both are 8-byte aligned).  Where several arguments are
wrong the table says which one is reported.  The shapers' and the meters' rows were added behind those stages, ahead of folding the
shapers' checks into the helpers the filters and the VCAs use; they passed against the library as it stood."""
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

# ---- the shapers and the meters: behind the table above, whose cases keep their numbers -----------------------------------------------------------
TOTALS = 8 * 6 * 3 * 2   # f64 [STAT_COUNT][3 buses][2]; a level track is that per window
FN.update(shaper="srack_buses_shaper",   # n, d_rows, row_channels, d_cv, d_out
          meter="srack_buses_meter")     # first_sample, n, d_rows, row_channels, window, d_levels, n_windows, d_totals
WHO.update({k: FN[k][len("srack_"):] for k in ("shaper", "meter")})
GOOD.update(shaper=(N, A, 2, None, FAR), meter=(0, N, A, 2, 64, FAR, 1, None))
NOT_SET["shaper"] = "no shapers set: call srack_buses_set_shaper first"
case("no voices", "shaper", (0,) + GOOD["shaper"][1:], "ERR_STATE", ": call srack_voices_configure first")   # (zero samples is no excuse)
case("no voices", "meter", (0, 0) + GOOD["meter"][2:], "ERR_STATE", ": call srack_voices_configure first")
for c in ("shaper", "meter"):
    case("no voices", c, GOOD[c], "ERR_STATE", ": call srack_voices_configure first")
    case("no table", c, GOOD[c], "ERR_STATE", ": no mix table set: call srack_voices_set_buses first")
# the shapers: the filters' rows over again
case("nothing set", "shaper", GOOD["shaper"], "ERR_STATE", ": " + NOT_SET["shaper"])
case("nothing set", "shaper", (0, None, 99, None, None), "ERR_STATE", ": " + NOT_SET["shaper"])
case("all set", "shaper", (0, None, 99, None, None), "OK")
case("all set", "shaper", (N, None, 2, None, FAR), "ERR_INVALID", ": d_rows and d_out must be given")
case("all set", "shaper", (N, A, 2, None, None), "ERR_INVALID", ": d_rows and d_out must be given")
case("all set", "shaper", (N, None, 0, None, None), "ERR_INVALID", ": d_rows and d_out must be given")
for rc in (0, 9):
    case("all set", "shaper", (N, A, rc, None, FAR), "ERR_INVALID", ": row_channels must be 1 .. 8")
case("all set", "shaper", (N, A, 9, None, A + 4), "ERR_INVALID", ": row_channels must be 1 .. 8")
for d_in, d_out in ((A, A + 4), (A, A + ROWS - 4), (A + ROWS - 4, A), (A + 64, A)):
    case("all set", "shaper", (N, d_in, 2, None, d_out), "ERR_INVALID", IN_PART)
    case("all set", "shaper", (N, d_in, 2, d_out, d_out), "ERR_INVALID", IN_PART)         # (... ahead of d_cv on d_out)
for d_x in (A, A + ROWS - 4, A - ROW + 4):
    for d_in in (A, FAR):   # in place and out of place
        case("all set", "shaper", (N, d_in, 2, d_x, A), "ERR_INVALID", ": d_cv overlaps d_out")
# the meters need no setting.  Zero samples: nothing to do, whatever else is asked
case("nothing set", "meter", (0, 0, None, 99, 0, None, 0, None), "OK")
case("nothing set", "meter", (0, N, None, 2, 64, FAR, 1, None), "ERR_INVALID", ": d_rows must be given")
case("all set", "meter", (1 << 63, 0, None, 99, 0, 4, 0, 4), "OK")
# ... then, in the order the call looks: d_rows, row_channels, something to write, the alignments, the window, the windows' span, the overlaps
case("all set", "meter", (0, N, None, 2, 64, FAR, 1, None), "ERR_INVALID", ": d_rows must be given")
case("all set", "meter", (0, N, None, 99, 63, None, 0, None), "ERR_INVALID", ": d_rows must be given")
for rc in (0, 9):
    case("all set", "meter", (0, N, A, rc, 64, FAR, 1, None), "ERR_INVALID", ": row_channels must be 1 .. 8")
    case("all set", "meter", (0, N, A, rc, 64, None, 1, None), "ERR_INVALID", ": row_channels must be 1 .. 8")   # (... ahead of nothing to write)
case("all set", "meter", (0, N, A, 2, 64, None, 1, None), "ERR_INVALID", ": d_levels or d_totals must be given")
case("all set", "meter", (0, N, A, 2, 64, FAR + 4, 1, None), "ERR_INVALID", ": d_levels must be 8-byte aligned")
case("all set", "meter", (0, N, A, 2, 63, FAR + 4, 0, FARTHER + 4), "ERR_INVALID", ": d_levels must be 8-byte aligned")   # (... ahead of d_totals and the window)
case("all set", "meter", (0, N, A, 2, 64, None, 1, FARTHER + 4), "ERR_INVALID", ": d_totals must be 8-byte aligned")
case("all set", "meter", (0, N, A, 2, 63, FAR, 0, FARTHER + 4), "ERR_INVALID", ": d_totals must be 8-byte aligned")         # (... ahead of the window)
WINDOW = ": window must be at least SRACK_BUS_METER_MIN_WINDOW (64) samples"
case("all set", "meter", (0, N, A, 2, 63, FAR, 1, None), "ERR_INVALID", WINDOW)
case("all set", "meter", (0, N, A, 2, 63, FAR, 0, FARTHER), "ERR_INVALID", WINDOW)   # (... ahead of n_windows)
case("all set", "meter", (0, N, A, 2, 0, FAR, 1, None), "ERR_INVALID", WINDOW)
case("all set", "meter", (0, N, A, 2, 64, FAR, 0, None), "ERR_INVALID", ": n_windows must be at least 1")   # (64 is window enough)
case("all set", "meter", (0, N, A, 2, 64, A, 0, None), "ERR_INVALID", ": n_windows must be at least 1")     # (... ahead of the overlap)
SPAN = ": first_sample + n_samples exceeds n_windows * window"
case("all set", "meter", (64 - N + 1, N, A, 2, 64, FAR, 1, None), "ERR_INVALID", SPAN)        # one past the last window
case("all set", "meter", (3 * 64 - N + 1, N, A, 2, 64, FAR, 3, FARTHER), "ERR_INVALID", SPAN)
case("all set", "meter", (65, N, A, 2, 64, FAR, 1, None), "ERR_INVALID", SPAN)                # first_sample alone is past it
case("all set", "meter", ((1 << 64) - 8, N, A, 2, 64, FAR, 1, None), "ERR_INVALID", SPAN)     # (the sum would wrap to 8)
case("all set", "meter", ((1 << 64) - N, N, A, 2, 64, A, 1, None), "ERR_INVALID", SPAN)       # (... to 0; ahead of the overlap)
# ... (a call that ends with the last window passes that check: what it says next is the overlap; without d_levels the window is not looked at)
case("all set", "meter", (64 - N, N, FAR, 2, 64, FAR, 1, None), "ERR_INVALID", ": d_levels overlaps d_rows")
case("all set", "meter", (1 << 40, N, FAR, 2, 0, None, 0, FAR), "ERR_INVALID", ": d_totals overlaps d_rows")
for d_rows in (FAR, FAR + TOTALS - 4, FAR - ROWS + 4):
    case("all set", "meter", (0, N, d_rows, 2, 64, FAR, 1, None), "ERR_INVALID", ": d_levels overlaps d_rows")
    case("all set", "meter", (0, N, d_rows, 2, 64, None, 0, FAR), "ERR_INVALID", ": d_totals overlaps d_rows")
    case("all set", "meter", (0, N, d_rows, 2, 64, FAR, 1, FAR), "ERR_INVALID", ": d_levels overlaps d_rows")      # (d_levels ahead of d_totals)
    case("all set", "meter", (0, N, d_rows, 2, 64, FARTHER, 1, FAR), "ERR_INVALID", ": d_totals overlaps d_rows")
case("all set", "meter", (0, N, FAR + 3 * TOTALS - 4, 2, 64, FAR, 3, None), "ERR_INVALID", ": d_levels overlaps d_rows")   # (three windows deep)
for d_totals in (FAR, FAR + 3 * TOTALS - 8, FAR - TOTALS + 8):
    case("all set", "meter", (0, N, A, 2, 64, FAR, 3, d_totals), "ERR_INVALID", ": d_levels overlaps d_totals")
# ... (the rows begin where the levels end, in the totals that reach eight bytes back into the levels: the totals on the rows are reported)
case("all set", "meter", (0, N, FAR + 3 * TOTALS, 2, 64, FAR, 3, FAR + 3 * TOTALS - 8), "ERR_INVALID", ": d_totals overlaps d_rows")

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
            p.set_bus_shaper()
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
              "buses_master: d_master overlaps d_rows", "buses_reverb: d_bus_fx overlaps d_bus_mix",
              "buses_shaper" + IN_PART, "buses_shaper: d_cv overlaps d_out", "buses_shaper: d_rows and d_out must be given",
              "buses_shaper: no shapers set: call srack_buses_set_shaper first",
              "buses_meter: d_rows must be given", "buses_meter: d_levels or d_totals must be given", "buses_meter: d_levels must be 8-byte aligned",
              "buses_meter: d_totals must be 8-byte aligned", "buses_meter: window must be at least SRACK_BUS_METER_MIN_WINDOW (64) samples",
              "buses_meter: n_windows must be at least 1", "buses_meter" + SPAN, "buses_meter: d_levels overlaps d_rows",
              "buses_meter: d_totals overlaps d_rows", "buses_meter: d_levels overlaps d_totals"):
        assert t in texts, t
    for who in ("buses_send", "buses_vca", "buses_filter", "buses_shaper", "buses_master", "buses_meter"):
        assert who + ": row_channels must be 1 .. 8" in texts
