"""The ladder's vote on its clamp behind the cubic (csrc/modules.hip.h, vcf_b4_bounded_lane; notes/r30.md) against the ladder, on the CPU.

VcfRegs, clamp1, vcf_polys, vcf_step and the vote are cut out of modules.hip.h as they stand, between the header's `host-probe begin` and
`host-probe end` lines (the header itself needs the HIP runtime), and
compiled by g++ with -ffp-contract=off and the real fmaf into tests/cpp/vcf_bound_probe.cpp, a stand-alone program.  It sweeps every f32
cutoff within 64 ulp of the vote's pass/fail threshold (at resonance 0, 0.25, 0.5 and 1), the cutoffs 0, 0.05, 0.6, 0.89, 0.9 and 10^6
random ones; for each, b4 in {+-1, +-0.95, +-the largest f32 below 0.95, random} and a fourth-stage operand b3' + b3 in {+-2, random}
(the stage and the cubic alone, contracted and literal form), and whole steps WITHOUT the fifth clamp from the corners of the state's box
and from inside it, and runs of 256 such steps.

    vote true  =>  |g| <= 0.95, in both forms, in the stage model, after a whole step, and on every step of a run
    some vote-false point leaves [-1, 1]   (the sweep has teeth)
    the stage model's own bound, 2p + |f| max(|b4|, 0.95) <= 2.83, passes points whose whole step leaves [-1, 1]: the clamps act at the
    END of a step, the fourth stage sees the step's own b3 unclamped, and the vote has to carry the resonance term p^4 q (the note's proof)
"""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "s-rack_amd", "csrc", "modules.hip.h")
PROBE = os.path.join(ROOT, "tests", "cpp", "vcf_bound_probe.cpp")

# modules.hip.h marks what the probe compiles: the lines between a BEGIN line and the next END line, three pieces
BEGIN, END = "// host-probe begin", "// host-probe end"


def excerpt():
    out, inside = [], False
    for line in open(HEADER).read().splitlines():
        if line.strip() in (BEGIN, END):
            assert inside == (line.strip() == END), "host-probe markers of modules.hip.h do not pair up"
            inside = not inside
        elif inside:
            out.append(line)
    assert not inside and out, "host-probe markers of modules.hip.h do not pair up"
    text = "\n".join(out) + "\n"
    for name in ("clamp1", "vcf_polys", "vcf_step", "vcf_b4_bounded_lane", "kVcfB4PreMax = 2.83f", "kVcfB4Bound = 0.95f", "if (kClampB4) s.b4 = clamp1<kMed3>(s.b4);"):
        assert name in text, name
    assert "__builtin_amdgcn_ballot" not in text and "#include" not in text
    return text


@pytest.fixture(scope="module")
def result(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcf_bound")
    (d / "vcf_bound_excerpt.tmp").write_text(excerpt())
    binary = str(d / "vcf_bound_probe")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", str(d), "-o", binary, PROBE, "-lm"], check=True)
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res, indent=1))
    return res


def test_the_header_says_what_the_probe_reads(result):
    assert result["bound"] == pytest.approx(0.95, abs=1e-7) and result["pre_max"] == pytest.approx(2.83, abs=1e-6)
    assert re.search(r"vcf_step<true, true, false>\(sv, x, lp, bp, hp\)", open(os.path.join(ROOT, "s-rack_amd", "csrc", "fused.hip.h")).read())


def test_sweep_covers_the_threshold(result):
    t = result["thresholds"]
    # resonance 0: the vote is 2p + |f| 0.95 <= 2.83, which turns between 0.89 and 0.9; more resonance, a lower threshold
    assert 0.89 < t[0] < 0.9, t
    assert t[0] > t[1] > t[2] > t[3] > 0.6, t
    assert result["cutoffs"] >= 1000000 + 5 + 4 * 129


def test_vote_true_keeps_the_cubic_inside_the_bound(result):
    st, sp, runs = result["stage"], result["step"], result["runs"]
    print("stage model: passing points", st["pass"], "of", st["n"], "max |g| contracted / literal", st["pass_max_g"], "max |pre|", st["pass_max_pre"])
    print("whole step:  passing points", sp["pass"], "of", sp["n"], "max |b4'| contracted / literal", sp["pass_max_b4"])
    print("runs of 256 steps:", runs)
    assert st["pass"] > 1000000 and sp["pass"] > 1000000 and runs["n"] > 10000
    assert st["pass_over"] == 0 and max(st["pass_max_g"]) <= 0.95
    assert sp["pass_over"] == 0 and max(sp["pass_max_b4"]) <= 0.95
    assert runs["over"] == 0 and runs["max_b4"] <= 0.95
    assert st["pass_max_pre"] <= 2.83 + 1e-5


def test_the_sweep_has_teeth(result):
    st, sp = result["stage"], result["step"]
    assert st["fail_over_one"] > 0 and max(st["fail_max_g"]) > 1.0
    assert sp["fail_over_one"] > 0 and max(sp["fail_max_b4"]) > 1.0


def test_the_fourth_stage_alone_is_no_bound(result):
    """2p + |f| max(|b4|, 0.95) <= 2.83 takes b3' + b3 as clamped; the step's own b3' is not (filter.rs:78-81)."""
    sp = result["step"]
    print("passing the fourth stage's bound alone:", sp["stage_only_pass"], "of which leave [-1, 1]:", sp["stage_only_over_one"], "max |b4'|", sp["stage_only_max_b4"])
    assert sp["stage_only_over_one"] > 0 and sp["stage_only_max_b4"] > 1.0
