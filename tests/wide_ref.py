"""The wide family's cases, references and checker (tests/test_wide_fuzz_host.py, tests/test_gpu_wide_fuzz.py; TEST INFRASTRUCTURE).

random_wide_patch (tests/fuzz_patches.py) draws settings beyond the sliders; here are the seeds both suites run, voice 0's oracle render
with a class of wide values clamped back or not (the guards' question "is this class heard"), and the one checker both suites judge by."""
import functools
import os

import numpy as np

from tests.fuzz_patches import WIDE_CLASSES, WIDE_SUBCLASSES, random_wide_patch

FAMILIES = {"plain": list(range(60)), "noise": list(range(20)), "nonlin": list(range(2000, 2015)), "special": list(range(40))}
CASES = [(family, seed) for family, seeds in FAMILIES.items() for seed in seeds]
KINDS = WIDE_CLASSES + WIDE_SUBCLASSES


def draw(family, seed, clamp=()):
    """-> (B, build, overrides) of one case.  The NonLinear family is FUZZ_NONLIN's, as in tests/test_gpu_fuzz.py: set for the draw alone."""
    before = os.environ.pop("FUZZ_NONLIN", None)
    try:
        if family == "nonlin":
            os.environ["FUZZ_NONLIN"] = "1"
        return random_wide_patch(seed, noise=family == "noise", special=family == "special", clamp=clamp)
    finally:
        os.environ.pop("FUZZ_NONLIN", None)
        if before is not None:
            os.environ["FUZZ_NONLIN"] = before


def sizes(B):
    """V, T of a device case: past the first control chunk (1024) and, at buffer_size 1024, past two ring periods — tests/test_gpu_fuzz.py's"""
    return (67, 1300) if B < 1024 else (131, 2300)


@functools.lru_cache(maxsize=None)
def voice0(family, seed, clamp=()):
    """voice 0's oracle render, [channels][T] f32 (read-only: shared between the guards), T as on the device"""
    from oracle import oracle
    B, build, overrides = draw(family, seed, clamp)
    V, T = sizes(B)
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o)
    for m, f, fn in overrides:
        o.set_field(ids[m], f, float(fn(V)[0]))
    a = o.render(T)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=4)
def reference(family, seed):
    """a device case's reference: (V, T, overrides [(module id, field, values)], frames [channels][T][V] f32, read-only, the oracle's plan)"""
    from oracle import oracle
    B, build, overrides = draw(family, seed)
    V, T = sizes(B)
    o = oracle.OraclePatch(48000, B, 2)
    ids = build(o)
    ov = [(ids[m], f, fn(V)) for m, f, fn in overrides]
    ref, _ = o.render_batch(V, T, ov, threads=8)
    ref.setflags(write=False)
    return V, T, ov, ref, o.plan()


def differs(a, b, by=1e-2):
    """two renders differ by more than `by` somewhere, or are finite in different places"""
    fa, fb = np.isfinite(a), np.isfinite(b)
    if (fa != fb).any():
        return True
    both = fa & fb
    return bool(both.any() and np.abs(a[both].astype(np.float64) - b[both].astype(np.float64)).max() > by)


def check(got, ref, bits):
    """-> None, or what is wrong.  bits: every sample the reference's bit for bit, a NaN for a NaN (x86's default NaN is 0xffc00000, the
    GPU's 0x7fc00000).  Otherwise the contract: |got - ref| <= 1e-5 max(|ref|, 1) where both are finite, NaNs and infinities at the
    reference's positions, an infinity with the reference's sign."""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    if got.shape != ref.shape:
        return f"shape {got.shape} against {ref.shape}"
    if bits:
        same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
        return None if same.all() else f"{1 - same.mean():.5f} of the samples differ"
    if not (np.isnan(got) == np.isnan(ref)).all():
        return "NaNs at other positions"
    if not (np.isinf(got) == np.isinf(ref)).all():
        return "infinities at other positions"
    inf = np.isinf(ref)
    if not (np.signbit(got[inf]) == np.signbit(ref[inf])).all():
        return "an infinity of the other sign"
    ok = np.isfinite(ref)
    r64 = ref.astype(np.float64)[ok]
    err = np.abs(got.astype(np.float64)[ok] - r64) / np.maximum(np.abs(r64), 1.0)
    if err.size and float(err.max()) > 1e-5:
        return f"max rel err {float(err.max()):.2e}, {float((err > 1e-5).mean()):.5f} of the samples outside"
    return None


def worst(got, ref):
    """the largest |got - ref| / max(|ref|, 1) over the samples finite in both (for the notes: measured, not a bar)"""
    ok = np.isfinite(ref) & np.isfinite(got)
    r64 = np.asarray(ref, dtype=np.float64)[ok]
    err = np.abs(np.asarray(got, dtype=np.float64)[ok] - r64) / np.maximum(np.abs(r64), 1.0)
    return float(err.max()) if err.size else 0.0
