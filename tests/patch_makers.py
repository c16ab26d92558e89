"""Patch factories the GPU tests share: a fresh patch of a named workload per call, every call the same voices."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def patch_maker(S, B, build, overrides, V):
    def make():
        p = S.Patch(48000, B, 2)
        ids = build(p)
        p.configure_voices(V)
        for m, f, v in overrides(ids):
            p.set_voice_field(m, f, v)
        return p
    return make


def p2_overrides(S, V):
    beta, index = S.p2_voice_params(V)
    return lambda ids: [(ids["mul_fb"], S.MATH_CONSTANT, beta), (ids["mul_idx"], S.MATH_CONSTANT, index)]


def workload_maker(S, w, B, V):
    """`w`: "p2" (the FM pair at buffer_size B) or one of bench.py's workloads (at the buffer_size it has there)"""
    if w == "p2":
        return patch_maker(S, B, S.build_p2, p2_overrides(S, V), V)
    B2, build, overrides = S.bench_workload(w, V)
    return patch_maker(S, B2, build, overrides, V)
