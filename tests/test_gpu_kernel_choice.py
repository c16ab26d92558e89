"""Which kernel renders a patch (csrc/render.hip, pick_kernel) and what it writes in every output mode.

One table for every name srack_render_info can report.  Per row: the name; frames only and mix only give the bits of frames + mix (each output
mode is its own instantiation of a hand-written kernel, its own compilation of a specialised one); a render that writes nothing advances the
voices as one that writes everything; reserving first changes neither the choice nor a bit."""
import numpy as np
import pytest

import srack_pkg
from tests.patch_makers import bits, workload_maker

pytestmark = pytest.mark.gpu

EXACT, NO_FUSION, NO_HOIST, NO_SPEC, SPEC, KEEP = 1, 2, 4, 16, 32, 64
T2 = 1000

# (workload, buffer_size, V, T, flags, kernel).  V = 4097: the rules that only hold from 4096 voices up (the dispatcher's own choice of a
# specialised kernel); T = 3000 / 5000 at buffer_size 1024: either side of the shortest call the time-parallel FM pair takes (4096 samples)
CHOICES = [
    ("cfg3", 1024, 100, 5000, 0, "render_voice_chain_track"),
    ("cfg3", 1024, 257, 3000, EXACT, "render_voice_chain_track"),
    ("cfg3", 1024, 4097, 5000, 0, "render_voice_chain_track"),
    ("cfg3", 1024, 257, 5000, NO_HOIST, "render_voice_chain"),
    ("cfg3", 1024, 20, 3000, NO_HOIST | EXACT, "render_voice_chain"),
    ("cfg3", 1024, 100, 3000, NO_FUSION, "render_interp"),
    ("cfg3", 1024, 257, 5000, NO_FUSION | SPEC, "render_specialized"),
    ("cfg3_poly", 1024, 4097, 5000, 0, "render_specialized"),
    ("cfg3_poly", 1024, 4097, 5000, NO_SPEC, "render_voice_chain"),
    ("cfg3_poly", 1024, 100, 5000, 0, "render_voice_chain"),
    ("p3", 1024, 100, 5000, 0, "render_voice_chain_seq"),
    ("p3", 1024, 257, 5000, SPEC, "render_specialized"),
    ("p2", 1, 257, 5000, 0, "render_fm_pair_x"),
    ("p2", 1, 100, 5000, KEEP, "render_fm_pair"),
    ("p2", 1, 20, 3000, EXACT, "render_fm_pair"),  # (the two-wave split launch)
    ("p2", 1, 4097, 3000, KEEP, "render_specialized"),
    ("p2", 1, 4097, 3000, KEEP | NO_SPEC, "render_fm_pair"),
    ("p2", 1024, 100, 3000, KEEP, "render_fm_pair_ring"),  # (under the time-parallel kernel's shortest call)
    ("p2", 1024, 257, 3000, EXACT, "render_fm_pair_ring"),
    ("p2", 1024, 257, 5000, KEEP, "render_fm_pair_block"),
    ("p2", 1024, 100, 5000, 0, "render_fm_pair_block_x"),
    ("p2", 1024, 100, 3000, 0, "render_interp"),
    ("p2", 1024, 20, 5000, SPEC, "render_specialized"),
]


@pytest.fixture(scope="module")
def S():
    return srack_pkg.load()


def kernel_of(p):
    return p.info().split("kernel=")[-1]


@pytest.mark.parametrize("w,B,V,T,flags,kernel", CHOICES)
def test_kernel_choice_and_output_modes(S, w, B, V, T, flags, kernel):
    make = workload_maker(S, w, B, V)
    both = make()
    fr, mx = both.render(T, flags=flags)
    assert kernel_of(both) == kernel, both.info()
    # frames only, mix only: the same kernel, the same bits
    p = make()
    fr1, none = p.render(T, mix=False, flags=flags)
    assert none is None and kernel_of(p) == kernel, p.info()
    np.testing.assert_array_equal(bits(fr1), bits(fr))
    p = make()
    none, mx2 = p.render(T, frames=False, flags=flags)
    assert none is None and kernel_of(p) == kernel, p.info()
    np.testing.assert_array_equal(bits(mx2), bits(mx))
    # nothing written: the voices advance the same
    p = make()
    assert p.render(T, frames=False, mix=False, flags=flags) == (None, None)
    assert kernel_of(p) == kernel, p.info()
    fr_next, mx_next = both.render(T2, flags=flags)
    fr3, mx3 = p.render(T2, flags=flags)
    np.testing.assert_array_equal(bits(fr3), bits(fr_next))
    np.testing.assert_array_equal(bits(mx3), bits(mx_next))
    # reserved first
    p = make()
    p.reserve(T, flags=flags)
    fr4, mx4 = p.render(T, flags=flags)
    assert kernel_of(p) == kernel, p.info()
    np.testing.assert_array_equal(bits(fr4), bits(fr))
    np.testing.assert_array_equal(bits(mx4), bits(mx))
