"""The stream test of tests/test_gpu_voice_slots.py, in a process of its own (torch must start HIP before the library loads:
INTEGRATION.md section 3).  srack_render_buses with a slot table runs on a caller's stream while the DEFAULT stream is stalled (the
stall of tests/console_stream_driver.py), the table replaced by another slot table before the third call; nothing is synchronised
until the end.  `busy` records that the default stream had provably not finished when each call (and the replacement of the table) began, `busy_after`
whether it still had not when a call that uploads nothing returned.  This file only renders and records; the comparison is the test's.

    python tests/voice_slots_stream_driver.py <out.npz>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.console_stream_driver import DEV, Stall, busy  # noqa: E402  (starts torch's HIP, then loads the library)
import torch  # noqa: E402
import srack_pkg  # noqa: E402
from tests import voice_slots_ref as VR  # noqa: E402
from tests.test_gpu_mix_buses import maker  # noqa: E402

V, K, NB, CALLS, N = VR.STREAM_CASE


def main():
    S = srack_pkg.load()
    stall = Stall()
    (bus, gain), (bus2, gain2) = VR.stream_tables()
    q = maker(S, "cfg3", V)()
    q.set_bus_slots(NB, bus, gain)
    f32 = dict(dtype=torch.float32, device=DEV)
    bm, fr = torch.zeros((CALLS, NB, 2, N), **f32), torch.zeros((CALLS, 1, N, V), **f32)
    torch.cuda.synchronize()
    st, null, flags, after = torch.cuda.Stream(DEV), torch.cuda.default_stream(DEV), [], []
    for i in range(CALLS):
        stall(null)
        flags.append(busy(null))
        if i == 2:
            q.set_bus_slots(NB, bus2, gain2)   # the same n_buses, another table: it goes up again, behind the calls that read the old one
        q.render_buses_raw(N, bm[i].data_ptr(), d_frames=fr[i].data_ptr(), stream=st.cuda_stream)
        if i % 2 == 1:   # (calls 0 and 2 upload a table with a blocking copy, which waits for the default stream; these two upload nothing)
            after.append(busy(null))
    torch.cuda.synchronize()
    np.savez(sys.argv[1], bus_mix=bm.cpu().numpy(), frames=fr.cpu().numpy(), busy=np.array(flags), busy_after=np.array(after), info=np.array(q.info()), stall_ms=np.float64(stall.ms))


if __name__ == "__main__":
    main()
