"""The stream tests of tests/test_gpu_console.py, in a process of its own (torch must start HIP before the library loads: INTEGRATION.md
section 3).  The bus console — send -> reverb -> VCA -> filter -> master, the chain of tests/console_ref.py — runs on the caller's
streams with nothing synchronised inside a scenario, every buffer a torch tensor uploaded beforehand, results copied out behind one
torch.cuda.synchronize() at the scenario's end.  This file only renders and records; the comparisons with the reference are the tests'.

A stream is STALLED by a spin kernel of about 20 ms in front of a cut's calls (torch.cuda._sleep, calibrated at start; a queue of
element-wise operations on a 256 MB tensor where that is missing or implausible), so that the calls have provably not run when the host
goes on to edit settings, read state back, destroy the stream or call on another stream.  `<scenario>_busy` records stream.query() == False
immediately before every such in-flight action.

    python tests/console_stream_driver.py <out.npz>
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

torch.cuda.init()
import srack_pkg  # noqa: E402
from tests import console_ref as CR  # noqa: E402
from tests.test_gpu_mix_buses import maker, mixed_gains  # noqa: E402

DEV = torch.device("cuda", 0)
STALL_MS = 20.0


# ---- stalling a stream ----------------------------------------------------------------------------------------------------------------------
class Stall:
    def __init__(self):
        self.how, self.cycles, self.ms = "torch.cuda._sleep", 0, 0.0
        try:
            one = self._time(lambda: torch.cuda._sleep(1_000_000))
            self.cycles = int(1_000_000 * STALL_MS / max(one, 1e-6))
            self.ms = self._time(lambda: torch.cuda._sleep(self.cycles))
        except (AttributeError, RuntimeError):
            self.ms = 0.0
        if not 2.0 <= self.ms <= 200.0:   # no _sleep, or a calibration that cannot be: element-wise operations on 256 MB instead
            self.how = "element-wise operations on 256 MB"
            self.big = torch.zeros(64 * 1024 * 1024, dtype=torch.float32, device=DEV)
            one = self._time(lambda: self.big.add_(1.0))
            self.cycles = max(1, int(round(STALL_MS / max(one, 1e-6))))
            self.ms = self._time(self._ops)

    @staticmethod
    def _time(f):
        f()   # (the first launch of a kernel loads its code)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def _ops(self, scale=1.0):
        for _ in range(max(1, int(self.cycles * scale))):
            self.big.add_(1.0)

    def __call__(self, stream, scale=1.0):
        with torch.cuda.stream(stream):
            if self.how == "torch.cuda._sleep":
                torch.cuda._sleep(max(1, int(self.cycles * scale)))
            else:
                self._ops(scale)


def busy(stream):
    return not stream.query()


# ---- the chain's buffers: one set per cut, disjoint, uploaded beforehand ------------------------------------------------------------------------
class Buffers:
    def __init__(self, rows, ctl, cuts):
        nb, ch, _ = rows.shape
        self.cuts, self.nb, self.ch = list(cuts), nb, ch
        f32 = dict(dtype=torch.float32, device=DEV)
        self.rows, self.ctl, self.sent, self.buf, self.fx, self.vca, self.env, self.master, self.stats_at = ([] for _ in range(9))
        at = 0
        for n in self.cuts:
            self.rows.append(torch.from_numpy(np.ascontiguousarray(rows[:, :, at:at + n])).to(DEV))
            self.ctl.append(torch.from_numpy(np.ascontiguousarray(ctl[:, at:at + n])).to(DEV))
            self.sent.append(torch.zeros((nb, ch, n), **f32))
            for held in (self.buf, self.fx, self.vca):
                held.append(torch.full((nb, 2, n), -54321.5, **f32))
            self.env.append(torch.full((nb, n), -54321.5, **f32))
            self.master.append(torch.full((2, n), -54321.5, **f32))
            self.stats_at.append(torch.zeros((2, CR.RM.STAT_COUNT), dtype=torch.float64, device=DEV))
            at += n
        self.stats = torch.zeros((2, CR.RM.STAT_COUNT), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()

    def enqueue(self, p, k, stream, before_master=None):
        """cut k's five calls on `stream`, the intermediates kept by copies on the same stream (vca and filter work in place)"""
        n, ptr = self.cuts[k], stream.cuda_stream
        buf = self.buf[k].data_ptr()
        p.send_raw(n, self.rows[k].data_ptr(), self.ch, self.sent[k].data_ptr(), ptr)
        p.bus_reverb_raw(n, self.sent[k].data_ptr(), buf, ptr)
        with torch.cuda.stream(stream):
            self.fx[k].copy_(self.buf[k])
        p.bus_vca_raw(n, buf, 2, self.ctl[k].data_ptr(), buf, self.env[k].data_ptr(), ptr)
        with torch.cuda.stream(stream):
            self.vca[k].copy_(self.buf[k])
        p.bus_filter_raw(n, buf, 2, self.env[k].data_ptr(), buf, ptr)
        if before_master is not None:
            before_master()
        p.master_raw(n, buf, 2, self.master[k].data_ptr(), self.stats.data_ptr(), ptr)
        with torch.cuda.stream(stream):
            self.stats_at[k].copy_(self.stats)

    def collect(self, out, tag, upto=None):
        """(behind a synchronisation)"""
        k = len(self.cuts) if upto is None else upto
        cat = lambda held: np.concatenate([x.cpu().numpy() for x in held[:k]], axis=-1)
        for key, held in (("sent", self.sent), ("fx", self.fx), ("vca", self.vca), ("env", self.env), ("vcf", self.buf), ("master", self.master)):
            out[f"{tag}_{key}"] = cat(held)
        out[f"{tag}_stats"] = self.stats_at[k - 1].cpu().numpy()
        out[f"{tag}_stats_per_cut"] = np.stack([x.cpu().numpy() for x in self.stats_at[:k]])


def main():
    t_start = time.perf_counter()
    S = srack_pkg.load()
    out = {}
    stall = Stall()
    out["stall_ms"], out["stall_cycles"], out["stall_how"] = np.float64(stall.ms), np.int64(stall.cycles), np.array(stall.how)
    print(f"stall: {stall.cycles} units of {stall.how} take {stall.ms:.2f} ms")
    rows, ctl, s = CR.case()
    cuts = list(CR.CUTS)
    N = len(cuts)

    # ---- 1. one stream, no synchronisation ---------------------------------------------------------------------------------------------------
    p, B, st = CR.host(S, s), Buffers(rows, ctl, cuts), torch.cuda.Stream(DEV)
    for k in range(N):
        B.enqueue(p, k, st)
    torch.cuda.synchronize()
    B.collect(out, "s1")

    # ---- 2. edits in flight: the stream stalled in front of every cut, one host action per boundary while the cut has not run ------------------
    for run in ("grow", "primed"):
        edits = CR.edits(s, run)
        p, B, st = CR.host(S, s), Buffers(rows, ctl, cuts), torch.cuda.Stream(DEV)
        if run == "primed":   # the scratch of the sends and of the master at its final size, every state as new
            P = Buffers(rows[:, :, :max(cuts)], ctl[:, :max(cuts)], [max(cuts)])
            P.enqueue(p, 0, st)
            torch.cuda.synchronize()
            for stage in ("reverb", "filter", "vca"):
                CR.reset_on_device(p, stage)
            B.stats.zero_()
            torch.cuda.synchronize()
        now, flags = s, []
        for k in range(N):
            if k > 0:
                flags.append(busy(st))      # cut k - 1 is enqueued behind its stall: it has not run
                if k == CR.STATE_READS[run]:
                    out[f"s2{run}_vca_state"], out[f"s2{run}_vcf_state"] = p.bus_vca_state(), p.bus_filter_state()
                for e in edits:
                    if e.cut != k:
                        continue
                    if e.change is None:
                        CR.reset_on_device(p, e.stage)
                    else:
                        now = now.copy()
                        e.change(now)
                        CR.push(p, now, e.stage)
            stall(st)
            B.enqueue(p, k, st)
        torch.cuda.synchronize()
        B.collect(out, "s2" + run)
        out[f"s2{run}_busy"] = np.array(flags)
        out[f"s2{run}_vca_state_end"], out[f"s2{run}_vcf_state_end"] = p.bus_vca_state(), p.bus_filter_state()

    # ---- 3a. two streams take turns; the caller orders only its own buffer (the statistics the master adds to) ------------------------------------
    p, B = CR.host(S, s), Buffers(rows, ctl, cuts)
    two, flags, last = (torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)), [], None
    for k in range(N):
        st = two[k % 2]
        if k % 2 == 0:
            stall(st)
        else:
            flags.append(busy(two[0]))      # stream A has not run cut k - 1: the library alone keeps B's calls behind it
        B.enqueue(p, k, st, before_master=(lambda: st.wait_event(last)) if last is not None else None)
        last = torch.cuda.Event()
        last.record(st)
    torch.cuda.synchronize()
    B.collect(out, "s3a")
    out["s3a_busy"] = np.array(flags)

    # ---- 3b. shared scratch, independent data: the same stage on two streams at once, the second up to 120 us ahead of or behind the first, in steps of 5 --------
    ref, _, _ = CR.render(rows, ctl, s, cuts)   # (inputs only: what the tests compare with is computed there)
    pairs = 48
    for stage in ("master", "sends"):
        p = CR.host(S, s)
        x, y = (ref["vcf"], ref["fx"]) if stage == "master" else (rows[:, :, :700], rows[::-1, :, :700])
        dx, dy = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
        shape = (2, x.shape[2]) if stage == "master" else x.shape
        ox, oy = torch.zeros((pairs,) + shape, dtype=torch.float32, device=DEV), torch.zeros((pairs,) + shape, dtype=torch.float32, device=DEV)
        a, b = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
        torch.cuda.synchronize()
        flags = []

        def call(d_in, d_out, stream):
            if stage == "master":
                p.master_raw(x.shape[2], d_in.data_ptr(), 2, d_out.data_ptr(), None, stream.cuda_stream)
            else:
                p.send_raw(x.shape[2], d_in.data_ptr(), 2, d_out.data_ptr(), stream.cuda_stream)

        per_us = stall.cycles / (stall.ms * 1000.0)
        for i in range(pairs):
            # both streams start their stall together (the caller's events: they order nothing inside the pair); B's is a little longer or shorter
            ea, eb = torch.cuda.Event(), torch.cuda.Event()
            ea.record(a)
            eb.record(b)
            a.wait_event(eb)
            b.wait_event(ea)
            stall(a, 0.25)
            call(dx, ox[i], a)
            flags.append(busy(a))
            extra = (i - pairs // 2) * 5.0 * per_us / stall.cycles if stall.how == "torch.cuda._sleep" else 0.0
            stall(b, max(0.01, 0.25 + extra))
            call(dy, oy[i], b)
        torch.cuda.synchronize()
        out[f"s3b_{stage}_x"], out[f"s3b_{stage}_y"], out[f"s3b_{stage}_busy"] = ox.cpu().numpy(), oy.cpu().numpy(), np.array(flags)

    # ---- 3c. shared state: one stateful stage alone, its cuts alternating between a stalled stream and one that is not ---------------------------
    at = np.concatenate([[0], np.cumsum(cuts)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for stage in ("vca", "filter", "reverb"):
        p = CR.host(S, s)
        src = {"vca": ref["fx"], "filter": ref["vca"], "reverb": ref["sent"]}[stage]
        ins = [up(src[:, :, at[k]:at[k + 1]]) for k in range(N)]
        side = [up((ctl if stage == "vca" else ref["env"])[:, at[k]:at[k + 1]]) for k in range(N)]
        outs = [torch.zeros((70, 2, n), dtype=torch.float32, device=DEV) for n in cuts]
        envs = [torch.zeros((70, n), dtype=torch.float32, device=DEV) for n in cuts]
        two, flags = (torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)), []
        torch.cuda.synchronize()
        for k in range(N):
            st = two[k % 2]
            if k % 2 == 0:
                stall(st)
            else:
                flags.append(busy(two[0]))
            if stage == "vca":
                p.bus_vca_raw(cuts[k], ins[k].data_ptr(), 2, side[k].data_ptr(), outs[k].data_ptr(), envs[k].data_ptr(), st.cuda_stream)
            elif stage == "filter":
                p.bus_filter_raw(cuts[k], ins[k].data_ptr(), 2, side[k].data_ptr(), outs[k].data_ptr(), st.cuda_stream)
            else:
                p.bus_reverb_raw(cuts[k], ins[k].data_ptr(), outs[k].data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        key = {"vca": "vca", "filter": "vcf", "reverb": "fx"}[stage]
        out[f"s3c_{stage}_{key}"] = np.concatenate([x.cpu().numpy() for x in outs], axis=-1)
        if stage == "vca":
            out["s3c_vca_env"] = np.concatenate([x.cpu().numpy() for x in envs], axis=-1)
        out[f"s3c_{stage}_busy"] = np.array(flags)

    # ---- 4. streams and state that go away -----------------------------------------------------------------------------------------------------------
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    p, B = CR.host(S, s), Buffers(rows, ctl, cuts)
    ra, rb = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(ra), 1) == 0 and hip.hipStreamCreateWithFlags(C.byref(rb), 1) == 0  # hipStreamNonBlocking
    sa, sb = torch.cuda.ExternalStream(ra.value, device=DEV), torch.cuda.ExternalStream(rb.value, device=DEV)
    for k in range(5):
        B.enqueue(p, k, sa)
    del sa
    assert hip.hipStreamDestroy(ra) == 0     # right behind the last call (work in flight completes; the handle is dead)
    stall(sb)
    for k in range(5, N):                    # (cut 5 is the longest: nothing behind the stall makes the host wait for it)
        B.enqueue(p, k, sb)
    flags = [busy(sb)]
    p.set_buses(33)                          # another n_buses: every stage's state, tables and scratch go, behind the calls that use them
    torch.cuda.synchronize()
    B.collect(out, "s4")
    out["s4_busy"] = np.array(flags)
    rows33, ctl33, s33 = CR.case(33, 2, 400, CR.SEED3 + 1, 3, 48000)
    B33 = Buffers(rows33, ctl33, [400])
    CR.push_all(p, s33)
    B33.enqueue(p, 0, sb)
    torch.cuda.synchronize()
    B33.collect(out, "s4new")
    del sb
    assert hip.hipStreamDestroy(rb) == 0

    # ---- 5. srack_render_buses on a stream, the voice -> bus table replaced in flight -----------------------------------------------------------------
    V, T, calls = 70, 300, 4
    n = T // calls
    rng = np.random.default_rng(V + T)
    bus, gain = rng.permutation(V), mixed_gains(V, rng)
    bus2, gain2 = rng.permutation(V), mixed_gains(V, rng)
    make = maker(S, "cfg3", V)

    def voices(tag, stream, edit):
        q = make()
        q.set_buses(V, bus, gain)
        CR.push(q, s, "sends")
        CR.push(q, s, "master")
        f32 = dict(dtype=torch.float32, device=DEV)
        bm, sent, ms = torch.zeros((calls, V, 2, n), **f32), torch.zeros((calls, V, 2, n), **f32), torch.zeros((calls, 2, n), **f32)
        torch.cuda.synchronize()
        ptr, flags = (stream.cuda_stream if stream is not None else None), []
        for i in range(calls):
            if i == 2 and edit:
                if stream is not None:
                    flags.append(busy(stream))
                q.set_buses(V, bus2, gain2)   # the same n_buses: the console stays, the table goes up again
            if stream is not None:
                stall(stream)
            q.render_buses_raw(n, bm[i].data_ptr(), stream=ptr)
            q.send_raw(n, bm[i].data_ptr(), 2, sent[i].data_ptr(), ptr)
            q.master_raw(n, sent[i].data_ptr(), 2, ms[i].data_ptr(), None, ptr)
            if stream is None:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        join = lambda t: np.concatenate(list(t.cpu().numpy()), axis=-1)
        out[f"{tag}_bus_mix"], out[f"{tag}_sent"], out[f"{tag}_master"] = join(bm), join(sent), join(ms)
        if flags:
            out[f"{tag}_busy"] = np.array(flags)

    voices("s5null", None, True)
    voices("s5plain", None, False)
    voices("s5", torch.cuda.Stream(DEV), True)

    out["driver_seconds"] = np.float64(time.perf_counter() - t_start)
    print(f"driver: {float(out['driver_seconds']):.2f} s behind the imports")
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
