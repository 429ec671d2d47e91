#!/usr/bin/env python3
"""What per-face spans cost per step: ms per diffusion step of batch-64, latent-16 loops of 200 steps, alternated in one run (HIP events
around the graph replay loop, hd_get_profile):
    hd_sample (DDIM), hd_sample_faces_multistep (DPM-Solver++ 2M, all start rows 0) and hd_sample_spans with whole-table spans on this build,
and, with --parent DIR (a checkout of the parent commit with its library built), hd_sample and hd_sample_faces_multistep of that tree in a
second process that takes turns with this one, so that all figures come from one machine and one stretch of time.  The spread of a column
over the alternations is the run-to-run spread of one build against itself.
    python tools/spans_bench.py [--parent DIR] [--rounds 7] [--out profiles/r10_spans_bench.txt]"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, LAT, STEPS = 64, 16, 200


def worker(root):
    """One model of the tree at `root`; every line on stdin ("sample" / "faces" / "spans" / "quit") runs one loop and prints its ms per step."""
    sys.path.insert(0, root)
    import torch
    from hifidiff_amd import _lib, schedulers, synth
    from hifidiff_amd.refiner import FacialRefiner
    torch.set_grad_enabled(False)
    L = _lib.lib()
    m = FacialRefiner(LAT)
    m.load_state_dict(synth.refiner_state_dict(LAT))
    m.to("cuda:0")
    x, crl, crf = [t.cuda() for t in synth.sample_inputs(B, LAT)]
    m.prepare(crf, crl)
    ctx = m.engine.ctx
    L.hd_set_profiling(ctx, 1)
    tabs = {}
    for name, s, cls in (("ddim", schedulers.DDIMScheduler(clip_sample=True, clip_sample_range=3.0), _lib.Schedule),
                         ("dpm", schedulers.DPMSolverMultistepScheduler(), _lib.ScheduleMS)):
        s.set_timesteps(STEPS)
        ts, coef = [t.float().contiguous() for t in s.coefficient_table()]
        sc = cls()
        sc.n_steps = STEPS
        sc.timesteps = ctypes.cast(ts.data_ptr(), ctypes.POINTER(ctypes.c_float))
        sc.coef = ctypes.cast(coef.data_ptr(), ctypes.POINTER(ctypes.c_float))
        tabs[name] = (sc, ts, coef)
    i32 = lambda v: (ctypes.c_int32 * B)(*([v] * B))                   # noqa: E731
    zero, end = i32(0), i32(STEPS)
    seeds = (ctypes.c_uint64 * B)(*range(1, B + 1))
    stream = torch.cuda.current_stream().cuda_stream
    has_spans = hasattr(L, "hd_sample_spans")

    def loop(cmd):
        xd = x.clone()
        if cmd == "sample":
            rc = L.hd_sample(ctx, xd.data_ptr(), ctypes.byref(tabs["ddim"][0]), None, 1, stream)
        elif cmd == "faces":
            rc = L.hd_sample_faces_multistep(ctx, xd.data_ptr(), ctypes.byref(tabs["dpm"][0]), zero, STEPS, zero, seeds, None, 1, stream)
        else:
            rc = L.hd_sample_spans(ctx, xd.data_ptr(), ctypes.byref(tabs["dpm"][0]), zero, end, zero, STEPS, zero, seeds, None, 1, stream)
        _lib.check(rc, ctx)
        torch.cuda.synchronize()
        _lib.check(L.hd_check(ctx), ctx)
        step_ms = ctypes.c_double()
        L.hd_get_profile(ctx, None, ctypes.byref(step_ms), None, None)
        assert bool(torch.isfinite(xd).all())
        return step_ms.value

    for cmd in ("sample", "faces") + (("spans",) if has_spans else ()):   # captures the graphs, computes the FiLM tables
        loop(cmd)
    print("ready %d" % int(has_spans), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        print("%.6f" % loop(cmd), flush=True)


class Child:
    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        line = self.p.stdout.readline()
        while line and not line.startswith("ready"):
            line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("the worker of %s ended before it was ready" % root)

    def run(self, cmd):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("the worker ended")
        return float(line)

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.flush()
        self.p.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--parent", help="checkout of the parent commit (library built): its loops are alternated with this tree's")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_spans_bench.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    this = Child(ROOT)
    parent = Child(os.path.abspath(a.parent)) if a.parent else None
    cols = ["hd_sample", "faces_multistep", "spans"] + (["parent hd_sample", "parent faces_ms"] if parent else [])
    rows = []
    for _ in range(max(5, a.rounds)):
        r = [this.run("sample"), this.run("faces"), this.run("spans")]
        if parent:
            r += [parent.run("sample"), parent.run("faces")]
        rows.append(r)
    this.close()
    if parent:
        parent.close()
    lines = ["tools/spans_bench.py (MI355X): ms per diffusion step, batch %d, latent %d, %d steps per loop (HIP events around the graph replay" % (B, LAT, STEPS),
             "loop), %d alternations in one run.  hd_sample: DDIM; faces_multistep / spans: DPM-Solver++ 2M with per-face keys, every face from row 0," % len(rows),
             "spans = the whole table for every face.", "",
             "round  " + "  ".join("%16s" % c for c in cols)]
    for i, r in enumerate(rows):
        lines.append("%5d  " % i + "  ".join("%16.4f" % v for v in r))
    lines.append("")
    for j, c in enumerate(cols):
        v = sorted(r[j] for r in rows)
        lines.append("%-16s median %.4f  min %.4f  max %.4f  (spread %.4f ms)" % (c, v[len(v) // 2], v[0], v[-1], v[-1] - v[0]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
