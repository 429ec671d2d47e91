#!/usr/bin/env python3
"""What the low-pass fidelity guidance costs: ms per diffusion step of a batch-64, latent-16 loop of 200 DDIM steps with guidance never
enabled, and with all 64 faces guided at N = 1, 4 and 16 (the step then ends with guided_update_kernel), alternated on one build in one
process (HIP events around the graph replay loop, hd_get_profile).  With --parent DIR (a checkout of the parent commit with its library
built) a second process runs the plain loop of that tree in turn with this one, so that all figures come from one machine and one stretch
of time.  The guided worker is a second process of this tree: the "never enabled" worker never calls hd_guide_config.
    python tools/guide_bench.py [--parent DIR] [--rounds 5] [--out profiles/r14_guide_bench.txt]"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, LAT, STEPS = 64, 16, 200


def worker(root):
    """One model of the tree at `root`; every line on stdin ("plain" / "guided N" / "quit") runs one loop and prints its ms per step."""
    sys.path.insert(0, root)
    import torch
    from hifidiff_amd import _lib, sampling, schedulers, synth
    from hifidiff_amd.refiner import FacialRefiner
    torch.set_grad_enabled(False)
    L = _lib.lib()
    m = FacialRefiner(LAT)
    m.load_state_dict(synth.refiner_state_dict(LAT))
    m.to("cuda:0")
    x, crl, crf = [t.cuda() for t in synth.sample_inputs(B, LAT)]
    sch = schedulers.DDIMScheduler(clip_sample=True, clip_sample_range=3.0)
    sch.set_timesteps(STEPS)
    L.hd_set_profiling(m.engine.ctx, 1)

    def loop(scale):
        kw = dict(guide=crl, guide_weight=0.5, guide_scale=scale) if scale else {}
        out = sampling.sample(m, x, crf, crl, sch, **kw)
        step_ms = ctypes.c_double()
        L.hd_get_profile(m.engine.ctx, None, ctypes.byref(step_ms), None, None)
        assert bool(torch.isfinite(out).all())
        return step_ms.value

    loop(0)                                                            # captures the graphs
    print("ready %d" % int(hasattr(L, "hd_guide_faces")), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        print("%.6f" % loop(int(cmd.split()[1]) if cmd.startswith("guided") else 0), flush=True)


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
    ap.add_argument("--parent", help="checkout of the parent commit (library built): its plain loop is alternated with this tree's")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_guide_bench.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    never, guided = Child(ROOT), Child(ROOT)                            # guidance never enabled / enabled by its first guided loop
    parent = Child(os.path.abspath(a.parent)) if a.parent else None
    scales = (1, 4, 16)
    cols = (["parent"] if parent else []) + ["never enabled"] + ["guided N=%d" % n for n in scales]
    rows = []
    for _ in range(max(5, a.rounds)):
        r = [parent.run("plain")] if parent else []
        r.append(never.run("plain"))
        r += [guided.run("guided %d" % n) for n in scales]
        rows.append(r)
    for c in (never, guided, parent):
        if c:
            c.close()
    lines = ["tools/guide_bench.py (MI355X): ms per diffusion step, batch %d, latent %d, %d DDIM steps per loop (HIP events around the graph replay" % (B, LAT, STEPS),
             "loop), %d alternations in one run.  parent: the parent commit's build.  never enabled: this build, hd_guide_config never called." % len(rows),
             "guided: all %d faces guided towards their coarse latent, w = 0.5 on every row (one more launch per step)." % B, "",
             "round  " + "  ".join("%14s" % c for c in cols)]
    for i, r in enumerate(rows):
        lines.append("%5d  " % i + "  ".join("%14.4f" % v for v in r))
    lines.append("")
    med = {}
    for j, c in enumerate(cols):
        v = sorted(r[j] for r in rows)
        med[c] = v[len(v) // 2]
        lines.append("%-14s median %.4f  min %.4f  max %.4f  (spread %.4f ms)" % (c, v[len(v) // 2], v[0], v[-1], v[-1] - v[0]))
    lines.append("")
    for n in scales:
        lines.append("guided N=%-2d - never enabled: %+.2f us per step (medians)" % (n, 1e3 * (med["guided N=%d" % n] - med["never enabled"])))
    if parent:
        lines.append("never enabled - parent:      %+.2f us per step (medians)" % (1e3 * (med["never enabled"] - med["parent"])))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
