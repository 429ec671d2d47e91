#!/usr/bin/env python3
"""What the inpainting blend costs: ms per diffusion step of a batch-64, latent-16 loop of 200 DDPM steps, unmasked and with every face
masked, alternated on one build in one process (HIP events around the graph replay loop, hd_get_profile).  With --parent DIR (a checkout
of the parent commit with its library built) a second process runs the unmasked loop of that tree in turn with this one, so that all three
figures come from one machine and one stretch of time.
    python tools/mask_bench.py [--parent DIR] [--rounds 5] [--out profiles/r09_mask_bench.txt]"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, LAT, STEPS = 64, 16, 200


def worker(root):
    """One model of the tree at `root`; every line on stdin ("plain" / "masked" / "quit") runs one loop and prints its ms per step."""
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
    sch = schedulers.DDPMScheduler(clip_sample=True, clip_sample_range=3.0)
    sch.timesteps = sch.timesteps[:STEPS]
    L.hd_set_profiling(m.engine.ctx, 1)
    mask = torch.zeros((B, LAT, LAT))
    mask[:, 4:12, 2:14] = 1.0

    def loop(masked):
        kw = dict(mask=mask, known=crl, known_noise=x) if masked else {}
        out = sampling.sample(m, x, crf, crl, sch, seed=1, **kw)
        step_ms = ctypes.c_double()
        L.hd_get_profile(m.engine.ctx, None, ctypes.byref(step_ms), None, None)
        assert bool(torch.isfinite(out).all())
        return step_ms.value

    loop(False)                                                        # captures the graphs
    print("ready %d" % int(hasattr(L, "hd_mask_faces")), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        print("%.6f" % loop(cmd == "masked"), flush=True)


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
    ap.add_argument("--parent", help="checkout of the parent commit (library built): its unmasked loop is alternated with this tree's")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_mask_bench.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    this = Child(ROOT)
    parent = Child(os.path.abspath(a.parent)) if a.parent else None
    cols = ["unmasked", "masked"] + (["parent unmasked"] if parent else [])
    rows = []
    for _ in range(max(5, a.rounds)):
        r = [this.run("plain"), this.run("masked")]
        if parent:
            r.append(parent.run("plain"))
        rows.append(r)
    this.close()
    if parent:
        parent.close()
    lines = ["tools/mask_bench.py (MI355X): ms per diffusion step, batch %d, latent %d, %d DDPM steps per loop (HIP events around the graph replay" % (B, LAT, STEPS),
             "loop), %d alternations in one run.  masked: every face carries a box mask (hd_mask_faces)." % len(rows), "",
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
