#!/usr/bin/env python3
"""What the progress previews cost: ms per diffusion step of a batch-64, latent-16 loop of 200 DDIM steps with previews off and on
(every = 1, snapshots = 0: one more 4 KB store per face and step), alternated on one build in one process (HIP events around the graph
replay loop, hd_get_profile).  With --parent DIR (a checkout of the parent commit with its library built) a second process runs the loop of
that tree in turn with this one, so that all three figures come from one machine and one stretch of time; the off-path claim -- this
build with previews off is not distinguishable from the parent -- is then judged against the spread of the parent's own repeats.
    python tools/preview_bench.py [--parent DIR] [--rounds 7] [--out profiles/r11_preview_bench.txt]"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, LAT, STEPS = 64, 16, 200


def worker(root):
    """One model of the tree at `root`; every line on stdin ("off" / "on" / "quit") runs one loop and prints its ms per step."""
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
    sch = schedulers.DDIMScheduler(clip_sample_range=3.0)
    sch.set_timesteps(STEPS)
    L.hd_set_profiling(m.engine.ctx, 1)
    has = hasattr(m, "enable_previews")

    def loop(on):
        if has:
            m.enable_previews(1, 0) if on else m.disable_previews()
        out = sampling.sample(m, x, crf, crl, sch)
        step_ms = ctypes.c_double()
        L.hd_get_profile(m.engine.ctx, None, ctypes.byref(step_ms), None, None)
        assert bool(torch.isfinite(out).all())
        if on:
            assert m.previews()[1].cpu().tolist() == [STEPS - 1] * B
        return step_ms.value

    loop(False)                                                        # captures the graphs
    print("ready %d" % int(has), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "quit":
            break
        print("%.6f" % loop(cmd == "on"), flush=True)


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
    ap.add_argument("--parent", help="checkout of the parent commit (library built): its loop is alternated with this tree's")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_preview_bench.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    this = Child(ROOT)
    parent = Child(os.path.abspath(a.parent)) if a.parent else None
    cols = ["previews off", "previews on"] + (["parent"] if parent else [])
    rows = []
    for _ in range(max(5, a.rounds)):
        r = [this.run("off"), this.run("on")]
        if parent:
            r.append(parent.run("off"))
        rows.append(r)
    this.close()
    if parent:
        parent.close()
    mean = lambda j: sum(r[j] for r in rows) / len(rows)  # noqa: E731
    lines = ["tools/preview_bench.py (MI355X): ms per diffusion step, batch %d, latent %d, %d DDIM steps per loop (HIP events around the graph replay" % (B, LAT, STEPS),
             "loop), %d alternations in one run.  previews on: every = 1, snapshots = 0 (hd_preview_config): 4 KB more per face and step." % len(rows), "",
             "round  " + "  ".join("%16s" % c for c in cols)]
    for i, r in enumerate(rows):
        lines.append("%5d  " % i + "  ".join("%16.4f" % v for v in r))
    lines.append("")
    for j, c in enumerate(cols):
        v = sorted(r[j] for r in rows)
        lines.append("%-16s mean %.4f  median %.4f  min %.4f  max %.4f  (spread %.4f ms)" % (c, mean(j), v[len(v) // 2], v[0], v[-1], v[-1] - v[0]))
    lines.append("")
    lines.append("on-path cost: previews on - off = %+.4f ms per step (%+.2f %%), reported, not gated" % (mean(1) - mean(0), 100 * (mean(1) - mean(0)) / mean(0)))
    if parent:
        v = [r[2] for r in rows]
        d, spread = mean(0) - mean(2), max(v) - min(v)
        lines.append("off-path: previews off - parent = %+.4f ms per step; the parent's own repeats spread over %.4f ms: %s"
                     % (d, spread, "not distinguishable from the parent" if abs(d) <= spread else "DISTINGUISHABLE from the parent"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
