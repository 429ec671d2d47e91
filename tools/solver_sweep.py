#!/usr/bin/env python3
"""Solver report (GPU; a report, not a gate): how close few-step samplers get to the probability-flow ODE solution, and what a
face costs.  One synthetic batch (latent 16, batch 64); the reference trajectory is DDIM at 1000 steps with clip_sample=False
(the first-order solver at its finest grid).  Rows: DDIM at 10 / 20 / 50 steps and DPM-Solver++ 2M at 10 / 15 / 20 / 25 steps,
graph-replayed (sampling.sample), with rel-L2 of the final latents to the reference and ms per face (median of --reps timed
passes; the conditioning prologue is hoisted, so a pass is the loop alone).

    python tools/solver_sweep.py [--reps 3]            the whole table
    python tools/solver_sweep.py --ddim50-only [--reps 5]
        only the hd_sample DDIM-50 loop time: run alternately from this tree and from the tree before the multistep
        solver to see whether its history buffer costs the single-step path anything.

The weights are synthetic, so the distances say how well each solver integrates THIS network's ODE, nothing about face quality."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()                                                   # warm-up: FiLM table of the schedule, graph capture
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ddim50-only", action="store_true")
    a = ap.parse_args()
    import torch
    from hifidiff_amd import sampling, schedulers, synth
    from hifidiff_amd.refiner import FacialRefiner
    torch.set_grad_enabled(False)
    B = a.batch
    m = FacialRefiner(16)
    m.load_state_dict(synth.refiner_state_dict(16))
    m.to("cuda:0")
    x, crl, crf = (t.cuda() for t in synth.sample_inputs(B, 16))
    m.prepare(crf, crl)
    run = lambda s: sampling.sample(m, x, crf, crl, s, prepare=False)  # noqa: E731

    ddim50 = schedulers.DDIMScheduler(clip_sample=False)
    ddim50.set_timesteps(50)
    if a.ddim50_only:
        _, ms = timed(lambda: run(ddim50), a.reps)
        print(f"hd_sample DDIM-50 B={B}: {ms:.2f} ms per pass, {ms / B:.4f} ms per face ({os.path.basename(ROOT)})")
        return

    ref_s = schedulers.DDIMScheduler(clip_sample=False)
    ref_s.set_timesteps(1000)
    ref = run(ref_s).double()
    torch.cuda.synchronize()
    rows = []
    for name, steps in (("DDIM", 10), ("DDIM", 20), ("DDIM", 50), ("DPM++ 2M", 10), ("DPM++ 2M", 15), ("DPM++ 2M", 20), ("DPM++ 2M", 25)):
        s = schedulers.DDIMScheduler(clip_sample=False) if name == "DDIM" else schedulers.DPMSolverMultistepScheduler()
        s.set_timesteps(steps)
        out, ms = timed(lambda: run(s), a.reps)
        rel = float((out.double() - ref).norm() / ref.norm())
        rows.append((name, steps, rel, ms / B))
    print(f"solver sweep: latent 16, batch {B}, synthetic weights and inputs; reference = DDIM 1000 steps, clip_sample=False")
    print(f"{'solver':<10}{'steps':>6}{'rel-L2 to ref':>16}{'ms/face':>10}")
    for name, steps, rel, msf in rows:
        print(f"{name:<10}{steps:>6}{rel:>16.3e}{msf:>10.3f}")


if __name__ == "__main__":
    main()
