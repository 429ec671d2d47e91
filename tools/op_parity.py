#!/usr/bin/env python3
"""Op-by-op parity of the HIP launch programs against the CPU oracle (bf16-emulation mode).

Runs on the GPU box:  python tools/op_parity.py [--batch 2] [--latent 16] [--out gpurun_out/op_parity.txt]
For every launch of the conditioning prologue and of one denoiser evaluation, the program is run up to
and including that launch, its output buffer is read back and compared with the oracle's tap of the
same name.  The first op whose error jumps is the broken one.  (Test infrastructure: uses oracle/.)
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from forced import read_op                                # noqa: E402
from hifidiff_amd import _lib, synth                      # noqa: E402
from hifidiff_amd.refiner import FacialRefiner            # noqa: E402
from oracle import hifidiff_oracle as O                   # noqa: E402


def to_rows(name, t, s):
    """oracle tap (NCHW) -> the flat layout of the HIP buffer"""
    if name == "ending":
        return t.reshape(-1)
    if name == "idc_conv":
        B = t.shape[0]
        return t.reshape(B, 2048, s, s).permute(0, 2, 3, 1).reshape(-1)
    if t.dim() == 4:
        return t.permute(0, 2, 3, 1).reshape(-1)
    return t.reshape(-1)


def compare(name, got, ref):
    if got.numel() != ref.numel():
        return name, float("nan"), float("nan"), f"size {got.numel()} vs {ref.numel()}"
    d = (got.double() - ref.double())
    rel = float(d.norm() / ref.double().norm().clamp_min(1e-30))
    return name, rel, float(d.abs().max()), ""


def oracle_taps(P, x, crl, crf, t):
    taps = {}
    cond = O.Conditioning(P, crl, crf, prec=O.BF16, taps=taps)
    O.fused_denoiser(P, x, t, cond=cond, prec=O.BF16, taps=taps)
    return taps


def noise_floor(P, x, crl, crf, t, taps, eps=2e-7):
    """The emulation's own sensitivity: the same bf16-operand oracle on inputs perturbed by a relative 2e-7 (an fp32
    accumulation-order difference).  Where two evaluations differ by more than a fraction of a bf16 ulp their operand
    roundings decorrelate, so the difference grows tap by tap to ~1e-2 at the middle level with NO difference in the
    arithmetic: a HIP-vs-oracle error is only meaningful relative to this curve (Oracle and parity)."""
    g = torch.Generator().manual_seed(7)
    pert = lambda v: v * (1 + eps * torch.randn(v.shape, generator=g))       # noqa: E731
    other = oracle_taps(P, pert(x), pert(crl), pert(crf), t)
    floor = {}
    for k, v in taps.items():
        d = (other[k].double() - v.double()).norm() / v.double().norm().clamp_min(1e-30)
        floor[k] = float(d)
    return floor


def scan(model, P, x, crl, crf, t, report, which, taps=None, floor=None, slack=(1.5, 2.5e-3)):
    """Returns the worst rel-L2 over the launches; with `floor` (noise_floor) also flags every launch whose error
    exceeds slack[0] * floor + slack[1] (slack[1] covers the bf16 storage of G / G2 / pooled that the fp32 taps lack)."""
    L = _lib.lib()
    e = model.engine
    if taps is None:
        taps = oracle_taps(P, x, crl, crf, t)
    s = e.latent_res // 16
    worst = 0.0
    if which == 1:
        L.hd_debug_limit_ops(e.ctx, 1, -1)
        e.prepare(crl, cr_face=crf)
    n = L.hd_num_ops(e.ctx, which)
    xd = x.cuda()
    for i in range(n):
        name = L.hd_debug_op_name(e.ctx, which, i).decode()
        L.hd_debug_limit_ops(e.ctx, which, i + 1)
        if which == 1:
            e.prepare(crl, cr_face=crf)
        else:
            e.eps(xd, t)
        if name not in taps:
            report.append(f"{which}:{i:3d} {name:45s} (no tap)")
            continue
        nm, rel, mx, note = compare(name, read_op(e.ctx, which, i), to_rows(name, taps[name], s))
        lim = 5e-3 if floor is None else slack[0] * floor.get(name, 0.0) + slack[1]
        flag = "  <<<<<<" if not (rel < lim) else ""
        worst = max(worst, rel if rel == rel else 1e9)
        fl = "" if floor is None else f" floor {floor.get(name, 0.0):.3e} limit {lim:.3e}"
        report.append(f"{which}:{i:3d} {name:45s} rel {rel:.3e} maxabs {mx:.3e}{fl} {note}{flag}")
    L.hd_debug_limit_ops(e.ctx, which, -1)
    if which == 1:
        e.prepare(crl, cr_face=crf)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--latent", type=int, default=16)
    ap.add_argument("--t", type=float, default=500.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "op_parity.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    torch.set_grad_enabled(False)
    t0 = time.time()
    P = synth.refiner_state_dict(a.latent)
    print(f"weights {time.time() - t0:.1f}s", flush=True)
    model = FacialRefiner(a.latent)
    model.load_state_dict(P)
    t0 = time.time()
    model.to("cuda")
    torch.cuda.synchronize()
    print(f"upload+pack {time.time() - t0:.1f}s", flush=True)
    x, crl, crf = synth.sample_inputs(a.batch, a.latent)
    report = []
    taps = oracle_taps(P, x, crl, crf, a.t)
    floor = noise_floor(P, x, crl, crf, a.t, taps)
    w1 = scan(model, P, x, crl, crf, a.t, report, 1, taps, floor)
    print(f"prologue worst rel {w1:.3e}", flush=True)
    w0 = scan(model, P, x, crl, crf, a.t, report, 0, taps, floor)
    print(f"step worst rel {w0:.3e}", flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(report) + "\n")
    bad = [r for r in report if "<<<<<<" in r or "size" in r]
    print("\n".join(bad[:40]))
    print(f"{len(bad)} flagged of {len(report)} ops; report in {a.out}")


if __name__ == "__main__":
    main()
