#!/usr/bin/env python3
"""Latent 64 (FacialRefiner(64), 64 -> 512 px) against the oracle, measured on an MI355X; --out is the record kept in profiles/:
  a. eps of 3 faces against the bf16-emulating oracle (t in {999, 500, 0}, a timestep per face), face 0 alone against the batch;
  b. eps and the first 5 of 50 DDIM steps of one face against the reference goldens (oracle/make_golden.py --only l64);
  c. every launch of one eps evaluation on its own inputs (tools/op_forced.py), batch 1 and 3: worst rel-L2 per launch kind;
  d. the FPG / gate / idc_conv launches of the prologue on their own inputs (tools/prologue_forced.py), batch 1 and 3;
  e. the graph-replayed loop (first 5 rows of DDIM-50 and of DPM-Solver++ 2M-10, batch 2) against the eager loop and the oracle-network loop;
  and the dispatch tuples (hd_debug_op_info: loader / epilogue, mode, xcd_tile_affine, w_nt, ragged last row tile) of both programs at
  batch 1 and 3, marked `NEW` where no launch that the suite's latent-16 / latent-32 scans check has that tuple (denoiser: latent 16
  with one launch per GEMM at batch 2 / 64, latent 32 at batch 2 / 64; prologue: latent 16 at batch 3 / 8 / 32 / 33 / 64, latent 32 at
  batch 3 without the idc.* launches).
(Test infrastructure: uses oracle/.)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import op_forced                                               # noqa: E402
import prologue_forced as PF                                   # noqa: E402
from forced import op_names                                    # noqa: E402
from hifidiff_amd import _lib, sampling, schedulers, synth     # noqa: E402
from hifidiff_amd.refiner import FacialRefiner                 # noqa: E402
from oracle import hifidiff_oracle as O                        # noqa: E402
from parity_report import golden, psnr_pp, rel_l2              # noqa: E402

OUT = []


def say(s=""):
    print(s, flush=True)
    OUT.append(s)


def make_model(P, latent, no_xcd=False):
    if no_xcd:
        os.environ["HD_NO_XCD"] = "1"
    try:
        m = FacialRefiner(latent); m.load_state_dict(P); m.to("cuda:0")
    finally:
        os.environ.pop("HD_NO_XCD", None)
    return m


def program_tuples(engine, B, latent):
    """({launch name: tuple or None} of the denoiser program, the same of the prologue) at batch B: both are built by a prepare that runs
    no launch."""
    _, crl, crf = synth.sample_inputs(B, latent)
    pro = PF.program_tuples(engine, crl, crf)
    L, ctx, den = _lib.lib(), engine.ctx, {}
    for i, n in enumerate(op_names(ctx, 0)):
        v = L.hd_debug_op_info(ctx, 0, i)
        _lib.check(v, ctx)
        t = PF.unpack_info(v)
        if t is not None:
            tile = PF.TILE_ROWS.get(t[2] & 15)
            t = t + (int(tile is not None and op_forced.denoiser_gemm_rows(n, B, latent) % tile != 0),)
        den[n] = t
    return den, pro


def tuple_lines(title, tuples, seen):
    lines, groups = [title], {}
    for n, t in tuples.items():
        if t is not None:
            groups.setdefault(t, []).append(n)
    for t, names in sorted(groups.items()):
        lines.append(f"  {'NEW' if t not in seen else '   '} {PF.tuple_text(t):58s} {len(names):3d}  {names[0]}" + (f" .. {names[-1]}" if len(names) > 1 else ""))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="latent64.txt", help="report file; the full scan reports are written next to it")
    ap.add_argument("--only", default="a,b,c,d,e,tuples")
    a = ap.parse_args()
    what = set(a.only.split(","))
    a.out = os.path.abspath(a.out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    torch.set_grad_enabled(False)
    P16 = synth.refiner_state_dict(16)
    P = synth.refiner_state_dict(64, reuse=(P16, 16))
    m = make_model(P, 64)
    x, crl, crf = synth.sample_inputs(3, 64)
    xd, cld, cfd = x.cuda(), crl.cuda(), crf.cuda()
    say("latent 64 (FacialRefiner(64), 64 -> 512 px) on an MI355X: synthetic weights (the latent-16 ones + idc_conv 2048 -> 32768), synthetic inputs")
    if "a" in what:
        t0 = time.time()
        cond = O.Conditioning(P, crl, crf, prec=O.BF16)
        say(f"\n== a. eps, batch 3, against the bf16-emulating oracle (bounds 6e-3, worst face 8e-3); oracle conditioning {time.time() - t0:.0f} s")
        for name, t in [(str(t), t) for t in (999, 500, 0)] + [("(980, 37, 500) per face", torch.tensor([980.0, 37.0, 500.0]))]:
            ref = O.fused_denoiser(P, x, t, cond=cond, prec=O.BF16)
            td = t.cuda() if torch.is_tensor(t) else t
            e = m(xd, td, cfd, cld).sample.cpu()
            same = torch.equal(m(xd, td, cfd, cld).sample.cpu(), e)
            say(f"t = {name}: rel-L2 {rel_l2(e, ref):.3e}, worst face {max(rel_l2(e[f], ref[f]) for f in range(3)):.3e}, repeated evaluation bit-identical: {same}")
            if name == "500":
                e500 = e
        e1 = m(xd[:1], 500, cfd[:1], cld[:1]).sample.cpu()
        say(f"face 0 alone against face 0 of the batch (t = 500, bound 6e-3): rel-L2 {rel_l2(e1, e500[:1]):.3e}, bit-identical: {torch.equal(e1, e500[:1])}")
    if "b" in what:
        say("\n== b. one face against the reference goldens (bounds: eps 1e-2; DDIM 3e-2 and 40 dB)")
        e = m(xd[:1], torch.full((1,), 500), cfd[:1], cld[:1]).sample.cpu()
        say(f"eps t = 500: rel-L2 {rel_l2(e, golden('refiner_eps_L64.npz')['eps_t500']):.3e}")
        sch = schedulers.DDIMScheduler(clip_sample_range=3.0); sch.set_timesteps(50); sch.timesteps = sch.timesteps[:5]
        lat = sampling.sample(m, xd[:1], cfd[:1], cld[:1], sch).cpu()
        g5 = golden("ddim50_first5_L64.npz")["final"]
        ps, rng = psnr_pp(lat, g5)
        say(f"first 5 of 50 DDIM steps (eta 0, clip 3.0), graph-replayed: rel-L2 {rel_l2(lat, g5):.3e}, PSNR {ps:.1f} dB on peak-to-peak {rng:.2f}")
    if "c" in what:
        say("\n== c. every launch of one eps evaluation on its own inputs (tools/op_forced.py; bounds fp32 3e-4, bf16-stored 3e-3), t = 500")
        for B in (1, 3):
            rep, info = [], {}
            t0 = time.time()
            w = op_forced.forced_scan(m, P, x[:B], crl[:B], crf[:B], 500.0, rep, info=info)
            bad = [r for r in rep if "<<<<<<" in r or "no rule" in r]
            say(f"batch {B}: {info['launches']} launches, {len(rep)} lines, {len(bad)} flagged; worst fp32 {w['fp32']:.3e}, worst bf16-stored {w['bf16']:.3e} ({time.time() - t0:.0f} s)")
            say("  worst per launch kind: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(info["kinds"].items())))
            for r in bad:
                say("  " + r)
            with open(os.path.join(os.path.dirname(a.out), f"latent64_op_forced_B{B}.txt"), "w") as f:
                f.write("\n".join(rep) + "\n")
    if "d" in what:
        say("\n== d. the prologue without the idc.* ResNet launches, on their own inputs (tools/prologue_forced.py; the same bounds)")
        for B in (1, 3):
            rep, info = [], {}
            w = PF.prologue_scan(m, P, crl[:B], crf[:B], rep, lambda n, t: not n.startswith("idc.") or n == "idc_conv", info)
            bad = [r for r in rep if "<<<<<<" in r or "no rule" in r]
            for ln in PF.summary(B, 64, w, info)[:-1 - len(PF.tuple_table(info["tuples"]))]:
                say(ln)
            say(f"{len(bad)} flagged of {len(rep)} lines")
            for r in bad:
                say("  " + r)
            with open(os.path.join(os.path.dirname(a.out), f"latent64_prologue_B{B}.txt"), "w") as f:
                f.write("\n".join(rep) + "\n")
    if "e" in what:
        say("\n== e. the graph-replayed loop, batch 2, first 5 rows (bounds: eager loop 50 dB on a range of 6, oracle-network loop rel-L2 2e-2)")
        cond2 = O.Conditioning(P, crl[:2], crf[:2], prec=O.BF16)
        for kind, n in (("ddim", 50), ("dpm", 10)):
            s = schedulers.DDIMScheduler(clip_sample_range=3.0) if kind == "ddim" else schedulers.DPMSolverMultistepScheduler()
            s.set_timesteps(n)
            ts, coef = s.coefficient_table()

            class Table:
                def coefficient_table(self):
                    return ts[:5].contiguous(), coef[:5].contiguous()
            graph = sampling.sample(m, xd[:2], cfd[:2], cld[:2], Table()).cpu()
            again = sampling.sample(m, xd[:2], cfd[:2], cld[:2], Table()).cpu()
            xe = xd[:2]
            for t in s.timesteps[:5]:
                xe = s.step(m(xe, int(t), cfd[:2], cld[:2]).sample, t, xe).prev_sample
            mse = float(((xe.cpu().double() - graph.double()) ** 2).mean())
            xr, h = x[:2].double(), None
            for i, t in enumerate(ts[:5].tolist()):
                eps = O.fused_denoiser(P, xr.float(), torch.full((2,), int(t)), prec=O.BF16, cond=cond2).double()
                c = [float(v) for v in coef[i]] + [0.0] * (8 - coef.shape[1])
                x0 = (xr - c[0] * eps) / c[1]
                x0 = x0.clamp(-c[2], c[2]) if np.isfinite(c[2]) else x0
                xr, h = c[3] * x0 + c[4] * xr + c[5] * eps + (c[7] * h if c[7] != 0.0 else 0.0), x0
            say(f"{kind}-{n}: eager loop {10.0 * np.log10(36.0 / max(mse, 1e-30)):.1f} dB, oracle-network loop rel-L2 {rel_l2(graph, xr):.3e}, repeated loop bit-identical: {torch.equal(graph, again)}")
    if "tuples" in what:
        say("\n== dispatch tuples of the two programs at latent 64 (count, first .. last launch); NEW: in no latent-16 / latent-32 scan of the suite")
        t64 = {B: program_tuples(m.engine, B, 64) for B in (1, 3)}
        del m
        seen = set()
        m16 = make_model(P16, 16, no_xcd=True)
        for B in (2, 3, 8, 32, 33, 64):
            den, pro = program_tuples(m16.engine, B, 16)
            seen |= set(den.values()) if B in (2, 64) else set(pro.values())
            if B == 64:
                seen |= set(pro.values())
        del m16
        m32 = make_model(synth.refiner_state_dict(32, reuse=(P16, 16)), 32)
        for B in (2, 3, 64):
            den, pro = program_tuples(m32.engine, B, 32)
            seen |= set(den.values()) if B != 3 else {t for n, t in pro.items() if not n.startswith("idc.") or n == "idc_conv"}
        del m32
        seen.discard(None)
        for B in (1, 3):
            for lines in (tuple_lines(f"denoiser program, batch {B}:", t64[B][0], seen),
                          tuple_lines(f"prologue without idc.*, batch {B}:", {n: t for n, t in t64[B][1].items() if not n.startswith("idc.") or n == "idc_conv"}, seen)):
                for ln in lines:
                    say(ln)
    with open(a.out, "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
