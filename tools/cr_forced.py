#!/usr/bin/env python3
"""Teacher-forced parity of CoarseRestoration: every launch of hd_cr_forward against the CPU oracle ON THE LAUNCH'S OWN INPUTS
(for the program built in hd_aux.hip from the kernels of hd_cr.hpp and the refiner path).

The level buffers are reused by every stage, so the state is taken by prefix runs; checks, bounds, the prefix runs and the rules of
the NAF blocks and of the down / up convs: tools/forced.py.  Here: what CoarseRestoration has of its own --
  * the STN launches (the two localisation convs, theta, the grid sample), intro and outro: no bf16 operand, held against float64;
  * skip copy / add: bit-exact, the sum's 1 x C LayerNorm partials and bf16 copy next to it;
  * the weight sets (`per-face`, `offset`) with the conditions they are there to create, and `skip_add_prefix`.
`max |row mean| / row std` is printed per statistics buffer.  (Test infrastructure: uses oracle/.)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from forced import (BF16_BOUND, F64_MARGIN, FP32_BOUND, STAT_BOUND, Check, LaunchIO, NafRules, PrefixRun, down_rule, intro_rule,      # noqa: E402,F401
                    nchw, q, read_buffer, rows, up_rule)
from hifidiff_amd import arch                                  # noqa: E402
from oracle import hifidiff_oracle as O                         # noqa: E402

PR = O.BF16
CR_OPS = 175                                                    # 2 + encoders 20 + 20 + 14 + 22, middle 44, decoders 16 + 9 + 9 + 19
KINDS = {"intro", "conv1", "conv2_gate_pool.unfused", "conv2_gate_pool.strips", "conv2_gate_pool.fused", "pool_finish", "sca.f32", "sca.bf16",
         "conv3", "conv4", "conv5", "conv5.chain", "localization.0", "localization.3", "theta", "grid_sample", "down", "skip_copy",
         "skip_add", "up", "outro", "stats", "bf16_copy"}
F64_KINDS = ("intro", "outro", "localization.0", "localization.3", "theta", "grid_sample", "pool_finish")
EXACT_KINDS = ("skip_copy", "skip_add", "bf16_copy")

# ---- the `per-face` weight set and its inputs (tests/test_cr_ops.py verifies both conditions on the thetas read back) ----
# synth.cr_state_dict(wild=True) with `*.stn.fc_loc.2.weight` scaled, so that the three faces of a batch get different thetas
# (>= 0.25 in some entry between any two faces at every STN: one pixel at side 8) while at least four STNs still sample
# 10 % .. 60 % of their output from outside the map.  One factor for all nine STNs cannot do that: the hidden layer's
# face-dependent part is 20 - 100 x smaller than its common part and 60 x smaller at the 8 x 8 levels than at level 0 (on the
# CPU oracle, factors 1 .. 8000: the middle STN's thetas differ by 0.003 at the factor where encoders.0 already samples 99 %
# outside, and beyond that every map is zero and the faces are equal again).  Hence one factor per STN, found upstream first on
# the CPU oracle for a pair difference of 0.32 (0.30 .. 0.33 reached, bf16 emulation), and faces of different amplitude.
PER_FACE_FACTORS = {"encoders.0": 8.8, "encoders.1": 13.0, "encoders.2": 30.0, "encoders.3": 34.0, "middle_blocks": 1100.0,
                    "decoders.0": 84.0, "decoders.1": 1000.0, "decoders.2": 130.0, "decoders.3": 22.0}
PER_FACE_AMPLITUDE = (1.0, 30.0, -30.0)
THETA_MIN_DIFF, OUTSIDE_RANGE, OUTSIDE_MIN_STNS = 0.25, (0.10, 0.60), 4
# ---- the `offset` weight set: plain weights, encoders.3.sampling.bias + BIAS_OFFSET: the level-4 skip and with it the decoder
# input x = middle + skip sit far from zero: max |row mean| / row std 39 on the CPU oracle (19.4 at 2.0, 77.6 at 8.0; wanted >= 30)
BIAS_OFFSET = 4.0
RATIO_MIN = 30.0


def per_face_state_dict(P_wild):
    S = dict(P_wild)
    for stage, f in PER_FACE_FACTORS.items():
        S[f"{stage}.stn.fc_loc.2.weight"] = P_wild[f"{stage}.stn.fc_loc.2.weight"] * f
    return S


def offset_state_dict(P):
    S = dict(P)
    S["encoders.3.sampling.bias"] = P["encoders.3.sampling.bias"] + BIAS_OFFSET
    return S


def faces(B, per_face=False):
    from hifidiff_amd import synth
    amp = PER_FACE_AMPLITUDE if per_face else (1.0,) * B
    return torch.from_numpy(np.stack([synth.rand(f"ln_face/{f}", (3, 128, 128)) * np.float32(amp[f % 3]) for f in range(B)]))


def theta_conditions(thetas):
    """thetas: {stn name: ([B, 6], side)} as read back.  Returns (smallest over STNs of the smallest pair difference (max over the six
    entries), number of STNs whose output samples 10 % .. 60 % from outside the map, the per-STN figures)."""
    per = {}
    for name, (th, side) in thetas.items():
        B = th.shape[0]
        d = min((float((th[a] - th[b]).abs().max()) for a in range(B) for b in range(a + 1, B)), default=float("inf"))
        g = F.affine_grid(th.double().reshape(B, 2, 3), [B, 1, side, side], align_corners=False)
        per[name] = (d, float((g.abs() > 1.0).any(-1).double().mean()))
    n_in = sum(OUTSIDE_RANGE[0] <= o <= OUTSIDE_RANGE[1] for _, o in per.values())
    return min(d for d, _ in per.values()), n_in, per


# ---------------------------------------------------------------------------------------------- what a launch writes
def _stage_table():
    return {name: (c, r, (c // 32).bit_length() - 1, samp) for name, c, r, n, samp in arch.cr_stages()}


def _parse(name, stages):
    """-> (stage name or None, level, block prefix or None, leaf)"""
    if name in ("intro", "outro"):
        return None, 0, None, name
    if name == "middle_blocks":                                  # the middle stage's last launch carries the stage's name
        return name, 4, None, "stn"
    st = next(s for s in sorted(stages, key=len, reverse=True) if name == s or name.startswith(s + "."))
    l = stages[st][2]
    rest = name[len(st) + 1:]
    if rest.startswith("nfbs."):
        j, leaf = rest.split(".")[1:3]
        return st, l, f"{st}.nfbs.{j}", leaf
    return st, l, None, {"": "sampling", "stn": "stn", "stn.theta": "theta"}.get(rest, rest.replace("stn.", ""))


# ---------------------------------------------------------------------------------------------- the rules
class _Scan:
    def __init__(self, model, P, x, ck, info):
        self.P, self.B, self.x, self.ck, self.info = P, x.shape[0], x, ck, info
        xd = x.cuda()
        self.run = PrefixRun(model._ctx, lambda: model(xd))
        self.run.run_to(1)                                      # builds the program for this batch
        self.names = self.run.names()
        self.stages = _stage_table()
        self.naf = NafRules(P, ck, extras=True, own_t1=True)

    def rule(self, i):
        P, B, ck, name, io = self.P, self.B, self.ck, self.names[i], LaunchIO(self.run, i)
        stage, l, p, leaf = _parse(name, self.stages)
        C, H = 32 << l, 128 >> l
        s = str(l)
        if p is not None:
            self.naf.launch(i, self.names, p, l, B, C, H, None, io)
        elif leaf == "intro":
            out = io.out()
            intro_rule(ck, i, name, "intro", "X0", out, self.x, P["intro.weight"], P["intro.bias"])
            ck.copy_and_stats(i, name, io.after, 0, "x", out, 32, 1, 32)
        elif leaf == "outro":
            intro_rule(ck, i, name, "outro", "image", io.out(), nchw(io.before("X0"), B, 32, 128), P["outro.weight"], P["outro.bias"], lambda t: t.reshape(-1))
        elif leaf in ("localization.0", "localization.3"):
            w, b = P[f"{stage}.stn.{leaf}.weight"], P[f"{stage}.stn.{leaf}.bias"]
            if leaf == "localization.0":
                src = nchw(io.before("X" + s), B, C, H)
            else:
                h1 = (H - P[f"{stage}.stn.localization.0.weight"].shape[-1] + 1) // 2
                src = io.before("loc1")[:B * 8 * h1 * h1].reshape(B, 8, h1, h1)
            f = lambda t, w, b: torch.relu(F.max_pool2d(F.conv2d(t, w, b), 2, stride=2))     # noqa: E731
            ck.against64(i, name, leaf, "loc", io.out(), f(src.double(), w.double(), b.double()), f(src, w, b))
        elif leaf == "theta":
            fc = f"{stage}.stn.fc_loc"
            xs = io.before("loc2")[:P[fc + ".0.weight"].shape[1] * B].reshape(B, -1)
            f = lambda t, c: F.linear(torch.relu(F.linear(t, c(P[fc + ".0.weight"]), c(P[fc + ".0.bias"]))), c(P[fc + ".2.weight"]), c(P[fc + ".2.bias"]))     # noqa: E731
            out = io.out()
            ck.against64(i, name, "theta", "theta", out, f(xs.double(), lambda t: t.double()), f(xs, lambda t: t))
            self.info.setdefault("theta", {})[f"{stage}.stn"] = (out.reshape(B, 6).clone(), H)
        elif leaf == "stn":
            X, th = nchw(io.before("X" + s), B, C, H), io.before("theta").reshape(B, 2, 3)
            f = lambda t, x: F.grid_sample(x, F.affine_grid(t, list(x.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)     # noqa: E731
            out = io.out()
            ck.against64(i, name, "grid_sample", "Y", out, rows(f(th.double(), X.double())), rows(f(th, X)))
            ck.exact(i, name, "bf16_copy", "Yb" + s, io.after("Yb" + s)[:out.numel()], q(out))
        elif leaf == "sampling" and self.stages[stage][3] == "down":
            src, out = nchw(io.before("Yb" + s), B, C, H), io.out()
            down_rule(ck, i, name, f"X{l + 1}", out, src, P[stage + ".sampling.weight"], P[stage + ".sampling.bias"])
            ck.copy_and_stats(i, name, io.after, l + 1, "x", out, 2 * C, 2 * C // 32, 32)
        elif leaf == "skip_copy":
            ck.exact(i, name, "skip_copy", f"skip{l + 1}", io.out(), io.before(f"X{l + 1}"))
        elif leaf == "skip_add":
            want, out = io.before("Y" + s) + io.before("skip" + s), io.out()
            ck.exact(i, name, "skip_add", "X" + s, out, want)
            ck.copy_and_stats(i, name, io.after, l, "x", out, C, 1, C)
        elif leaf == "sampling" and self.stages[stage][3] == "up":
            d, C2, H2 = l - 1, C // 2, 2 * H
            src = nchw(io.before("Yb" + s), B, C, H)
            skip = nchw(io.before(f"skip{d}"), B, C2, H2) if d >= 1 else None
            out = io.out()
            up_rule(ck, i, name, f"X{d}", out, src, P[stage + ".sampling.0.weight"], skip, contribution="X-skip")
            ck.copy_and_stats(i, name, io.after, d, "x", out, C2, C2 // 32, 32)
        else:
            ck.no_rule(i, name)


def cr_scan(model, P, x, report, info=None):
    """Every launch of hd_cr_forward(x [B,3,128,128]).  Returns {launch kind: worst rel-L2 (exact kinds: differing elements)} plus "launches";
    info (a dict) receives "theta" {stn: ([B, 6], side)} as read back, "ratio" {statistics buffer: max |row mean| / row std} and "f64"
    {fp32-only kind: (kernel max-abs, torch fp32 max-abs)}."""
    info = info if info is not None else {}
    ck = Check(report)
    sc = _Scan(model, P, x, ck, info)
    try:
        for i in range(len(sc.names)):
            sc.rule(i)
    finally:
        sc.run.reset()
    ck.worst["launches"] = len(sc.names)
    info["ratio"], info["f64"] = ck.ratio, ck.f64
    return ck.worst


def skip_add_prefix(model, P, x, report):
    """One prefix run up to the launch behind `decoders.0.skip_add` (the first decoder block's fused conv1 -> depthwise -> gate, which reads
    the 1 x 512 partials): the sum, its partials and bf16 copy, and that next launch's G.  Returns (mean error / row std, rstd relative
    error, max |row mean| / row std of the sum, rel-L2 of the next launch's G)."""
    B = x.shape[0]
    ck = Check(report)
    sc = _Scan(model, P, x, ck, {})
    names, run = sc.names, sc.run
    k = names.index("decoders.0.skip_add")
    assert names[k + 1] == "decoders.0.nfbs.0.conv2_gate_pool", names[k + 1]
    try:
        run.run_to(k + 2)                                       # the next launch writes G4 / pooled4 only: X4, sx4, Xb4, Y4, skip4 are as skip_add left them
        X4, G = run.op(k), run.op(k + 1)
        rd = {b: run.buf(b) for b in ("Y4", "skip4", "sx4", "Xb4")}
    finally:
        run.reset()
    ck.exact(k, names[k], "skip_add", "X4", X4, rd["Y4"] + rd["skip4"])
    ck.exact(k, names[k], "bf16_copy", "Xb4", rd["Xb4"], q(X4))
    mean_err, rstd_err, ratio = ck.stats(k, names[k], "sx4", rd["sx4"], X4.reshape(B * 64, 512), 1, 512)
    g = sc.naf.gate_of_x("decoders.0.nfbs.0", nchw(X4, B, 512, 8))
    ck.rel(k + 1, names[k + 1], "conv2_gate_pool.fused", "G", G, rows(PR.q(g)), True)
    return mean_err, rstd_err, ratio, ck.worst["conv2_gate_pool.fused"]


def main():
    import argparse
    from hifidiff_amd import synth
    from hifidiff_amd.cr import CoarseRestoration
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--weights", choices=("plain", "per-face", "offset"), default="plain")
    ap.add_argument("--out", default="cr_forced.txt", help="report file")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    P = {"plain": synth.cr_state_dict, "per-face": lambda: per_face_state_dict(synth.cr_state_dict(wild=True)),
         "offset": lambda: offset_state_dict(synth.cr_state_dict())}[a.weights]()
    m = CoarseRestoration(); m.load_state_dict(P); m.to("cuda:0")
    report, info = [f"== CoarseRestoration, batch {a.batch}, {a.weights} weights"], {}
    worst = cr_scan(m, P, faces(a.batch, a.weights == "per-face"), report, info)
    cond = theta_conditions(info["theta"])
    with open(a.out, "w") as f:
        f.write("\n".join(report) + "\n")
        f.write(f"worst per launch kind: {worst}\nfp32-only kinds (kernel, torch fp32) max-abs: {info['f64']}\n")
        f.write(f"thetas: smallest pair difference {cond[0]:.3f}, STNs sampling 10-60 % outside {cond[1]}, per STN (difference, outside) {cond[2]}\n")
    bad = [ln for ln in report if "<<<<<<" in ln or "no rule" in ln]
    print("\n".join(bad[:40]))
    print(f"{worst}\n{len(bad)} flagged of {len(report)} lines; report in {a.out}")


if __name__ == "__main__":
    main()
