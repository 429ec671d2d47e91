#!/usr/bin/env python3
"""Teacher-forced scan of the hd_lpips program: every launch against its rule ON THE LAUNCH'S OWN INPUTS (the pattern of
tools/vae_forced.py, built on tools/forced.py: `Check`, `PrefixRun`, `conv`, `q`).

Every launch of this program writes a buffer of its own (the prepared input, five feature maps, two pooled maps, the partial sums, the
scores), so one run of the whole program holds every launch's inputs and outputs; they are read back with `hd_debug_read_op`.  Rules:
  input            its three live channels within one bf16 rounding of the contract's steps 2 - 4 in fp32 (unresampled, unnormalised inputs);
                   the five padding channels bit-exact zero
  slice{k}.conv    relu(conv) of the read-back input with bf16 operands (`forced.conv`), rounded to bf16, at BF16_BOUND, per face too
  slice{k}.pool    F.max_pool2d(3, 2) of the read-back map, bit-exact
  distance         the partial sums of a (face, layer) added up and divided by the position count, against float64 on the read-back
                   features: max-abs error <= F64_MARGIN x that of torch's fp32 evaluation of the same formula, rel-L2 <= FP32_BOUND
  combine          layers_out and out: the bits of the partial sums added in index order (float64, sequential), divided, and summed
A launch without a rule is reported as `no rule`; a line over its bound carries `<<<<<<`.  (Test infrastructure: uses oracle/ through
tools/forced.py.)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from forced import Check, PrefixRun, conv, q      # noqa: E402
from hifidiff_amd import arch, metrics            # noqa: E402

POS_PER_WG = 64                                    # hd_lpips.hpp: LP_POS_PER_WG
CONV_OF = {"slice%d.conv" % (k + 1): k for k in range(5)}


def _f64_words(flat):
    """An fp64 output as hd_debug_read_op returns it (two 32-bit words per value) -> float64."""
    return torch.from_numpy(flat.numpy().view(np.float64).copy())


def _map(flat, N, C):
    """A channels-last read-back [N, s, s, C] -> NCHW."""
    s = int(round((flat.numel() // (N * C)) ** 0.5))
    assert N * s * s * C == flat.numel(), (flat.numel(), N, C)
    return flat.reshape(N, s, s, C).permute(0, 3, 1, 2).contiguous()


def _one_rounding(ck, i, name, got, want32):
    """|got - x| <= 2^-8 |x| for the fp32 formula's x: half a bf16 step (2^-9 |x| at most for round to nearest even), doubled for an x
    that another fp32 evaluation puts on the other side of a tie."""
    err = (got.double() - want32.double()).abs()
    lim = want32.double().abs() * 2.0 ** -8 + 1e-38
    bad = int((err > lim).sum())
    ck.worst["input"] = max(ck.worst.get("input", 0), bad)
    ck._line(i, name, "rgb", f"{bad} of {got.numel()} values further than one bf16 rounding from the fp32 formula (worst {float((err / lim).max()):.3f} of the bound)", bad == 0)


def scan(model, state, images, ref, report, normalize=True):
    """Every launch of hd_lpips(images, ref) with unresampled, unnormalised inputs.  Returns Check.worst (launch kind -> worst figure;
    "launches": their number; "no_rule": launches without a rule)."""
    assert images.shape == ref.shape
    B, R = int(images.shape[0]), int(images.shape[2])
    N = 2 * B
    a, b = images.cuda(), ref.cuda()
    held = {}

    def run():
        held["out"], held["layers"] = model(a, b, normalize=normalize, per_layer=True)

    pre = PrefixRun(model._ctx, run)
    try:
        pre.run_to(1)
        names = pre.names()
        pre.run_to(len(names))
        outs = [pre.op(i) for i in range(len(names))]
    finally:
        pre.reset()
    ck = Check(report, batch=N, name_width=16)
    sides = arch.lpips_sides(R)
    P = [s * s for s in (sides[0], sides[1], sides[2], sides[2], sides[2])]
    C = [c[1] for c in arch.LPIPS_CONVS]
    wg = [(p + POS_PER_WG - 1) // POS_PER_WG for p in P]
    wg0 = np.concatenate([[0], np.cumsum(wg)])
    feats, no_rule, partial = {}, 0, None
    for i, name in enumerate(names):
        if name == "input":
            got = outs[i].reshape(N, R, R, 8)
            x = torch.cat([metrics.lpips_prepare(state, images, None, normalize), metrics.lpips_prepare(state, ref, None, normalize)])      # fp32
            _one_rounding(ck, i, name, got[..., :3].permute(0, 3, 1, 2), x)
            ck.exact(i, name, "input.pad", "pad", got[..., 3:].contiguous(), torch.zeros(N, R, R, 5))
        elif name in CONV_OF:
            k = CONV_OF[name]
            cname, cout, cin, _, stride, pad = arch.LPIPS_CONVS[k]
            src = outs[i - 1]
            x = src.reshape(N, R, R, 8)[..., :3].permute(0, 3, 1, 2).contiguous() if k == 0 else _map(src, N, cin)
            w, bias = state[cname + ".weight"], state[cname + ".bias"]
            want = q(torch.relu(conv(x, w, bias, stride=stride, padding=pad)))
            feats[k] = _map(outs[i], N, cout)
            ck.rel(i, name, "conv", f"f{k + 1}", feats[k], want, True,
                   lambda: q(torch.relu(conv(x, w, bias, stride=stride, padding=pad, halves=True))))
        elif name.endswith(".pool"):
            k = int(name[len("slice")]) - 2                                  # slice2.pool pools f1
            ck.exact(i, name, "pool", f"pool(f{k + 1})", _map(outs[i], N, C[k]), F.max_pool2d(feats[k], 3, 2))
        elif name == "distance":
            partial = _f64_words(outs[i]).reshape(B, int(wg0[-1]))
            got = torch.stack([partial[:, wg0[k]:wg0[k + 1]].sum(dim=1) / P[k] for k in range(5)], dim=1)
            fl = [feats[k] for k in range(5)]
            d64 = metrics.lpips_distance(state, [f[:B].double() for f in fl], [f[B:].double() for f in fl])
            d32 = metrics.lpips_distance(state, [f[:B] for f in fl], [f[B:] for f in fl])
            ck.B = B                                                         # one row of five per face here
            ck.against64(i, name, "distance", "d_k", got, d64, d32)
            ck.B = N
        elif name == "combine":
            lay = np.zeros((B, 5))
            for f in range(B):
                for k in range(5):
                    s = np.float64(0.0)
                    for v in partial[f, wg0[k]:wg0[k + 1]].numpy():
                        s = s + v
                    lay[f, k] = s / np.float64(P[k])
            tot = np.zeros(B)
            for k in range(5):
                tot = tot + lay[:, k]
            as32 = lambda t: t.contiguous().view(torch.int32)                # noqa: E731  (Check.exact compares 32-bit words)
            ck.exact(i, name, "combine", "layers_out", as32(held["layers"].cpu()), as32(torch.from_numpy(lay)))
            ck.exact(i, name, "combine", "out", as32(held["out"].cpu()), as32(torch.from_numpy(tot)))
            ck.exact(i, name, "combine", "read-back", as32(_f64_words(outs[i])), as32(held["out"].cpu()))
        else:
            ck.no_rule(i, name)
            no_rule += 1
    ck.worst["launches"], ck.worst["no_rule"] = len(names), no_rule
    ck.worst["f64"] = dict(ck.f64)
    ck.worst["face"] = dict(ck.face)
    return ck.worst


def main():
    import argparse
    import lpips_cases as lc
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--amp", type=float, default=0.05)
    ap.add_argument("--out", default="lpips_forced.txt", help="report file")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    img, ref = lc.family(a.amp, a.batch, a.res, a.res, tag="forced")
    report = [f"== hd_lpips, {a.res} px, batch {a.batch}, perturbation {a.amp}"]
    worst = scan(lc.model(), lc.state(), img, ref, report)
    with open(a.out, "w") as f:
        f.write("\n".join(report) + f"\nworst per launch kind: {worst}\n")
    bad = [ln for ln in report if "<<<<<<" in ln or "no rule" in ln]
    print("\n".join(bad[:40]))
    print(f"{worst}\n{len(bad)} flagged of {len(report)} lines; report in {a.out}")


if __name__ == "__main__":
    main()
