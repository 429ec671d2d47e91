#!/usr/bin/env python3
"""Teacher-forced parity of the VAE boundary: every launch of hd_vae_encode / hd_vae_decode against the CPU oracle ON THE
LAUNCH'S OWN INPUTS (the pattern of tools/op_forced.py, for the programs built in hd_aux.hip from the kernels of hd_vae.hpp).

The workspace buffers (X, T, S, H, H2, Xb, U, Q, K, V, mom) are reused and conv2 writes X while reading it as the residual, so
the state is taken by prefix runs: for n = 1 .. N the program runs with `hd_debug_limit_ops(ctx, 0, n)` (one limit for both
programs) and the output of launch n - 1 is read back (`hd_debug_read_op`, which = 0 encode / 1 decode) and kept on the host.
Every launch's inputs are then earlier launches' outputs, and the oracle's arithmetic for that one launch (bf16-operand
emulation at the points the kernels round) is applied to exactly those values.  Helpers, the `Check` class and its bounds (3e-4 for
fp32 outputs, 3e-3 for bf16-stored outputs, compared with the reference rounded to bf16) and the prefix runs: tools/forced.py; the
rules here are the VAE's own (nothing in it is a NAF block).  Pure data movement (`encoder.input`, the `nearest`
upsamplers, `decoder.output`) must be bit-exact.  What is not a GEMM (GroupNorm, softmax(QK^T/sqrt(C)) V, quant_conv + posterior
sample, post_quant_conv) is held against float64.  Report lines carry `<<<<<<` where a bound is exceeded; a launch without a
rule is reported as `no rule`.  (Test infrastructure: uses oracle/.)
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from forced import BF16_BOUND, FP32_BOUND, Check, PrefixRun, nchw, q as _q64, read_op, rows      # noqa: E402
from oracle import hifidiff_oracle as O                         # noqa: E402

PR = O.BF16
ENC_OPS, DEC_OPS = 56, 75                                       # launches of the two programs without the bicubic resize (57 with it)

# ---- the `stress` weight set: synth.vae_state_dict() with the changes below (tests/test_vae_ops.py verifies, from the values
# read back, that each change creates the condition it is there for) ----
Q_FACTOR = {"encoder": 256.0, "decoder": 64.0}                  # to_q.weight: sharp softmax, logits past exp's fp32 range (88).  64 leaves the encoder's
                                                                # median max-probability at 0.10 for T = 1024 once conv_in is offset; 256 gives about 0.6
GN_SHIFT = {"encoder": 20.0, "decoder": 64.0}                   # conv_in.bias: |group mean| / group std >= 30 at the first norm1 (group std of conv_in's
                                                                # output is at most 0.47 / 1.5 on the synthetic inputs)
LOGVAR_SCALE = 256.0                                            # quant_conv.weight[4:8]: logvar reaches both ends of clamp(-30, 20)


def stress_state_dict(P):
    S = dict(P)
    for side in ("encoder", "decoder"):
        S[f"{side}.mid_block.attentions.0.to_q.weight"] = P[f"{side}.mid_block.attentions.0.to_q.weight"] * Q_FACTOR[side]
        S[f"{side}.conv_in.bias"] = P[f"{side}.conv_in.bias"] + GN_SHIFT[side]
    w = P["quant_conv.weight"].clone()
    w[4:8] *= LOGVAR_SCALE
    S["quant_conv.weight"] = w
    return S


# ---------------------------------------------------------------------------------------------- helpers
def _side(flat, B, C):
    return math.isqrt(flat.numel() // (B * C))


def group_ratio(x):
    """min over (face, group) of |group mean| / group std of an NCHW map: how far from centred GroupNorm's input is."""
    g = x.double().reshape(x.shape[0], 32, -1)
    return float((g.mean(-1).abs() / g.std(-1, unbiased=False)).min())


def attention_stats(q, k):
    """What the softmax of one attention input looks like (q, k: [B, T, 512] as the kernel read them)."""
    lg = q.double() @ k.double().transpose(1, 2) / math.sqrt(q.shape[-1])
    mp, am = torch.softmax(lg, -1).max(-1)
    return {"T": q.shape[1], "median_maxp": float(mp.median()), "min_maxp": float(mp.min()), "logit_absmax": float(lg.abs().max()),
            "argmax_past_tile0": float((am >= 64).double().mean())}


def _check(report, fp32_bound=FP32_BOUND, bf16_bound=BF16_BOUND):
    return Check(report, None, fp32_bound, bf16_bound, 52, 8)


def _prefix_outputs(pre):
    """(names, outs) of pre's program: outs[i] = output of launch i after a run of launches 0 .. i only."""
    try:
        pre.run_to(1)                                           # builds the program for the run's arguments
        names = pre.names()
        outs = [pre.op(0)]
        for n in range(2, len(names) + 1):
            pre.run_to(n)
            outs.append(pre.op(n - 1))
    finally:
        pre.reset()
    return names, outs


def _groupnorm64(x, w, b, silu):
    y = F.group_norm(x.double(), 32, w.double(), b.double(), eps=1e-6)
    return F.silu(y) if silu else y


def bicubic_errors(got, x, R):
    """(max-abs error of `got`, max-abs error of torch's fp32 CPU bicubic), both against torch's float64 bicubic of the same input."""
    ref = F.interpolate(x.double(), size=(R, R), mode="bicubic", align_corners=False)
    f32 = F.interpolate(x, size=(R, R), mode="bicubic", align_corners=False)
    return float((got.reshape(ref.shape).double() - ref).abs().max()), float((f32.double() - ref).abs().max())


def _scan(P, names, outs, B, feed, ck, info, first=0, X=None):
    """The rules.  feed: what the program's first launch read ("images", "vae_range", "noise" for encode; "latents" for decode).
    X: the fp32 residual stream (NCHW) as the HIP path holds it before launch i."""
    S = None                                                    # conv_shortcut's output of the resnet in flight
    for i, name in enumerate(names):
        if i < first:
            continue
        out = outs[i]
        leaf = name.split(".")[-1]
        wk, bk = name + ".weight", name + ".bias"
        if name == "bicubic":
            R = math.isqrt(out.numel() // (B * 3))
            err, err32 = bicubic_errors(out, feed["images"], R)
            info.setdefault("bicubic", []).append((err, err32))
            ck.worst["bicubic"] = max(ck.worst.get("bicubic", 0.0), err)
            ck.report.append(f"{i:3d} {name:52s} resized  maxabs {err:.3e} (torch fp32 {err32:.3e}; <= 4 x that){'' if err <= 4 * err32 else '  <<<<<<'}")
        elif name == "encoder.input":
            src = feed["images"] if i == 0 else outs[i - 1].reshape(B, 3, -1)
            src = src.reshape(B, 3, -1)
            if feed.get("vae_range"):
                src = src.clamp(0, 1) * 2.0 - 1.0
            want = torch.zeros(B, src.shape[2], 8)
            want[:, :, :3] = PR.q(src).permute(0, 2, 1)
            ck.exact(i, name, "encoder.input", "in8", out, want.reshape(-1))
        elif name == "post_quant_conv":
            z = feed["latents"].double() / 0.18215
            y = F.conv2d(z, P[wk].double(), P[bk].double())
            want = torch.zeros(B, y.shape[2] * y.shape[3], 8, dtype=torch.float64)
            want[:, :, :4] = y.reshape(B, 4, -1).permute(0, 2, 1)
            got = out.reshape(B, -1, 8)
            ck.rel(i, name, "post_quant_conv", "in8", got[:, :, :4], _q64(want[:, :, :4]), True)
            ck.exact(i, name, "post_quant_conv.pad", "pad", got[:, :, 4:].contiguous(), torch.zeros_like(got[:, :, 4:]))
        elif leaf == "conv_in":                                 # cin 3 / 4 zero padded to 8
            cin = P[wk].shape[1]
            H = _side(outs[i - 1], B, 8)
            src = nchw(outs[i - 1], B, 8, H)[:, :cin]
            want = O._gemm_conv(src, P[wk], P[bk], PR, padding=1)
            ck.rel(i, name, "conv_in", "X", out, rows(want), False)
            X = nchw(out, B, want.shape[1], H)
        elif leaf in ("norm1", "norm2", "group_norm", "conv_norm_out"):
            C = P[wk].shape[0]
            src = X if leaf != "norm2" else nchw(outs[i - 1], B, C, _side(outs[i - 1], B, C))
            info.setdefault("gn_ratio", {})[name] = group_ratio(src)
            want = _groupnorm64(src, P[wk], P[bk], leaf != "group_norm")
            ck.rel(i, name, "groupnorm", "H", out, rows(_q64(want)), True)
        elif leaf == "conv1":
            cin = P[wk].shape[1]
            src = nchw(outs[i - 1], B, cin, _side(outs[i - 1], B, cin))
            want = O._gemm_conv(src, P[wk], P[bk], PR, padding=1)
            ck.rel(i, name, "conv3x3", "T", out, rows(want), False)
        elif leaf == "conv_shortcut":                            # 1x1 on the fp32 loader: the residual stream itself is the operand
            want = O._gemm_conv(X, P[wk], P[bk], PR)
            ck.rel(i, name, "conv_shortcut", "S", out, rows(want), False)
            S = nchw(out, B, want.shape[1], X.shape[2])
        elif leaf == "conv2":
            j = i - 1 if names[i - 1].endswith(".norm2") else i - 2
            cin = P[wk].shape[1]
            src = nchw(outs[j], B, cin, _side(outs[j], B, cin))
            resid = S if names[i - 1].endswith(".conv_shortcut") else X
            want = resid + O._gemm_conv(src, P[wk], P[bk], PR, padding=1)
            ck.rel(i, name, "conv3x3", "X", out, rows(want), False)
            # the block's own contribution x' - x: the residual carries part of the norm of x'
            ck.rel(i, name, "conv3x3", "X'-X", out - rows(resid), rows(want - resid), False)
            X, S = nchw(out, B, want.shape[1], want.shape[2]), None
        elif name.endswith(".downsamplers.0.conv"):              # stride 2, zeros read past the right and bottom edge
            want = O._gemm_conv(F.pad(X, (0, 1, 0, 1)), P[wk], P[bk], PR, stride=2)
            got = nchw(out, B, want.shape[1], want.shape[2])
            ck.rel(i, name, "downsample", "X", got, want, False)
            ck.rel(i, name, "downsample", "last row", got[:, :, -1, :], want[:, :, -1, :], False)
            ck.rel(i, name, "downsample", "last col", got[:, :, :, -1], want[:, :, :, -1], False)
            X = nchw(out, B, want.shape[1], want.shape[2])
        elif leaf in ("to_q", "to_k", "to_v"):
            g = i - 1 - ("to_q", "to_k", "to_v").index(leaf)
            assert names[g].endswith(".group_norm"), names[g]
            h = outs[g].reshape(B, -1, 512)
            want = O._gemm_linear(h, P[wk], P[bk], PR)
            ck.rel(i, name, "linear", leaf[3:].upper(), out, want.reshape(-1), False)
        elif leaf == "softmax_qk_v":
            q, k, v = (outs[i - 3 + j].reshape(B, -1, 512) for j in range(3))
            info.setdefault("attn", {})[name] = attention_stats(q, k)
            ck.rel(i, name, "softmax_qk_v", "A", out, _q64(attention64(q, k, v)).reshape(-1), True)
        elif name.endswith(".to_out.0"):
            a = outs[i - 1].reshape(B, -1, 512)
            o = O._gemm_linear(a, P[wk], P[bk], PR)
            want = X + o.transpose(1, 2).reshape(X.shape)
            ck.rel(i, name, "to_out", "X", out, rows(want), False)
            ck.rel(i, name, "to_out", "X'-X", out - rows(X), rows(want - X), False)
            X = nchw(out, B, 512, X.shape[2])
        elif name.endswith(".upsamplers.0.nearest"):
            want = F.interpolate(PR.q(X), scale_factor=2.0, mode="nearest")
            ck.exact(i, name, "nearest", "U", out, rows(want))
        elif name.endswith(".upsamplers.0.conv"):
            C, H = X.shape[1], 2 * X.shape[2]
            want = O._gemm_conv(nchw(outs[i - 1], B, C, H), P[wk], P[bk], PR, padding=1)
            ck.rel(i, name, "upsample_conv", "X", out, rows(want), False)
            X = nchw(out, B, C, H)
        elif leaf == "conv_out":                                # N = 8 / N = 3 output columns
            cin = P[wk].shape[1]
            src = nchw(outs[i - 1], B, cin, X.shape[2])
            want = O._gemm_conv(src, P[wk], P[bk], PR, padding=1)
            ck.rel(i, name, "conv_out", "out", out, rows(want), False)
        elif name == "quant_conv.sample":
            Lr = X.shape[2]
            mom = nchw(outs[i - 1], B, 8, Lr).double()          # the encoder.conv_out output this launch read
            m = F.conv2d(mom, P["quant_conv.weight"].double(), P["quant_conv.bias"].double())
            lv = m[:, 4:]
            info["logvar"] = (float((lv < -30.0).double().mean()), float((lv > 20.0).double().mean()))
            if feed.get("noise") is not None:
                want = (m[:, :4] + torch.exp(0.5 * lv.clamp(-30.0, 20.0)) * feed["noise"].double()) * 0.18215
                ck.rel(i, name, "quant_conv.sample", "latents", out, want.reshape(-1), False)
            else:
                ck.rel(i, name, "quant_conv.sample", "moments", out, m.reshape(-1), False)
        elif name == "decoder.output":
            H = X.shape[2]
            ck.exact(i, name, "decoder.output", "images", out, nchw(outs[i - 1], B, 3, H).reshape(-1))
        else:
            ck.no_rule(i, name)


def _scan_last(P, names, outs, B, feed, ck, info, X):
    """The rule of the program's last launch alone (outs holds the last two launches' outputs)."""
    _scan(P, names, outs, B, feed, ck, info, first=len(names) - 1, X=X)


def attention64(q, k, v):
    """softmax(Q K^T / sqrt(512)) V in float64."""
    q, k, v = q.double(), k.double(), v.double()
    return torch.softmax(q @ k.transpose(1, 2) / math.sqrt(q.shape[-1]), dim=-1) @ v


# ---------------------------------------------------------------------------------------------- entry points
def _encode_run(vae, xd, R, vae_range, nzd):
    if nzd is None:
        return lambda: vae._encode(xd, R, vae_range, True, None, 0)
    return lambda: vae._encode(xd, R, vae_range, False, nzd, 0)


def encode_scan(vae, P, x, image_res, report, noise=None, vae_range=False, info=None, fp32_bound=FP32_BOUND, bf16_bound=BF16_BOUND):
    """Every launch of hd_vae_encode(x [B,3,r,r] -> image_res; noise [B,4,L,L]: the posterior sample, None: the moments).
    Returns {launch kind: worst rel-L2}; info (a dict) receives the statistics of the inputs the launches read."""
    xd = x.cuda()
    nzd = noise.cuda() if noise is not None else None
    names, outs = _prefix_outputs(PrefixRun(vae._ctx, _encode_run(vae, xd, image_res, vae_range, nzd)))
    ck = _check(report, fp32_bound, bf16_bound)
    _scan(P, names, outs, x.shape[0], {"images": x, "vae_range": vae_range, "noise": noise}, ck, info if info is not None else {})
    # the last launch has two forms (vae_sample_kernel / vae_moments_kernel): the other one, in a whole run of its own
    n, Lr = len(names), image_res // 8
    _encode_run(vae, xd, image_res, vae_range, None if nzd is not None else torch.zeros(x.shape[0], 4, Lr, Lr).cuda())()
    tail = [None] * (n - 2) + [read_op(vae._ctx, 0, n - 2), read_op(vae._ctx, 0, n - 1)]
    Xl = torch.zeros(x.shape[0], 1, Lr, Lr)                      # only its side is used by the rule
    _scan_last(P, names, tail, x.shape[0], {"noise": None if nzd is not None else torch.zeros(x.shape[0], 4, Lr, Lr)}, ck, {}, Xl)
    ck.worst["launches"] = n
    return ck.worst


def decode_scan(vae, P, z, report, info=None, fp32_bound=FP32_BOUND, bf16_bound=BF16_BOUND):
    """Every launch of hd_vae_decode(z [B,4,L,L] scaled latents)."""
    zd = z.cuda()
    names, outs = _prefix_outputs(PrefixRun(vae._ctx, lambda: vae.decode_scaled(zd), 1, 0))
    ck = _check(report, fp32_bound, bf16_bound)
    _scan(P, names, outs, z.shape[0], {"latents": z}, ck, info if info is not None else {})
    ck.worst["launches"] = len(names)
    return ck.worst


def attention_prefix(vae, which, run, B, report, bf16_bound=BF16_BOUND):
    """The program run up to `...softmax_qk_v` only; Q, K, V are the to_q / to_k / to_v outputs (buffers of their own, written by
    nothing else, so one prefix run holds all four).  Returns (rel-L2 of the attention output against float64 rounded to bf16,
    attention_stats of the Q, K it read)."""
    pre = PrefixRun(vae._ctx, run, which, 0)
    try:
        pre.run_to(1)
        names = pre.names()
        s = next(i for i, n in enumerate(names) if n.endswith(".softmax_qk_v"))
        assert [n.split(".")[-1] for n in names[s - 3:s]] == ["to_q", "to_k", "to_v"], names[s - 3:s]
        pre.run_to(s + 1)
        qq, k, v = (pre.op(s - 3 + j).reshape(B, -1, 512) for j in range(3))
        got = pre.op(s)
    finally:
        pre.reset()
    ck = _check(report, FP32_BOUND, bf16_bound)
    ck.rel(s, names[s], "softmax_qk_v", f"T={qq.shape[1]}", got, _q64(attention64(qq, k, v)).reshape(-1), True)
    return ck.worst["softmax_qk_v"], attention_stats(qq, k)


def first_op(vae, x, image_res, vae_range=False):
    """Launch 0 of the encode program alone (limit 1): the bicubic resize when x is not image_res wide, else encoder.input."""
    xd = x.cuda()
    pre = PrefixRun(vae._ctx, lambda: vae._encode(xd, image_res, vae_range, True, None, 0))
    try:
        pre.run_to(1)
        return pre.names()[0], pre.op(0)
    finally:
        pre.reset()


def main():
    import argparse
    from hifidiff_amd import synth
    from hifidiff_amd.vae import AutoencoderKL
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--image-res", type=int, default=64)
    ap.add_argument("--in-res", type=int, default=0, help="side of the input images (default: image-res, no bicubic launch)")
    ap.add_argument("--stress", action="store_true", help="the stress weight set (stress_state_dict)")
    ap.add_argument("--out", default="vae_forced.txt", help="report file")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))      # noqa: E731
    P = synth.vae_state_dict()
    if a.stress:
        P = stress_state_dict(P)
    vae = AutoencoderKL(); vae.load_state_dict(P); vae.to("cuda:0")
    B, R, r = a.batch, a.image_res, a.in_res or a.image_res
    x = T(np.stack([synth.rand(f"cr_face_vae/{f}", (3, r, r)) for f in range(B)]))
    nz = T(np.stack([synth.randn(f"vae_noise/{f}", (4, R // 8, R // 8)) for f in range(B)]))
    z = T(np.stack([np.float32(0.8) * synth.randn(f"vae_z/{f}", (4, R // 8, R // 8)) for f in range(B)]))
    report, info = [], {}
    report.append(f"== encode, {r} -> {R} px, batch {B}, {'stress' if a.stress else 'plain'} weights")
    we = encode_scan(vae, P, x, R, report, noise=nz, info=info)
    report.append(f"== decode, latent {R // 8}, batch {B}")
    wd = decode_scan(vae, P, z, report, info=info)
    with open(a.out, "w") as f:
        f.write("\n".join(report) + "\n")
        f.write(f"worst per launch kind, encode: {we}\nworst per launch kind, decode: {wd}\ninputs: {info}\n")
    bad = [ln for ln in report if "<<<<<<" in ln or "no rule" in ln]
    print("\n".join(bad[:40]))
    print(f"encode {we}\ndecode {wd}\n{len(bad)} flagged of {len(report)} lines; report in {a.out}")


if __name__ == "__main__":
    main()
