#!/usr/bin/env python3
"""Teacher-forced parity of CoarseRestoration: every launch of hd_cr_forward against the CPU oracle ON THE LAUNCH'S OWN INPUTS
(the pattern of tools/vae_forced.py, for the program built in hd_aux.hip from the kernels of hd_cr.hpp and the refiner path).

The level buffers are reused by every stage, so the state is taken by prefix runs: for n = 1 .. N the program runs with
`hd_debug_limit_ops(ctx, 0, n)`; the output of launch n - 1 (`hd_debug_read_op`) and the side buffers that launch wrote
(`hd_debug_read`: pooled*, S*, sx* / sy*, Xb* / Yb*, theta, loc1, loc2) are read back and kept on the host.  Every rule applies
the oracle's arithmetic for that one launch (bf16-operand emulation at the points the kernels round, O.BF16) to values the HIP
path itself produced.  Bounds:
  * launches with a bf16 operand: rel-L2 3e-4 for fp32 outputs, 3e-3 for bf16-stored outputs (as tools/op_forced.py); the bf16
    copies (Xb / Yb / pooled16) and pure data movement are bit-exact against RNE-bf16 of the fp32 values read back;
  * launches without one (intro, outro, the two localisation convs, theta, the grid sample, pool_finish) are held against
    float64: max-abs error at most 4 x the max-abs error of torch's own fp32 CPU evaluation of the same op on the same inputs
    (summation order and FMA contraction differ, nothing else should; exactly 0 where torch's is 0) and rel-L2 <= 3e-4;
  * LayerNorm partials (sx / sy, (mean, M2) per 32 or C values of a row): mean against float64 of the values the partial covers,
    error in units of the row's std (sqrt(var + 1e-6), the LayerNorm's own denominator), and 1 / sqrt(M2 / cnt + 1e-6) against
    float64, relative; both <= 3e-4.  `max |row mean| / row std` is printed per statistics buffer.
A line over its bound carries `<<<<<<`; a launch without a rule is reported as `no rule`.  (Test infrastructure: uses oracle/.)
"""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hifidiff_amd import _lib, arch                            # noqa: E402
from oracle import hifidiff_oracle as O                         # noqa: E402

PR = O.BF16
FP32_BOUND, BF16_BOUND, STAT_BOUND, F64_MARGIN = 3e-4, 3e-3, 3e-4, 4.0
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


# ---------------------------------------------------------------------------------------------- helpers
def _names(L, ctx):
    return [L.hd_debug_op_name(ctx, 0, i).decode() for i in range(L.hd_num_ops(ctx, 0))]


def _read_op(L, ctx, i):
    n = L.hd_debug_read_op(ctx, 0, i, None, 0)
    _lib.check(n, ctx)
    buf = np.empty(n, dtype=np.float32)
    _lib.check(L.hd_debug_read_op(ctx, 0, i, buf.ctypes.data_as(ctypes.c_void_p), n), ctx)
    return torch.from_numpy(buf)


def read_buffer(ctx, name):
    L = _lib.lib()
    n = L.hd_debug_read(ctx, name.encode(), None, 0)
    _lib.check(n, ctx)
    buf = np.empty(n, dtype=np.float32)
    _lib.check(L.hd_debug_read(ctx, name.encode(), buf.ctypes.data_as(ctypes.c_void_p), n), ctx)
    return torch.from_numpy(buf)


def _nchw(flat, B, C, H):
    return flat[:B * H * H * C].reshape(B, H, H, C).permute(0, 3, 1, 2).contiguous()


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1) if t.dim() == 4 else t.reshape(-1)


def _rel(got, want):
    d = got.double() - want.double()
    return float(d.norm() / want.double().norm().clamp_min(1e-30)), float(d.abs().max())


def _q(x):
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float32)


class _Check:
    def __init__(self, report):
        self.report = report
        self.worst = {}                                         # launch kind -> worst rel-L2 (exact kinds: number of differing elements)
        self.f64 = {}                                           # fp32-only kinds -> (kernel max-abs, torch fp32 max-abs) of the worst ratio
        self.ratio = {}                                         # statistics buffer (by launch name) -> max |row mean| / row std

    def _line(self, i, name, what, text, ok):
        self.report.append(f"{i:3d} {name:44s} {what:10s} {text}{'' if ok else '  <<<<<<'}")

    def rel(self, i, name, kind, what, got, want, stored_bf16):
        rel, mx = _rel(got, want)
        lim = BF16_BOUND if stored_bf16 else FP32_BOUND
        if rel != rel:
            rel = 1e9
        self.worst[kind] = max(self.worst.get(kind, 0.0), rel)
        self._line(i, name, what, f"rel {rel:.3e} maxabs {mx:.3e} ({'bf16' if stored_bf16 else 'fp32'} <= {lim:.0e})", rel <= lim)

    def exact(self, i, name, kind, what, got, want):
        bad = int((got.view(torch.int32) != want.contiguous().view(torch.int32)).sum()) if got.shape == want.shape else max(got.numel(), want.numel())
        self.worst[kind] = max(self.worst.get(kind, 0), bad)
        self._line(i, name, what, f"{bad} of {want.numel()} elements differ (bit-exact)", bad == 0)

    def against64(self, i, name, kind, what, got, ref64, ref32):
        """No bf16 operand: max-abs error <= 4 x torch's fp32 error against the same float64 result, and rel-L2 <= 3e-4."""
        rel, err = _rel(got, ref64)
        err32 = float((ref32.double() - ref64).abs().max())
        if rel != rel:
            rel, err = 1e9, 1e9
        self.worst[kind] = max(self.worst.get(kind, 0.0), rel)
        old = self.f64.get(kind)
        if old is None or err * max(old[1], 1e-300) > old[0] * max(err32, 1e-300) or (err32 == 0.0 and err > 0.0):
            self.f64[kind] = (err, err32)
        self._line(i, name, what, f"rel {rel:.3e} maxabs {err:.3e} (torch fp32 {err32:.3e}; <= {F64_MARGIN:.0f} x that, rel <= {FP32_BOUND:.0e})",
                   err <= F64_MARGIN * err32 and rel <= FP32_BOUND)

    def stats(self, i, name, what, sflat, vals, np_, cnt):
        """sflat: [M][np_] (mean, M2) partials as read back; vals: [M, np_ * cnt] the fp32 values they describe (read back)."""
        M = vals.shape[0]
        s = sflat[:M * np_ * 2].reshape(M, np_, 2).double()
        v = vals.double().reshape(M, np_, cnt)
        mean64 = v.mean(-1)
        m2_64 = (v - mean64[..., None]).pow(2).sum(-1)
        row_std = (vals.double().var(1, unbiased=False) + 1e-6).sqrt()
        mean_err = float(((s[..., 0] - mean64).abs() / row_std[:, None]).max())
        rstd, rstd64 = 1.0 / (s[..., 1] / cnt + 1e-6).sqrt(), 1.0 / (m2_64 / cnt + 1e-6).sqrt()
        rstd_err = float(((rstd - rstd64).abs() / rstd64).max())
        if mean_err != mean_err or rstd_err != rstd_err:
            mean_err = rstd_err = 1e9
        ratio = float((vals.double().mean(1).abs() / row_std).max())
        self.ratio[f"{name} {what}"] = ratio
        self.worst["stats"] = max(self.worst.get("stats", 0.0), mean_err, rstd_err)
        self._line(i, name, what, f"{np_} x {cnt}: mean err / row std {mean_err:.3e}, rstd rel err {rstd_err:.3e} (<= {STAT_BOUND:.0e}); max |row mean| / row std {ratio:.2f}",
                   mean_err <= STAT_BOUND and rstd_err <= STAT_BOUND)
        return mean_err, rstd_err, ratio


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


def _side_buffers(leaf, l, samp, form):
    s = str(l)
    if leaf == "intro":
        return ["Xb0", "sx0"]
    if leaf == "conv2_gate_pool":
        return ["pooled" + s, "pooled16_" + s] if form == "fused" else []
    if leaf == "conv3":
        return ["sy" + s, "Yb" + s]
    if leaf == "conv5":
        return ["sx" + s, "Xb" + s] + (["pooled" + s] if form == "chain" else [])
    if leaf == "stn":
        return ["Yb" + s]
    if leaf == "skip_add":
        return ["sx" + s, "Xb" + s]
    if leaf == "sampling":
        d = str(l + 1 if samp == "down" else l - 1)
        return ["sx" + d, "Xb" + d]
    return []


# ---------------------------------------------------------------------------------------------- the rules
class _Scan:
    def __init__(self, P, B, x, ck, info):
        self.P, self.B, self.x, self.ck, self.info = P, B, x, ck, info
        self.stages = _stage_table()
        self.st = {}                                            # buffer name -> latest value read back (flat, fp32)
        self.gate = {}                                          # level -> (float64, fp32) gate of the unfused depthwise launch, for pool_finish

    def ln(self, x, p, which):
        return O.layernorm2d(x, self.P[f"{p}.norm{which}.weight"], self.P[f"{p}.norm{which}.bias"], prec=PR)

    def gate_of_x(self, p, l, C, H):
        """conv1 -> depthwise 3x3 -> SimpleGate on the HIP path's own block input (X is not written before conv5)."""
        P = self.P
        h = self.ln(_nchw(self.st[f"X{l}"], self.B, C, H), p, 1)
        t1 = O._gemm_conv(h, P[p + ".conv1.weight"], P[p + ".conv1.bias"], PR)
        return O.simple_gate(F.conv2d(t1, P[p + ".conv2.weight"], P[p + ".conv2.bias"], padding=1, groups=2 * C))

    def copy_and_stats(self, i, name, l, which, vals_flat, C, np_, cnt):
        """The bf16 copy and the LayerNorm partials a launch wrote next to its fp32 output `vals_flat` (channels-last rows)."""
        M = vals_flat.numel() // C
        b, s = ("Xb", "sx") if which == "x" else ("Yb", "sy")
        self.ck.exact(i, name, "bf16_copy", f"{b}{l}", self.new[f"{b}{l}"][:M * C], _q(vals_flat))
        self.ck.stats(i, name, f"{s}{l}", self.new[f"{s}{l}"], vals_flat.reshape(M, C), np_, cnt)

    def form(self, names, i, leaf, C, H):
        strips = (C, H) in ((128, 32), (256, 16))
        if leaf == "conv2_gate_pool":
            return "unfused" if names[i - 1].endswith(".conv1") else "strips" if strips else "fused"
        if leaf == "conv5":
            return "chain" if names[i - 1].endswith(".conv2_gate_pool") else "gemm"
        return ""

    def rule(self, i, names, out, new):
        """out: the launch's output read back; new: its side buffers read back; self.st: everything before the launch."""
        P, B, ck, st = self.P, self.B, self.ck, self.st
        name = names[i]
        self.new = new
        stage, l, p, leaf = _parse(name, self.stages)
        C, H = 32 << l, 128 >> l
        M = B * H * H
        s = str(l)
        upd = dict(new)
        if leaf == "intro":
            w, b = P["intro.weight"], P["intro.bias"]
            ck.against64(i, name, "intro", "X0", out, _rows(F.conv2d(self.x.double(), w.double(), b.double(), padding=1)), _rows(F.conv2d(self.x, w, b, padding=1)))
            self.copy_and_stats(i, name, 0, "x", out, 32, 1, 32)
            upd["X0"] = out
        elif leaf == "outro":
            w, b = P["outro.weight"], P["outro.bias"]
            X = _nchw(st["X0"], B, 32, 128)
            ck.against64(i, name, "outro", "image", out, F.conv2d(X.double(), w.double(), b.double(), padding=1).reshape(-1), F.conv2d(X, w, b, padding=1).reshape(-1))
        elif leaf == "conv1":
            want = O._gemm_conv(self.ln(_nchw(st["X" + s], B, C, H), p, 1), P[p + ".conv1.weight"], P[p + ".conv1.bias"], PR)
            ck.rel(i, name, "conv1", "T1", out, _rows(want), False)
            upd["T1_" + s] = out
        elif leaf == "conv2_gate_pool":
            form = self.form(names, i, leaf, C, H)
            kind = "conv2_gate_pool." + form
            if form == "unfused":
                t1 = _nchw(st["T1_" + s], B, 2 * C, H)
                w2, b2 = P[p + ".conv2.weight"], P[p + ".conv2.bias"]
                g = O.simple_gate(F.conv2d(t1, w2, b2, padding=1, groups=2 * C))
                self.gate[l] = (O.simple_gate(F.conv2d(t1.double(), w2.double(), b2.double(), padding=1, groups=2 * C)), g)
            else:
                g = self.gate_of_x(p, l, C, H)
            got, want = _nchw(out, B, C, H), PR.q(g)
            ck.rel(i, name, kind, "G", got, want, True)
            if form == "unfused":                               # 8-row bands: the rows on either side of a seam, and the face's border lines
                ys = torch.arange(H)
                for what, a, b in (("band top", got[:, :, ys % 8 == 0], want[:, :, ys % 8 == 0]), ("band bottom", got[:, :, ys % 8 == 7], want[:, :, ys % 8 == 7]),
                                   ("first row", got[:, :, 0], want[:, :, 0]), ("last row", got[:, :, -1], want[:, :, -1]),
                                   ("first col", got[:, :, :, 0], want[:, :, :, 0]), ("last col", got[:, :, :, -1], want[:, :, :, -1])):
                    ck.rel(i, name, kind, what, a, b, True)
            if form == "fused":
                ck.rel(i, name, kind, "pooled", new["pooled" + s][:B * C], g.mean(dim=(2, 3)).reshape(-1), False)
                ck.exact(i, name, "bf16_copy", "pooled16", new["pooled16_" + s][:B * C], _q(new["pooled" + s][:B * C]))
            upd["G" + s] = out
        elif leaf == "pool_finish":
            g64, g32 = self.gate.pop(l)
            ck.against64(i, name, "pool_finish", "pooled", out, g64.mean(dim=(2, 3)).reshape(-1), g32.mean(dim=(2, 3)).reshape(-1))
            upd["pooled" + s] = out
        elif leaf == "sca":
            f32 = names[i - 1].endswith(".pool_finish")          # LK_F32 on the fp32 pooled vector; else the bf16 copy the fused conv1 left
            pooled = (st["pooled" + s] if f32 else st["pooled16_" + s])[:B * C].reshape(B, C, 1, 1)
            sv = O._gemm_conv(pooled, P[p + ".sca.1.weight"], P[p + ".sca.1.bias"], PR)
            ck.rel(i, name, "sca.f32" if f32 else "sca.bf16", "S", out, sv.reshape(-1), False)
            upd["S" + s] = out
        elif leaf == "conv3":
            X = _nchw(st["X" + s], B, C, H)
            g = PR.q(_nchw(st["G" + s], B, C, H) * st["S" + s][:B * C].reshape(B, C, 1, 1))     # the loader scales G by S and rounds
            y = X + O._gemm_conv(g, P[p + ".conv3.weight"], P[p + ".conv3.bias"], PR) * P[p + ".beta"]
            ck.rel(i, name, "conv3", "Y", out, _rows(y), False)
            ck.rel(i, name, "conv3", "Y-X", out - _rows(X), _rows(y - X), False)
            self.copy_and_stats(i, name, l, "y", out, C, C // 32, 32)
            upd["Y" + s] = out
        elif leaf == "conv4":
            h = self.ln(_nchw(st["Y" + s], B, C, H), p, 2)
            g2 = O.simple_gate(O._gemm_conv(h, P[p + ".conv4.weight"], P[p + ".conv4.bias"], PR))
            ck.rel(i, name, "conv4", "G2", out, _rows(PR.q(g2)), True)
            upd["G" + s] = out
        elif leaf == "conv5":
            chain = self.form(names, i, leaf, C, H) == "chain"
            g = _nchw(st["G" + s], B, C, H)
            if chain:                                            # sca -> conv3 -> LN -> conv4 -> gate -> conv5 in one launch, strip sums added up first
                X = _nchw(st["X" + s], B, C, H)
                pooled = new["pooled" + s][:B * C]
                ck.rel(i, name, "conv5.chain", "pooled", pooled, self.gate_of_x(p, l, C, H).mean(dim=(2, 3)).reshape(-1), False)
                sv = O._gemm_conv(pooled.reshape(B, C, 1, 1), P[p + ".sca.1.weight"], P[p + ".sca.1.bias"], PR)
                y = X + O._gemm_conv(PR.q(g * sv), P[p + ".conv3.weight"], P[p + ".conv3.bias"], PR) * P[p + ".beta"]
                g = PR.q(O.simple_gate(O._gemm_conv(self.ln(y, p, 2), P[p + ".conv4.weight"], P[p + ".conv4.bias"], PR)))
                base = X
            else:
                y = base = _nchw(st["Y" + s], B, C, H)
            want = y + O._gemm_conv(g, P[p + ".conv5.weight"], P[p + ".conv5.bias"], PR) * P[p + ".gamma"]
            kind = "conv5.chain" if chain else "conv5"
            ck.rel(i, name, kind, "X", out, _rows(want), False)
            # the launch's own contribution (the residual carries most of the norm of x'): a difference of fp32 outputs, fp32 bound
            ck.rel(i, name, kind, "X'-X" if chain else "X'-Y", out - _rows(base), _rows(want - base), False)
            self.copy_and_stats(i, name, l, "x", out, C, C // 32, 32)
            upd["X" + s] = out
        elif leaf in ("localization.0", "localization.3"):
            q = f"{stage}.stn.{leaf}"
            w, b = P[q + ".weight"], P[q + ".bias"]
            if leaf == "localization.0":
                src = _nchw(st["X" + s], B, C, H)
            else:
                h1 = (H - P[f"{stage}.stn.localization.0.weight"].shape[-1] + 1) // 2
                src = st["loc1"][:B * 8 * h1 * h1].reshape(B, 8, h1, h1)
            f = lambda t, w, b: torch.relu(F.max_pool2d(F.conv2d(t, w, b), 2, stride=2))     # noqa: E731
            ck.against64(i, name, leaf, "loc", out, f(src.double(), w.double(), b.double()).reshape(-1), f(src, w, b).reshape(-1))
            upd["loc1" if leaf == "localization.0" else "loc2"] = out
        elif leaf == "theta":
            q = f"{stage}.stn.fc_loc"
            xs = st["loc2"][:P[q + ".0.weight"].shape[1] * B].reshape(B, -1)
            f = lambda t, c: F.linear(torch.relu(F.linear(t, c(P[q + ".0.weight"]), c(P[q + ".0.bias"]))), c(P[q + ".2.weight"]), c(P[q + ".2.bias"]))     # noqa: E731
            ck.against64(i, name, "theta", "theta", out, f(xs.double(), lambda t: t.double()).reshape(-1), f(xs, lambda t: t).reshape(-1))
            self.info.setdefault("theta", {})[f"{stage}.stn"] = (out.reshape(B, 6).clone(), H)
            upd["theta"] = out
        elif leaf == "stn":
            X = _nchw(st["X" + s], B, C, H)
            th = st["theta"].reshape(B, 2, 3)
            f = lambda t, x: F.grid_sample(x, F.affine_grid(t, list(x.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)     # noqa: E731
            ck.against64(i, name, "grid_sample", "Y", out, _rows(f(th.double(), X.double())), _rows(f(th, X)))
            ck.exact(i, name, "bf16_copy", "Yb" + s, new["Yb" + s][:M * C], _q(out))
            upd["Y" + s] = out
        elif leaf == "sampling" and self.stages[stage][3] == "down":
            d, C2, H2 = l + 1, 2 * C, H // 2
            want = O._gemm_conv(_nchw(st["Yb" + s], B, C, H), P[stage + ".sampling.weight"], P[stage + ".sampling.bias"], PR, stride=2)
            ck.rel(i, name, "down", f"X{d}", out, _rows(want), False)
            self.copy_and_stats(i, name, d, "x", out, C2, C2 // 32, 32)
            upd[f"X{d}"] = out
        elif leaf == "skip_copy":
            ck.exact(i, name, "skip_copy", f"skip{l + 1}", out, st[f"X{l + 1}"])
            upd[f"skip{l + 1}"] = out
        elif leaf == "skip_add":
            want = st["Y" + s] + st["skip" + s]
            ck.exact(i, name, "skip_add", "X" + s, out, want)
            self.copy_and_stats(i, name, l, "x", out, C, 1, C)
            upd["X" + s] = out
        elif leaf == "sampling" and self.stages[stage][3] == "up":
            d, C2, H2 = l - 1, C // 2, 2 * H
            up = O._up_shuffle(_nchw(st["Yb" + s], B, C, H), P[stage + ".sampling.0.weight"], 2, PR)
            skip = _nchw(st[f"skip{d}"], B, C2, H2) if d >= 1 else None
            ck.rel(i, name, "up", f"X{d}", out, _rows(up + skip if skip is not None else up), False)
            if skip is not None:
                ck.rel(i, name, "up", "X-skip", out - _rows(skip), _rows(up), False)
            self.copy_and_stats(i, name, d, "x", out, C2, C2 // 32, 32)
            upd[f"X{d}"] = out
        else:
            ck.report.append(f"{i:3d} {name:44s} (no rule)")
        st.update(upd)


def _build(model, xd):
    L = _lib.lib()
    _lib.check(L.hd_debug_limit_ops(model._ctx, 0, 1), model._ctx)
    try:
        model(xd)                                               # builds the program for this batch
    finally:
        L.hd_debug_limit_ops(model._ctx, 0, -1)
    return _names(L, model._ctx)


def cr_scan(model, P, x, report, info=None):
    """Every launch of hd_cr_forward(x [B,3,128,128]).  Returns {launch kind: worst rel-L2 (exact kinds: differing elements)} plus "launches";
    info (a dict) receives "theta" {stn: ([B, 6], side)} as read back, "ratio" {statistics buffer: max |row mean| / row std} and "f64"
    {fp32-only kind: (kernel max-abs, torch fp32 max-abs)}."""
    L = _lib.lib()
    info = info if info is not None else {}
    xd = x.cuda()
    names = _build(model, xd)
    ck = _Check(report)
    sc = _Scan(P, x.shape[0], x, ck, info)
    try:
        for i, name in enumerate(names):
            _lib.check(L.hd_debug_limit_ops(model._ctx, 0, i + 1), model._ctx)
            model(xd)
            out = _read_op(L, model._ctx, i)
            stage, l, p, leaf = _parse(name, sc.stages)
            C, H = 32 << l, 128 >> l
            form = sc.form(names, i, leaf, C, H)
            new = {b: read_buffer(model._ctx, b) for b in _side_buffers(leaf, l, sc.stages[stage][3] if stage else None, form)}
            sc.rule(i, names, out, new)
    finally:
        L.hd_debug_limit_ops(model._ctx, 0, -1)
    ck.worst["launches"] = len(names)
    info["ratio"], info["f64"] = ck.ratio, ck.f64
    return ck.worst


def skip_add_prefix(model, P, x, report):
    """One prefix run up to the launch behind `decoders.0.skip_add` (the first decoder block's fused conv1 -> depthwise -> gate, which reads
    the 1 x 512 partials): the sum, its partials and bf16 copy, and that next launch's G.  Returns (mean error / row std, rstd relative
    error, max |row mean| / row std of the sum, rel-L2 of the next launch's G)."""
    L = _lib.lib()
    B = x.shape[0]
    xd = x.cuda()
    names = _build(model, xd)
    k = names.index("decoders.0.skip_add")
    assert names[k + 1] == "decoders.0.nfbs.0.conv2_gate_pool", names[k + 1]
    try:
        _lib.check(L.hd_debug_limit_ops(model._ctx, 0, k + 2), model._ctx)
        model(xd)                                               # the next launch writes G4 / pooled4 only: X4, sx4, Xb4, Y4, skip4 are as skip_add left them
        X4, G = _read_op(L, model._ctx, k), _read_op(L, model._ctx, k + 1)
        rd = {b: read_buffer(model._ctx, b) for b in ("Y4", "skip4", "sx4", "Xb4")}
    finally:
        L.hd_debug_limit_ops(model._ctx, 0, -1)
    ck = _Check(report)
    ck.exact(k, names[k], "skip_add", "X4", X4, rd["Y4"] + rd["skip4"])
    ck.exact(k, names[k], "bf16_copy", "Xb4", rd["Xb4"], _q(X4))
    mean_err, rstd_err, ratio = ck.stats(k, names[k], "sx4", rd["sx4"], X4.reshape(B * 64, 512), 1, 512)
    sc = _Scan(P, B, x, ck, {})
    sc.st["X4"] = X4
    g = sc.gate_of_x("decoders.0.nfbs.0", 4, 512, 8)
    ck.rel(k + 1, names[k + 1], "conv2_gate_pool.fused", "G", G, _rows(PR.q(g)), True)
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
