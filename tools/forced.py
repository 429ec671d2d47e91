"""What the teacher-forced scans share (tools/op_forced.py, cr_forced.py, prologue_forced.py, vae_forced.py): every launch of a
program against the CPU oracle ON THE LAUNCH'S OWN INPUTS.

  * read-back and layout helpers (`read_buffer`, `read_op`, `op_names`, `nchw`, `rows`, `rel`, `q`, `conv`);
  * `Check`: the report lines and the bounds.  Launches with a bf16 operand: rel-L2 <= FP32_BOUND for fp32 outputs, BF16_BOUND for
    bf16-stored outputs; bf16 copies and pure data movement bit-exact; launches without a bf16 operand against float64 (max-abs
    error at most F64_MARGIN x that of torch's own fp32 CPU evaluation on the same inputs, and rel-L2 <= FP32_BOUND); LayerNorm
    partials against float64 at STAT_BOUND.  A line over its bound carries `<<<<<<`, a launch without a rule is reported as `no rule`;
  * `PrefixRun`: the state is taken by prefix runs (`hd_debug_limit_ops`): what launch i reads is read back while launches
    0 .. i - 1 have run, what it wrote one launch later;
  * `NafRules`: the launch forms of the library's add_naf_block (hd_internal.hpp), which builds the NAF block of the denoiser, the
    FPG and CoarseRestoration alike, and the rules of the transitions between levels.
Every rule applies the oracle's arithmetic for that one launch (bf16-operand emulation at the points the kernels round, O.BF16) to
values the HIP path itself produced; tests/test_forced_rules_host.py holds the block rules against the oracle's taps without a GPU.
(Test infrastructure: uses oracle/.)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hifidiff_amd import _lib                                  # noqa: E402
from oracle import hifidiff_oracle as O                         # noqa: E402

PR = O.BF16
FP32_BOUND, BF16_BOUND, STAT_BOUND, F64_MARGIN = 3e-4, 3e-3, 3e-4, 4.0
STRIP_SHAPES = ((128, 32), (256, 16))                           # (C, H) of the faces add_naf_block runs by strips (hd_strip.hpp)


# ---------------------------------------------------------------------------------------------- read-back and layout
def _read(fn, ctx, *args):
    n = fn(ctx, *args, None, 0)                                 # the size first, then the values
    _lib.check(n, ctx)
    buf = np.empty(n, dtype=np.float32)
    _lib.check(fn(ctx, *args, buf.ctypes.data, n), ctx)
    return torch.from_numpy(buf)


def read_buffer(ctx, name):
    """A named buffer of the active workspace (hd_debug_read), flat fp32."""
    return _read(_lib.lib().hd_debug_read, ctx, name.encode())


def read_op(ctx, which, i):
    """The output of launch i of program `which` (hd_debug_read_op), flat fp32."""
    return _read(_lib.lib().hd_debug_read_op, ctx, which, i)


def op_names(ctx, which):
    L = _lib.lib()
    return [L.hd_debug_op_name(ctx, which, i).decode() for i in range(L.hd_num_ops(ctx, which))]


def nchw(flat, B, C, H):
    return flat[:B * H * H * C].reshape(B, H, H, C).permute(0, 3, 1, 2).contiguous()


def rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1) if t.dim() == 4 else t.reshape(-1)


def rel(got, want):
    d = got.double() - want.double()
    return float(d.norm() / want.double().norm().clamp_min(1e-30)), float(d.abs().max())


def q(x):
    """The bf16 value a kernel stores (RNE) for x (fp32 or a float64 reference), as fp32."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def conv(x, w, b, stride=1, padding=0, halves=False):
    """O._gemm_conv; halves: K summed in two halves of the input channels (the oracle's own reordering noise)."""
    x, w = PR.q(x), PR.q(w)
    if not halves:
        return F.conv2d(x, w, b, stride=stride, padding=padding)
    h = max(x.shape[1] // 2, 1)
    return F.conv2d(x[:, :h], w[:, :h], None, stride=stride, padding=padding) + F.conv2d(x[:, h:], w[:, h:], b, stride=stride, padding=padding)


# ---------------------------------------------------------------------------------------------- the checks
class Check:
    """batch: also take every rel-L2 over the rows of each single face and hold the worst face to the same bound (a fault confined to
    the ragged last row tile of a many-row GEMM disappears in the whole-tensor figure).  A max-abs figure is the worst face's by
    construction, LayerNorm partials and bit-exact outputs are per row / per element already."""

    def __init__(self, report, batch=None, fp32_bound=FP32_BOUND, bf16_bound=BF16_BOUND, name_width=44, what_width=10):
        self.report, self.B, self.fp32_bound, self.bf16_bound, self.widths = report, batch, fp32_bound, bf16_bound, (name_width, what_width)
        self.worst = {}                                         # launch kind -> worst rel-L2 (exact kinds: number of differing elements)
        self.stored = {"fp32": 0.0, "bf16": 0.0}                # how the output is stored -> worst rel-L2
        self.face = {}                                          # launch kind -> worst per-face rel-L2 (with batch)
        self.f64 = {}                                           # fp32-only kinds -> (kernel max-abs, torch fp32 max-abs) of the worst ratio
        self.ratio = {}                                         # statistics buffer (by launch name) -> max |row mean| / row std

    def _line(self, i, name, what, text, ok):
        self.report.append(f"{i:3d} {name:{self.widths[0]}s} {what:{self.widths[1]}s} {text}{'' if ok else '  <<<<<<'}")

    def note(self, i, name, text):
        self.report.append(f"{i:3d} {name:{self.widths[0]}s} ({text})")

    def no_rule(self, i, name):
        self.note(i, name, "no rule")

    def _per_face(self, got, want):
        d = (got.double() - want.double()).reshape(self.B, -1)
        r = d.norm(dim=1) / want.double().reshape(self.B, -1).norm(dim=1).clamp_min(1e-30)
        r = torch.where(r == r, r, torch.full_like(r, 1e9))
        return float(r.max()), int(r.argmax())

    def rel(self, i, name, kind, what, got, want, stored_bf16, alt=None):
        """alt: the same reference with K summed in two halves, evaluated and printed only on a line that is over its bound."""
        got, want = got.reshape(-1), want.reshape(-1)
        store = "bf16" if stored_bf16 else "fp32"
        lim = self.bf16_bound if stored_bf16 else self.fp32_bound
        if got.numel() != want.numel():
            self.worst[kind] = self.stored[store] = self.face[kind] = 1e9
            return self._line(i, name, what, f"size {got.numel()} vs {want.numel()}", False)
        r, mx = rel(got, want)
        r = r if r == r else 1e9
        self.worst[kind] = max(self.worst.get(kind, 0.0), r)
        self.stored[store] = max(self.stored[store], r)
        ok, face = r <= lim, ""
        if self.B:
            pf, f = self._per_face(got, want)
            self.face[kind] = max(self.face.get(kind, 0.0), pf)
            ok, face = ok and pf <= lim, f" worst face {pf:.3e} (face {f})"
        note = ""
        if not ok and alt is not None:                          # a finding: the oracle's own reordering noise for this launch
            a = alt().reshape(-1)
            note = f"; oracle K in two halves: rel {rel(a, want)[0]:.3e}" + (f" worst face {self._per_face(a, want)[0]:.3e}" if self.B else "")
        self._line(i, name, what, f"rel {r:.3e}{face} maxabs {mx:.3e} ({store} <= {lim:.0e}){note}", ok)

    def exact(self, i, name, kind, what, got, want):
        bad = int((got.view(torch.int32) != want.contiguous().view(torch.int32)).sum()) if got.shape == want.shape else max(got.numel(), want.numel())
        self.worst[kind] = max(self.worst.get(kind, 0), bad)
        self._line(i, name, what, f"{bad} of {want.numel()} elements differ (bit-exact)", bad == 0)

    def against64(self, i, name, kind, what, got, ref64, ref32):
        """No bf16 operand: max-abs error <= F64_MARGIN x torch's fp32 error against the same float64 result (summation order and FMA
        contraction differ, nothing else should; exactly 0 where torch's is 0), and rel-L2 <= FP32_BOUND."""
        got, ref64, ref32 = got.reshape(-1), ref64.reshape(-1), ref32.reshape(-1)
        r, err = rel(got, ref64)
        err32 = float((ref32.double() - ref64).abs().max())
        if r != r:
            r, err = 1e9, 1e9
        self.worst[kind] = max(self.worst.get(kind, 0.0), r)
        old = self.f64.get(kind)
        if old is None or err * max(old[1], 1e-300) > old[0] * max(err32, 1e-300) or (err32 == 0.0 and err > 0.0):
            self.f64[kind] = (err, err32)
        ok, face = err <= F64_MARGIN * err32 and r <= FP32_BOUND, ""
        if self.B:
            pf, f = self._per_face(got, ref64)
            self.face[kind] = max(self.face.get(kind, 0.0), pf)
            ok, face = ok and pf <= FP32_BOUND, f" worst face rel {pf:.3e} (face {f})"
        self._line(i, name, what, f"rel {r:.3e} maxabs {err:.3e} (torch fp32 {err32:.3e}; <= {F64_MARGIN:.0f} x that, rel <= {FP32_BOUND:.0e}){face}", ok)

    def stats(self, i, name, what, sflat, vals, np_, cnt):
        """sflat: [M][np_] (mean, M2) partials as read back; vals: [M, np_ * cnt] the fp32 values they describe (read back).  The mean
        against float64 of the values the partial covers, error in units of the row's std (sqrt(var + 1e-6), the LayerNorm's own
        denominator), and 1 / sqrt(M2 / cnt + 1e-6) against float64, relative."""
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

    def copy_and_stats(self, i, name, read, l, which, vals, C, np_, cnt):
        """The bf16 copy and the LayerNorm partials a launch wrote next to its fp32 output `vals` (channels-last rows) at level l."""
        M = vals.numel() // C
        b, s = ("Xb", "sx") if which == "x" else ("Yb", "sy")
        self.exact(i, name, "bf16_copy", f"{b}{l}", read(f"{b}{l}")[:M * C], q(vals))
        self.stats(i, name, f"{s}{l}", read(f"{s}{l}"), vals.reshape(M, C), np_, cnt)


# ---------------------------------------------------------------------------------------------- prefix runs
class PrefixRun:
    """run(*state) runs the program; limit: the program `hd_debug_limit_ops` stops, which: the one `hd_debug_read_op` reads (the two
    VAE programs share limit 0).  A named buffer is read while the launch that overwrites it has not yet run."""

    def __init__(self, ctx, run, which=0, limit=None):
        self.L, self.ctx, self.run, self.which, self.limit = _lib.lib(), ctx, run, which, which if limit is None else limit
        self.cur = None

    def run_to(self, n, *state):
        """Launches 0 .. n - 1 (cached: nothing runs while that is what the device holds)."""
        if self.cur != (n, state):
            _lib.check(self.L.hd_debug_limit_ops(self.ctx, self.limit, n), self.ctx)
            try:
                self.run(*state)
            except BaseException:                                # leave no limit behind for whoever uses the context next
                self.reset()
                raise
            self.cur = (n, state)

    def names(self):
        return op_names(self.ctx, self.which)

    def buf(self, name, n=None):
        return read_buffer(self.ctx, name)[:n]

    def op(self, i):
        assert i < self.cur[0], (i, self.cur)                   # the producer has run in this prefix
        return read_op(self.ctx, self.which, i)

    def reset(self):
        self.L.hd_debug_limit_ops(self.ctx, self.limit, -1)
        self.cur = None


class LaunchIO:
    """What launch i read (`before`: named buffers while launches 0 .. i - 1 have run) and wrote (`after`, and `out`, its output)."""

    def __init__(self, run, i):
        self.run, self.i = run, i

    def before(self, name):
        self.run.run_to(self.i)
        return self.run.buf(name)

    def after(self, name):
        self.run.run_to(self.i + 1)
        return self.run.buf(name)

    def out(self):
        self.run.run_to(self.i + 1)
        return self.run.op(self.i)


# ---------------------------------------------------------------------------------------------- the NAF block
def naf_gemm_rows(leaf, B, H):
    """Rows M of the GEMM launch `leaf` of a block on B faces of side H."""
    return B if leaf == "sca" else B * H * H


class NafRules:
    """One rule per launch form of add_naf_block: fused, by strips or unfused `conv2_gate_pool`; `pool_finish`; `sca` with or without
    the in-place rescale of G; `conv3`; `conv4`; `conv5` as a GEMM or as the chain kernel (hd_chain.hpp).  The form is derived from
    the launch names and the shape.
    extras: also the launch's own contribution (`Y-X`, `X'-Y`, `X'-X`: the residual carries most of the norm of the output; a
    difference of fp32 outputs, fp32 bound), the bf16 copies (bit-exact) and the LayerNorm partials the launch wrote.
    own_t1: the unfused form on its own inputs -- conv1's T1 is checked, the depthwise launch is held against T1 (with the rows at
    the seams of its 8-row bands) and `pool_finish` against the float64 gate of T1; else T1 is checked through the next launch's G
    and both against the oracle's conv1 -> depthwise -> gate of the block input."""

    def __init__(self, P, ck, extras=False, own_t1=False):
        self.P, self.ck, self.extras, self.own_t1 = P, ck, extras, own_t1
        self.gate = {}                                          # block -> (float64, fp32) gate of the unfused depthwise launch, for pool_finish

    def ln(self, x, p, which, affine):
        """affine: None for the plain block, else a callable: 1 / 2 (norm1 / norm2) -> the FiLM (shift, scale)."""
        h = O.layernorm2d(x, self.P[f"{p}.norm{which}.weight"], self.P[f"{p}.norm{which}.bias"], prec=PR)
        if affine is None:
            return h
        shift, scale = affine(which)
        return h * (scale + 1) + shift

    def gate_of_x(self, p, X, affine=None):
        """conv1 -> depthwise 3x3 -> SimpleGate on the HIP path's own block input (X is not written before conv5)."""
        P = self.P
        t1 = conv(self.ln(X, p, 1, affine), P[p + ".conv1.weight"], P[p + ".conv1.bias"])
        return O.simple_gate(F.conv2d(t1, P[p + ".conv2.weight"], P[p + ".conv2.bias"], padding=1, groups=t1.shape[1]))

    def launch(self, i, names, p, l, B, C, H, affine, io):
        """Launch i = names[i] of block p at level l (the suffix of the level's buffer names), B faces of C x H x H; io: LaunchIO."""
        P, ck = self.P, self.ck
        name, prev = names[i], names[i - 1] if i else ""
        leaf = name[len(p) + 1:]
        M, s = B * H * H, str(l)
        g4 = lambda flat: nchw(flat, B, C, H)                    # noqa: E731
        vec = lambda flat: flat[:B * C].reshape(B, C, 1, 1)      # noqa: E731
        wb = lambda k: (P[f"{p}.{k}.weight"], P[f"{p}.{k}.bias"])     # noqa: E731
        strips = (C, H) in STRIP_SHAPES
        if leaf == "conv1":
            if self.own_t1:
                want = conv(self.ln(g4(io.before("X" + s)), p, 1, affine), *wb("conv1"))
                ck.rel(i, name, "conv1", "T1", io.out(), rows(want), False)
            else:                                               # T1 has no check of its own here
                ck.note(i, name, "checked through the next launch's G")
        elif leaf == "conv2_gate_pool":
            form = "unfused" if prev.endswith(".conv1") else "strips" if strips else "fused"
            kind = "conv2_gate_pool." + form
            if form == "unfused" and self.own_t1:
                t1, (w2, b2) = nchw(io.before("T1_" + s), B, 2 * C, H), wb("conv2")
                g = O.simple_gate(F.conv2d(t1, w2, b2, padding=1, groups=2 * C))
                self.gate[p] = (O.simple_gate(F.conv2d(t1.double(), w2.double(), b2.double(), padding=1, groups=2 * C)), g)
            else:
                g = self.gate_of_x(p, g4(io.before("X" + s)), affine)
            got, want = g4(io.out()), PR.q(g)
            ck.rel(i, name, kind, "G", got, want, True)          # NCHW order, as the band lines below
            if form == "unfused" and self.own_t1:               # 8-row bands: the rows on either side of a seam, and the face's border lines
                ys = torch.arange(H)
                for what, a, b in (("band top", got[:, :, ys % 8 == 0], want[:, :, ys % 8 == 0]), ("band bottom", got[:, :, ys % 8 == 7], want[:, :, ys % 8 == 7]),
                                   ("first row", got[:, :, 0], want[:, :, 0]), ("last row", got[:, :, -1], want[:, :, -1]),
                                   ("first col", got[:, :, :, 0], want[:, :, :, 0]), ("last col", got[:, :, :, -1], want[:, :, :, -1])):
                    if a.numel():                               # a face of fewer than 8 rows has no seam
                        ck.rel(i, name, kind, what, a, b, True)
            if form == "fused":                                 # unfused: band sums only, by strips: per-strip sums; the mean comes later
                pooled = io.after("pooled" + s)[:B * C]
                ck.rel(i, name, kind, "pooled", pooled, g.mean(dim=(2, 3)), False)
                if self.extras:
                    ck.exact(i, name, "bf16_copy", "pooled16", io.after("pooled16_" + s)[:B * C], q(pooled))
        elif leaf == "pool_finish":
            if self.own_t1:
                g64, g32 = self.gate.pop(p)
                ck.against64(i, name, "pool_finish", "pooled", io.out(), g64.mean(dim=(2, 3)), g32.mean(dim=(2, 3)))
            else:
                g = self.gate_of_x(p, g4(io.before("X" + s)), affine)
                ck.rel(i, name, "pool_finish", "pooled", io.out()[:B * C], g.mean(dim=(2, 3)), False)
        elif leaf == "sca":
            f32 = prev.endswith(".pool_finish")                  # LK_F32 on the fp32 pooled vector; else the bf16 copy the fused conv1 left
            prescale = not f32 and H * H <= 16                   # the launch also rescales G in place (few pixels per face)
            pooled = vec(io.before(("pooled" if f32 else "pooled16_") + s))
            g = g4(io.before("G" + s)) if prescale else None
            w, b = wb("sca.1")
            sv = conv(pooled, w, b)
            ck.rel(i, name, "sca.f32" if f32 else "sca.prescale" if prescale else "sca.bf16", "S", io.out()[:B * C], sv, False,
                   lambda: conv(pooled, w, b, halves=True))
            if prescale:
                ck.rel(i, name, "sca.scale_G", "G*s", io.after("G" + s)[:M * C], rows(PR.q(g * sv)), True)
        elif leaf == "conv3":
            X, g = g4(io.before("X" + s)), g4(io.before("G" + s))
            if H * H > 16 or names[i - 2].endswith(".pool_finish"):      # else the sca launch has rescaled G; here the loader scales it, and rounds
                g = PR.q(g * vec(io.before("S" + s)))
            (w, b), beta = wb("conv3"), P[p + ".beta"]
            y, out = X + conv(g, w, b) * beta, io.out()[:M * C]
            alt = lambda: rows(X + conv(g, w, b, halves=True) * beta)            # noqa: E731
            ck.rel(i, name, "conv3", "Y", out, rows(y), False, alt)
            if self.extras:
                ck.rel(i, name, "conv3", "Y-X", out - rows(X), rows(y - X), False, lambda: alt() - rows(X))
                ck.copy_and_stats(i, name, io.after, l, "y", out, C, C // 32, 32)
        elif leaf == "conv4":
            h, (w, b) = self.ln(g4(io.before("Y" + s)), p, 2, affine), wb("conv4")
            ck.rel(i, name, "conv4", "G2", io.out()[:M * C], rows(PR.q(O.simple_gate(conv(h, w, b)))), True,
                   lambda: rows(PR.q(O.simple_gate(conv(h, w, b, halves=True)))))
        elif leaf == "conv5":
            chain = prev.endswith((".conv2_gate_pool", ".pool_finish"))      # levels 0 / 1: sca -> conv3 -> LN -> conv4 -> gate -> conv5 in one launch
            g, (w, b), gamma = g4(io.before("G" + s)), wb("conv5"), P[p + ".gamma"]
            kind = "conv5.chain" if chain else "conv5"
            if chain:
                base = X = g4(io.before("X" + s))
                if strips and prev.endswith(".conv2_gate_pool"):         # per-strip sums so far: this launch adds them up and stores the mean
                    pooled = io.after("pooled" + s)[:B * C]
                    ck.rel(i, name, kind, "pooled", pooled, self.gate_of_x(p, X, affine).mean(dim=(2, 3)), False)
                else:
                    pooled = io.before("pooled" + s)
                sv = conv(vec(pooled), *wb("sca.1"))
                y = X + conv(PR.q(g * sv), *wb("conv3")) * P[p + ".beta"]
                g = PR.q(O.simple_gate(conv(self.ln(y, p, 2, affine), *wb("conv4"))))
            else:
                y = base = g4(io.before("Y" + s))
            want, out = y + conv(g, w, b) * gamma, io.out()[:M * C]
            alt = lambda: rows(y + conv(g, w, b, halves=True) * gamma)           # noqa: E731
            ck.rel(i, name, kind, "X", out, rows(want), False, alt)
            if self.extras:
                ck.rel(i, name, kind, "X'-X" if chain else "X'-Y", out - rows(base), rows(want - base), False, lambda: alt() - rows(base))
                ck.copy_and_stats(i, name, io.after, l, "x", out, C, C // 32, 32)
        else:
            ck.no_rule(i, name)


# ---------------------------------------------------------------------------------------------- transitions between levels
def intro_rule(ck, i, name, kind, what, out, x, w, b, layout=rows):
    """A 3x3 conv without a bf16 operand, against float64."""
    ck.against64(i, name, kind, what, out, layout(F.conv2d(x.double(), w.double(), b.double(), padding=1)), layout(F.conv2d(x, w, b, padding=1)))


def down_rule(ck, i, name, what, out, src, w, b):
    """The stride-2 down conv (a patch-gather GEMM) on src."""
    ck.rel(i, name, "down", what, out, rows(conv(src, w, b, stride=2)), False, lambda: rows(conv(src, w, b, stride=2, halves=True)))


def up_rule(ck, i, name, what, out, src, w, skip, r=2, contribution=None):
    """1x1 conv (no bias) + PixelShuffle(r) + the skip (None: there is none).  contribution: the label of a second line, the launch's own
    part out - skip against the shuffled conv alone (None: not asked for)."""
    f = lambda halves: (lambda y: F.pixel_shuffle(y, r) if r > 1 else y)(conv(src, w, None, halves=halves))      # noqa: E731
    up = f(False)
    if skip is None:
        return ck.rel(i, name, "up", what, out, rows(up), False, lambda: rows(f(True)))
    ck.rel(i, name, "up", what, out, rows(up + skip), False, lambda: rows(f(True) + skip))
    if contribution:
        ck.rel(i, name, "up", contribution, out - rows(skip), rows(up), False, lambda: rows(f(True)))
