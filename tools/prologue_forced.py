#!/usr/bin/env python3
"""Teacher-forced parity of the conditioning prologue (hd_prepare, launch program 1: FPG, ResNet-50, HCA gates, idc_conv): every
launch against the CPU oracle ON THE LAUNCH'S OWN INPUTS (the pattern of tools/op_forced.py and tools/cr_forced.py, whose helpers,
bounds and block rules are used here).

The state is taken by prefix runs: `hd_debug_limit_ops(ctx, 1, i)` + `engine.prepare` runs launches 0 .. i - 1; what launch i reads is
then read back -- named buffers (`hd_debug_read`: the level buffers, `prior*`, `id_emb`) and, for the rotating ResNet buffers and the
gate temporaries, the output of the producing launch (`hd_debug_read_op`: it is intact while its consumer is next) -- and after one
more launch the output of launch i and the side buffers it wrote.  Every rule applies the oracle's arithmetic for that one launch
(oracle/hifidiff_oracle.py: fpg / naf_block, resnet50, hca_gates, _conv_bn, the idc_conv GEMM; bf16-operand emulation O.BF16, which
rounds the BN-folded weights as the packer does) to values the HIP path itself produced.  Bounds (none of them new):
  * GEMM launches with an fp32 output: rel-L2 <= 3e-4; bf16-stored outputs (every idc.* conv, G / G2 of the FPG blocks): <= 3e-3;
  * the FPG blocks by the block rules of the other two tools, the LayerNorm affine being the FiLM row (scale = shift = 0); the chain
    kernel of levels 0 / 1 holds X and X' - X;
  * LayerNorm partials a producer writes (fpg.intro, the downs, conv3 / conv5) against float64 at cr_forced.STAT_BOUND, the bf16
    copies next to them bit-exact; idc.input (layout + bf16 rounding) and idc.max_pool (a max of bf16 values) differ in 0 elements;
  * launches without a bf16 operand (fpg.intro, hcas.*.pool, hcas.*.spatial_mlp.3, idc.avgpool) against float64: max-abs error at most
    cr_forced.F64_MARGIN x the max-abs error of torch's own fp32 evaluation on the same inputs, and rel-L2 <= 3e-4;
  * PER FACE: every rel-L2 above is also taken over the rows of each single face and the worst face is held to the same bound (a
    fault confined to the ragged last row tile of a many-row GEMM disappears in the whole-tensor figure).  A max-abs figure is the
    worst face's by construction, LayerNorm partials and bit-exact outputs are per row / per element already.
A line over its bound carries `<<<<<<` and, where the launch is a GEMM, the oracle's own reordering noise for it (the same CPU
computation with K summed in two halves) is printed next to it; a launch without a rule is reported as `no rule`.
For every GEMM launch the dispatch tuple (loader, epilogue, mode, xcd_tile_affine, w_nt, M % tile rows != 0) is read with
hd_debug_op_info and recorded.  (Test infrastructure: uses oracle/.)
"""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cr_forced as CRF                                         # noqa: E402
from cr_forced import BF16_BOUND, F64_MARGIN, FP32_BOUND, STAT_BOUND, _nchw, _q, _rel, _rows, read_buffer      # noqa: E402
from hifidiff_amd import _lib                                  # noqa: E402
from oracle import hifidiff_oracle as O                         # noqa: E402

PR = O.BF16
PROLOGUE_OPS = {16: 160, 32: 160}                               # FPG 1 + 4 x 2 + 12 x 5 + 4 + 5, ResNet-50 56, gates 5 x 5, idc_conv (both latents)
LOADERS = ("F32", "LN", "BF16", "BF16S", "CONV_F32", "CONV_F32G", "CONV_BF16")
EPILOGUES = ("BIASF32", "RESID", "GATE", "PIXSHUF", "BIASBF16", "DWGATE", "SCA")
TILE_ROWS = {0: 128, 1: 64, 2: 64, 3: 32, 4: 32, 5: 128, 6: 256}
F64_KINDS = ("fpg.intro", "gate.pool", "gate.spatial_mlp.3", "idc.avgpool")
EXACT_KINDS = ("bf16_copy", "idc.input", "idc.max_pool")
BF16_KINDS = ("conv2_gate_pool.fused", "conv2_gate_pool.strips", "sca.scale_G", "conv4", "idc.conv7x7", "idc.1x1", "idc.3x3", "idc.3x3s2",
              "idc.downsample", "idc.downsample.s2", "idc.conv3")
KINDS_GATES = {"gate.pool", "gate.channel_mlp.0", "gate.channel_mlp.2", "gate.spatial_mlp.0", "gate.spatial_mlp.3", "idc_conv"}
KINDS_FPG16 = {"fpg.intro", "conv2_gate_pool.fused", "conv5.chain", "sca.prescale", "sca.scale_G", "conv3", "conv4", "conv5", "down", "up", "stats", "bf16_copy"}
KINDS_FPG32 = KINDS_FPG16 | {"conv2_gate_pool.strips", "sca.bf16"}            # 32 x 32 / 16 x 16 faces by strips, level 2 with the row scale in conv3's loader
KINDS_IDC = {"idc.input", "idc.max_pool", "idc.avgpool"} | {k for k in BF16_KINDS if k.startswith("idc.")}
KINDS_FULL16 = KINDS_FPG16 | KINDS_IDC | KINDS_GATES


def unpack_info(v):
    """hd_debug_op_info -> (loader, epilogue, mode, xcd_tile_affine, w_nt), or None for a launch that is no GEMM."""
    if v == 0:
        return None
    return (v & 0xff) - 1, ((v >> 8) & 0xff) - 1, ((v >> 16) & 0xff) - 1, (v >> 24) & 1, (v >> 25) & 1


def gemm_rows(name, B, latent):
    """Rows M of the GEMM launch `name` of the prologue at batch B."""
    lv = lambda l: B * (latent >> l) ** 2                       # noqa: E731
    p = name.split(".")
    if name == "idc_conv" or (p[0] == "hcas" and p[2] == "channel_mlp"):
        return B
    if p[0] == "hcas":
        return lv(4 - int(p[1]))
    if p[1] == "encoders":
        return B if p[4] == "sca" else lv(int(p[2]))
    if p[1] == "downs":
        return lv(int(p[2]) + 1)
    if p[1] == "convs":
        return lv(4 if p[2] == "0" else 5 - int(p[2]))
    if name == "idc.conv1":
        return B * 64 * 64
    li = int(p[1][5:])                                           # idc.layer<li>.<b>.<leaf>
    h_in = 32 >> (li - 1) if (p[2] != "0" or li == 1) else 32 >> (li - 2)
    h_out = 32 >> (li - 1)
    return B * (h_in if p[3] == "conv1" else h_out) ** 2


def op_tuple(L, ctx, i, name, B, latent):
    """(loader, epilogue, mode, affine, nt, ragged last row tile) of launch i of program 1, None if it is no GEMM."""
    v = L.hd_debug_op_info(ctx, 1, i)
    _lib.check(v, ctx)
    t = unpack_info(v)
    if t is None:
        return None
    rows = TILE_ROWS.get(t[2] & 15)
    return t + (int(rows is not None and gemm_rows(name, B, latent) % rows != 0),)


def tuple_text(t):
    return f"{LOADERS[t[0]]}/{EPILOGUES[t[1]]} mode {t[2]} affine {t[3]} nt {t[4]} ragged {t[5]}"


def program_tuples(engine, crl, crf):
    """{launch name: tuple or None} of the prologue at the batch of crl / crf: the program is built by a run of no launch."""
    L = _lib.lib()
    _lib.check(L.hd_debug_limit_ops(engine.ctx, 1, 0), engine.ctx)
    try:
        engine.prepare(crl.cuda(), cr_face=crf.cuda())
    finally:
        L.hd_debug_limit_ops(engine.ctx, 1, -1)
    B = crl.shape[0]
    names = [L.hd_debug_op_name(engine.ctx, 1, i).decode() for i in range(L.hd_num_ops(engine.ctx, 1))]
    return {n: op_tuple(L, engine.ctx, i, n, B, engine.latent_res) for i, n in enumerate(names)}


def _conv(x, w, b, stride=1, padding=0, halves=False):
    """O._gemm_conv; halves: K summed in two halves of the input channels (the oracle's own reordering noise)."""
    x, w = PR.q(x), PR.q(w)
    if not halves:
        return F.conv2d(x, w, b, stride=stride, padding=padding)
    h = max(x.shape[1] // 2, 1)
    return F.conv2d(x[:, :h], w[:, :h], None, stride=stride, padding=padding) + F.conv2d(x[:, h:], w[:, h:], b, stride=stride, padding=padding)


def _folded(P, conv, bn):
    """conv -> BatchNorm(eval) folded as O._conv_bn does in emulation mode (fp32, before rounding)."""
    s, o = O._bn_affine(P, bn)
    b = P.get(conv + ".bias")
    return P[conv + ".weight"] * s.view(-1, 1, 1, 1), (o if b is None else b * s + o)


class _Check(CRF._Check):
    """cr_forced's checks with the per-face figure: rel-L2 over the rows of each single face, the worst face against the same bound."""

    def __init__(self, report, B):
        super().__init__(report)
        self.B = B
        self.face = {}                                          # launch kind -> worst per-face rel-L2

    def _per_face(self, got, want):
        d = (got.double() - want.double()).reshape(self.B, -1)
        r = d.norm(dim=1) / want.double().reshape(self.B, -1).norm(dim=1).clamp_min(1e-30)
        r = torch.where(r == r, r, torch.full_like(r, 1e9))
        return float(r.max()), int(r.argmax())

    def rel(self, i, name, kind, what, got, want, stored_bf16, alt=None):
        got, want = got.reshape(-1), want.reshape(-1)
        lim = BF16_BOUND if stored_bf16 else FP32_BOUND
        if got.numel() != want.numel():
            self.worst[kind] = self.face[kind] = 1e9
            return self._line(i, name, what, f"size {got.numel()} vs {want.numel()}", False)
        rel, mx = _rel(got, want)
        rel = rel if rel == rel else 1e9
        pf, f = self._per_face(got, want)
        self.worst[kind] = max(self.worst.get(kind, 0.0), rel)
        self.face[kind] = max(self.face.get(kind, 0.0), pf)
        ok = rel <= lim and pf <= lim
        note = ""
        if not ok and alt is not None:                          # a finding: the oracle's own reordering noise for this launch
            a = alt().reshape(-1)
            note = f"; oracle K in two halves: rel {_rel(a, want)[0]:.3e} worst face {self._per_face(a, want)[0]:.3e}"
        self._line(i, name, what, f"rel {rel:.3e} worst face {pf:.3e} (face {f}) maxabs {mx:.3e} ({'bf16' if stored_bf16 else 'fp32'} <= {lim:.0e}){note}", ok)

    def against64(self, i, name, kind, what, got, ref64, ref32):
        got, ref64, ref32 = got.reshape(-1), ref64.reshape(-1), ref32.reshape(-1)
        n0 = len(self.report)
        super().against64(i, name, kind, what, got, ref64, ref32)
        pf, f = self._per_face(got, ref64)
        self.face[kind] = max(self.face.get(kind, 0.0), pf)
        ok = pf <= FP32_BOUND
        ln = self.report[n0]
        self.report[n0] = ln + f" worst face rel {pf:.3e} (face {f})" + ("" if ok or ln.endswith("<<<<<<") else "  <<<<<<")


class _Scan:
    def __init__(self, engine, P, crl, crf, ck):
        self.L, self.e, self.ctx, self.P, self.ck = _lib.lib(), engine, engine.ctx, P, ck
        self.B, self.lat = crl.shape[0], engine.latent_res
        self.crl, self.crf, self.crl_d, self.crf_d = crl, crf, crl.cuda(), crf.cuda()
        self.cur = None
        self.run_to(0)                                          # builds the program for this batch
        self.names = [self.L.hd_debug_op_name(self.ctx, 1, i).decode() for i in range(self.L.hd_num_ops(self.ctx, 1))]
        self.index = {n: i for i, n in enumerate(self.names)}
        self.res = self._resnet_table()

    # ---- state ----
    def run_to(self, n):
        if self.cur != n:
            _lib.check(self.L.hd_debug_limit_ops(self.ctx, 1, n), self.ctx)
            self.e.prepare(self.crl_d, cr_face=self.crf_d)
            self.cur = n

    def buf(self, name, n=None):
        t = read_buffer(self.ctx, name)
        return t if n is None else t[:n]

    def op(self, which):
        i = which if isinstance(which, int) else self.index[which]
        assert i < self.cur, (which, self.cur)                  # the producer has run in this prefix
        n = self.L.hd_debug_read_op(self.ctx, 1, i, None, 0)
        _lib.check(n, self.ctx)
        b = np.empty(n, dtype=np.float32)
        _lib.check(self.L.hd_debug_read_op(self.ctx, 1, i, b.ctypes.data_as(ctypes.c_void_p), n), self.ctx)
        return torch.from_numpy(b)

    def _resnet_table(self):
        """launch name -> (input launch, Cin, Hin, Cout, Hout, k, stride, pad, conv key, bn key, identity launch or None, relu, kind)"""
        tab = {"idc.conv1": ("idc.input", 3, 128, 64, 64, 7, 2, 3, "idc.conv1", "idc.batch_norm1", None, True, "idc.conv7x7")}
        x, H, cin = "idc.max_pool", 32, 64
        for li, nblk in enumerate((3, 4, 6, 3), start=1):
            pl = 32 << li
            for b in range(nblk):
                q = f"idc.layer{li}.{b}"
                st = 2 if (b == 0 and li > 1) else 1
                Ho = H // st
                tab[q + ".conv1"] = (x, cin, H, pl, H, 1, 1, 0, q + ".conv1", q + ".batch_norm1", None, True, "idc.1x1")
                tab[q + ".conv2"] = (q + ".conv1", pl, H, pl, Ho, 3, st, 1, q + ".conv2", q + ".batch_norm2", None, True, "idc.3x3s2" if st == 2 else "idc.3x3")
                idn = x
                if b == 0:
                    tab[q + ".i_downsample"] = (x, cin, H, 4 * pl, Ho, 1, st, 0, q + ".i_downsample.0", q + ".i_downsample.1", None, False,
                                                "idc.downsample.s2" if st == 2 else "idc.downsample")
                    idn = q + ".i_downsample"
                tab[q + ".conv3"] = (q + ".conv2", pl, Ho, 4 * pl, Ho, 1, 1, 0, q + ".conv3", q + ".batch_norm3", idn, True, "idc.conv3")
                x, H, cin = q + ".conv3", Ho, 4 * pl
        self.res_last = (x, cin, H)
        return tab

    # ---- shared pieces ----
    def ln(self, x, p, which):
        return O.layernorm2d(x, self.P[f"{p}.norm{which}.weight"], self.P[f"{p}.norm{which}.bias"], prec=PR)

    def gate_of_x(self, p, X):
        """conv1 -> depthwise 3x3 -> SimpleGate on the HIP path's own block input (cr_forced / op_forced: gate_of_x)."""
        P = self.P
        t1 = O._gemm_conv(self.ln(X, p, 1), P[p + ".conv1.weight"], P[p + ".conv1.bias"], PR)
        return O.simple_gate(F.conv2d(t1, P[p + ".conv2.weight"], P[p + ".conv2.bias"], padding=1, groups=t1.shape[1]))

    def copy_and_stats(self, i, name, l, which, vals, C, np_, cnt):
        """The bf16 copy and the LayerNorm partials the launch wrote next to its fp32 output `vals` (channels-last rows)."""
        M = vals.numel() // C
        b, s = ("Xb", "sx") if which == "x" else ("Yb", "sy")
        self.ck.exact(i, name, "bf16_copy", f"{b}{l}", self.buf(f"{b}{l}", M * C), _q(vals))
        self.ck.stats(i, name, f"{s}{l}", self.buf(f"{s}{l}"), vals.reshape(M, C), np_, cnt)

    # ---- the rules ----
    def rule(self, i):
        name = self.names[i]
        p = name.split(".")
        self.run_to(i)
        if name == "fpg.intro":
            self.intro(i, name)
        elif p[0] == "fpg" and p[1] == "encoders":
            self.block(i, name, int(p[2]), ".".join(p[:4]), p[4])
        elif p[0] == "fpg" and p[1] == "downs":
            self.down(i, name, int(p[2]))
        elif p[0] == "fpg" and p[1] == "convs":
            self.up(i, name, int(p[2]))
        elif name in self.res:
            self.resconv(i, name)
        elif name in ("idc.input", "idc.max_pool", "idc.avgpool"):
            self.resnet_other(i, name)
        elif p[0] == "hcas":
            self.gate(i, name, int(p[1]), ".".join(p[2:]))
        elif name == "idc_conv":
            self.idc_conv(i, name)
        else:
            self.ck.report.append(f"{i:3d} {name:44s} (no rule)")

    def intro(self, i, name):
        w, b = self.P["fpg.intro.weight"], self.P["fpg.intro.bias"]
        self.run_to(i + 1)
        out = self.op(i)
        self.ck.against64(i, name, "fpg.intro", "X0", out, _rows(F.conv2d(self.crl.double(), w.double(), b.double(), padding=1)), _rows(F.conv2d(self.crl, w, b, padding=1)))
        self.copy_and_stats(i, name, 0, "x", out, 128, 1, 128)

    def block(self, i, name, l, p, leaf):
        P, B, ck = self.P, self.B, self.ck
        C, H = 128 << l, self.lat >> l
        M, s = B * H * H, str(l)
        strips = (C, H) in ((128, 32), (256, 16))
        prev = self.names[i - 1]
        g4 = lambda flat: _nchw(flat, B, C, H)                   # noqa: E731
        if leaf == "conv2_gate_pool" and not prev.endswith(".conv1"):
            X = g4(self.buf("X" + s))
            self.run_to(i + 1)
            g = self.gate_of_x(p, X)
            kind = "conv2_gate_pool." + ("strips" if strips else "fused")
            ck.rel(i, name, kind, "G", self.op(i), _rows(PR.q(g)), True)
            if not strips:                                       # strips: per-strip sums only, the chain kernel adds them up
                pooled = self.buf("pooled" + s, B * C)
                ck.rel(i, name, kind, "pooled", pooled, g.mean(dim=(2, 3)).reshape(-1), False)
                ck.exact(i, name, "bf16_copy", "pooled16", self.buf("pooled16_" + s, B * C), _q(pooled))
        elif leaf == "conv5" and prev.endswith(".conv2_gate_pool"):
            # levels 0 / 1: sca -> conv3 -> LN -> conv4 -> gate -> conv5 in one launch (hd_chain.hpp), strip sums added up first
            X, g = g4(self.buf("X" + s)), g4(self.buf("G" + s))
            self.run_to(i + 1)
            out = self.op(i)
            pooled = self.buf("pooled" + s, B * C)
            if strips:
                ck.rel(i, name, "conv5.chain", "pooled", pooled, self.gate_of_x(p, X).mean(dim=(2, 3)).reshape(-1), False)
            sv = O._gemm_conv(pooled.reshape(B, C, 1, 1), P[p + ".sca.1.weight"], P[p + ".sca.1.bias"], PR)
            y = X + O._gemm_conv(PR.q(g * sv), P[p + ".conv3.weight"], P[p + ".conv3.bias"], PR) * P[p + ".beta"]
            g2 = PR.q(O.simple_gate(O._gemm_conv(self.ln(y, p, 2), P[p + ".conv4.weight"], P[p + ".conv4.bias"], PR)))
            want = y + O._gemm_conv(g2, P[p + ".conv5.weight"], P[p + ".conv5.bias"], PR) * P[p + ".gamma"]
            ck.rel(i, name, "conv5.chain", "X", out, _rows(want), False)
            ck.rel(i, name, "conv5.chain", "X'-X", out - _rows(X), _rows(want - X), False)
            self.copy_and_stats(i, name, l, "x", out, C, C // 32, 32)
        elif leaf == "sca":
            prescale = H * H <= 16                               # the launch also rescales G in place (few pixels per face)
            pooled16 = self.buf("pooled16_" + s, B * C).reshape(B, C, 1, 1)
            g = g4(self.buf("G" + s))
            self.run_to(i + 1)
            w, b = P[p + ".sca.1.weight"], P[p + ".sca.1.bias"]
            sv = _conv(pooled16, w, b)
            ck.rel(i, name, "sca.prescale" if prescale else "sca.bf16", "S", self.op(i)[:B * C], sv.reshape(-1), False, lambda: _conv(pooled16, w, b, halves=True))
            if prescale:
                ck.rel(i, name, "sca.scale_G", "G*s", self.buf("G" + s, M * C), _rows(PR.q(g * sv)), True)
        elif leaf == "conv3":
            X, g = g4(self.buf("X" + s)), g4(self.buf("G" + s))
            if H * H > 16:                                       # G is scaled by the loader instead, and rounded
                g = PR.q(g * self.buf("S" + s, B * C).reshape(B, C, 1, 1))
            self.run_to(i + 1)
            out = self.op(i)
            w, b, beta = P[p + ".conv3.weight"], P[p + ".conv3.bias"], P[p + ".beta"]
            y = X + _conv(g, w, b) * beta
            alt = lambda: _rows(X + _conv(g, w, b, halves=True) * beta)          # noqa: E731
            ck.rel(i, name, "conv3", "Y", out, _rows(y), False, alt)
            ck.rel(i, name, "conv3", "Y-X", out - _rows(X), _rows(y - X), False, lambda: alt() - _rows(X))
            self.copy_and_stats(i, name, l, "y", out, C, C // 32, 32)
        elif leaf == "conv4":
            h = self.ln(g4(self.buf("Y" + s)), p, 2)
            self.run_to(i + 1)
            w, b = P[p + ".conv4.weight"], P[p + ".conv4.bias"]
            ck.rel(i, name, "conv4", "G2", self.op(i), _rows(PR.q(O.simple_gate(_conv(h, w, b)))), True,
                   lambda: _rows(PR.q(O.simple_gate(_conv(h, w, b, halves=True)))))
        elif leaf == "conv5":
            Y, g = g4(self.buf("Y" + s)), g4(self.buf("G" + s))
            self.run_to(i + 1)
            out = self.op(i)
            w, b, gamma = P[p + ".conv5.weight"], P[p + ".conv5.bias"], P[p + ".gamma"]
            want = Y + _conv(g, w, b) * gamma
            alt = lambda: _rows(Y + _conv(g, w, b, halves=True) * gamma)         # noqa: E731
            ck.rel(i, name, "conv5", "X", out, _rows(want), False, alt)
            ck.rel(i, name, "conv5", "X'-Y", out - _rows(Y), _rows(want - Y), False, lambda: alt() - _rows(Y))
            self.copy_and_stats(i, name, l, "x", out, C, C // 32, 32)
        else:
            ck.report.append(f"{i:3d} {name:44s} (no rule)")

    def down(self, i, name, l):
        B, C, H = self.B, 128 << l, self.lat >> l
        xb = _nchw(self.buf(f"Xb{l}"), B, C, H)                 # gathers the bf16 copy conv5 wrote
        self.run_to(i + 1)
        out = self.op(i)
        w, b = self.P[f"fpg.downs.{l}.weight"], self.P[f"fpg.downs.{l}.bias"]
        self.ck.rel(i, name, "down", f"X{l + 1}", out, _rows(_conv(xb, w, b, stride=2)), False, lambda: _rows(_conv(xb, w, b, stride=2, halves=True)))
        self.copy_and_stats(i, name, l + 1, "x", out, 2 * C, 2 * C // 32, 32)

    def up(self, i, name, k):
        """fpg.convs.k: 1x1 conv, PixelShuffle(2) and the encoder skip (k = 0: no shuffle, no skip) -> prior k."""
        B, w = self.B, self.P[f"fpg.convs.{k}.0.weight"]
        hi = 4 if k == 0 else 5 - k
        src = _nchw(self.buf("X4" if k == 0 else f"prior{k - 1}"), B, 128 << hi, self.lat >> hi)
        skip = None if k == 0 else _nchw(self.buf(f"X{4 - k}"), B, 128 << (4 - k), self.lat >> (4 - k))
        self.run_to(i + 1)
        out = self.op(i)
        f = lambda halves: (lambda y: F.pixel_shuffle(y, 2) if k else y)(_conv(src, w, None, halves=halves))      # noqa: E731
        want = f(False)
        if skip is None:
            self.ck.rel(i, name, "up", "prior0", out, _rows(want), False, lambda: _rows(f(True)))
        else:
            self.ck.rel(i, name, "up", f"prior{k}", out, _rows(want + skip), False, lambda: _rows(f(True) + skip))
            self.ck.rel(i, name, "up", "P-skip", out - _rows(skip), _rows(want), False, lambda: _rows(f(True)))
        assert torch.equal(out, self.buf(f"prior{k}", out.numel()))          # the named buffer is the launch's output

    def resconv(self, i, name):
        B = self.B
        src, cin, Hin, cout, Hout, k, st, pad, conv, bn, idn, relu, kind = self.res[name]
        x = self.op(src)
        x = x.reshape(B, 128, 128, 8)[..., :3].permute(0, 3, 1, 2).contiguous() if name == "idc.conv1" else _nchw(x, B, cin, Hin)
        identity = _nchw(self.op(idn), B, cout, Hout) if idn else 0.0
        self.run_to(i + 1)
        w, b = _folded(self.P, conv, bn)

        def want(halves=False):
            y = _conv(x, w, b, stride=st, padding=pad, halves=halves) + identity
            return _rows(PR.q(torch.relu(y) if relu else y))
        self.ck.rel(i, name, kind, "out", self.op(i), want(), True, lambda: want(True))

    def resnet_other(self, i, name):
        B = self.B
        if name == "idc.input":
            self.run_to(i + 1)
            want = torch.zeros(B, 128, 128, 8)
            want[..., :3] = _q(self.crf.permute(0, 2, 3, 1))
            self.ck.exact(i, name, "idc.input", "face8", self.op(i), want.reshape(-1))
        elif name == "idc.max_pool":
            x = _nchw(self.op("idc.conv1"), B, 64, 64)
            self.run_to(i + 1)
            self.ck.exact(i, name, "idc.max_pool", "out", self.op(i), _rows(F.max_pool2d(x, 3, 2, 1)))
        else:
            src, C, H = self.res_last
            x = self.op(src).reshape(B, H * H, C)
            self.run_to(i + 1)
            out = self.op(i)
            self.ck.against64(i, name, "idc.avgpool", "id_emb", out, x.double().mean(1), x.mean(1))
            assert torch.equal(out, self.buf("id_emb", out.numel()))

    def gate(self, i, name, k, leaf):
        P, B, ck = self.P, self.B, self.ck
        l = 4 - k
        C, H = 128 << l, self.lat >> l
        q, n = f"denoiser.hcas.{k}", f"hcas.{k}"
        if leaf == "pool":
            pr = self.buf(f"prior{k}", B * H * H * C).reshape(B, H * H, C)
            self.run_to(i + 1)
            ck.against64(i, name, "gate.pool", "pool", self.op(i), pr.double().mean(1) + pr.double().amax(1), pr.mean(1) + pr.amax(1))
        elif leaf in ("channel_mlp.0", "channel_mlp.2"):
            x = self.op(n + (".pool" if leaf == "channel_mlp.0" else ".channel_mlp.0"))[:B * C].reshape(B, C, 1, 1)
            self.run_to(i + 1)
            w, b = P[f"{q}.{leaf}.weight"].reshape(C, C, 1, 1), P[f"{q}.{leaf}.bias"]
            act = torch.relu if leaf == "channel_mlp.0" else torch.sigmoid
            out = self.op(i)[:B * C]
            ck.rel(i, name, "gate." + leaf, "out", out, act(_conv(x, w, b)), False, lambda: act(_conv(x, w, b, halves=True)))
            if leaf == "channel_mlp.2":
                assert torch.equal(out, self.buf(f"wc{k}", B * C))
        elif leaf == "spatial_mlp.0":
            pr = _nchw(self.buf(f"prior{k}"), B, C, H)
            self.run_to(i + 1)
            w, b = _folded(P, q + ".spatial_mlp.0", q + ".spatial_mlp.1")
            ck.rel(i, name, "gate.spatial_mlp.0", "out", self.op(i)[:B * H * H * (C // 2)], _rows(torch.relu(_conv(pr, w, b))), False,
                   lambda: _rows(torch.relu(_conv(pr, w, b, halves=True))))
        elif leaf == "spatial_mlp.3":
            h = _nchw(self.op(n + ".spatial_mlp.0"), B, C // 2, H)
            self.run_to(i + 1)
            w, b = _folded(P, q + ".spatial_mlp.3", q + ".spatial_mlp.4")       # an fp32 VALU kernel on the folded weights (O._conv_bn, gemm=False)
            out = self.op(i)[:B * H * H]
            ck.against64(i, name, "gate.spatial_mlp.3", "w_s", out, torch.sigmoid(F.conv2d(h.double(), w.double(), b.double())), torch.sigmoid(F.conv2d(h, w, b)))
            assert torch.equal(out, self.buf(f"ws{k}", B * H * H))
        else:
            ck.report.append(f"{i:3d} {name:44s} (no rule)")

    def idc_conv(self, i, name):
        B, s = self.B, self.lat // 16
        emb = self.buf("id_emb", B * 2048).reshape(B, 2048, 1, 1)
        self.run_to(i + 1)
        w, b = self.P["denoiser.idc_conv.weight"], self.P["denoiser.idc_conv.bias"]
        rows = lambda t: t.reshape(B, 2048, s, s).permute(0, 2, 3, 1).reshape(-1)      # noqa: E731  (sub-pixel major, as the packer lays the columns out)
        out = self.op(i)
        self.ck.rel(i, name, "idc_conv", "idc", out, rows(_conv(emb, w, b)), False, lambda: rows(_conv(emb, w, b, halves=True)))
        assert torch.equal(out, self.buf("idc", out.numel()))


def prologue_scan(model, P, crl, crf, report, select=None, info=None):
    """The launches of hd_prepare(crl [B,4,L,L], crf [B,3,128,128]) for which select(name, tuple) holds (None: every launch).  Returns
    {launch kind: worst whole-tensor rel-L2 (exact kinds: differing elements)} plus "launches" (of the program) and "scanned"; info (a
    dict) receives "face" {kind: worst per-face rel-L2}, "f64" {fp32-only kind: (kernel max-abs, torch fp32 max-abs)}, "tuples"
    {launch name: (loader, epilogue, mode, affine, nt, ragged) or None} of the whole program and "scanned" (the names)."""
    info = info if info is not None else {}
    ck = _Check(report, crl.shape[0])
    sc = _Scan(model.engine, P, crl, crf, ck)
    tuples, scanned = {}, []
    try:
        for i, name in enumerate(sc.names):
            tuples[name] = t = op_tuple(sc.L, sc.ctx, i, name, sc.B, sc.lat)
            if select is not None and not select(name, t):
                continue
            if t is not None:
                report.append(f"{i:3d} {name:44s} tuple      {tuple_text(t)}")
            sc.rule(i)
            scanned.append(name)
    finally:
        sc.L.hd_debug_limit_ops(sc.ctx, 1, -1)
    ck.worst["launches"], ck.worst["scanned"] = len(sc.names), len(scanned)
    info["face"], info["f64"], info["tuples"], info["scanned"] = ck.face, ck.f64, tuples, scanned
    return ck.worst


def tuple_table(tuples):
    """{tuple text: [count, first launch name]} of the GEMM launches, idc.* and the others apart."""
    out = {}
    for name, t in tuples.items():
        if t is not None:
            e = out.setdefault(("idc " if name.startswith("idc.") else "     ") + tuple_text(t), [0, name])
            e[0] += 1
    return out


def summary(B, latent, worst, info):
    lines = [f"== latent {latent}, batch {B}: {worst['scanned']} of {worst['launches']} launches scanned",
             "worst per launch kind (whole tensor | worst face):"]
    for k in sorted(k for k in worst if k not in ("launches", "scanned")):
        lines.append(f"  {k:24s} {worst[k]:.3e}" + (f" | {info['face'][k]:.3e}" if k in info["face"] else ""))
    lines.append("fp32-only kinds, max-abs kernel / torch fp32: " + ", ".join(f"{k} {a:.2e} / {b:.2e}" for k, (a, b) in sorted(info["f64"].items())))
    lines.append("GEMM launches per tuple (count, first launch):")
    for k, (n, first) in sorted(tuple_table(info["tuples"]).items()):
        lines.append(f"  {k:58s} {n:3d}  {first}")
    return lines


def main():
    import argparse
    from hifidiff_amd import synth
    from hifidiff_amd.refiner import FacialRefiner
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--latent", type=int, default=16)
    ap.add_argument("--only", default="", help="comma-separated name prefixes to scan (default: every launch)")
    ap.add_argument("--out", default="prologue_forced.txt", help="report file")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    P = synth.refiner_state_dict(a.latent)
    m = FacialRefiner(a.latent); m.load_state_dict(P); m.to("cuda")
    _, crl, crf = synth.sample_inputs(a.batch, a.latent)
    only = tuple(s for s in a.only.split(",") if s)
    report, info = [], {}
    worst = prologue_scan(m, P, crl, crf, report, (lambda n, t: n.startswith(only)) if only else None, info)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(summary(a.batch, a.latent, worst, info) + report) + "\n")
    bad = [ln for ln in report if "<<<<<<" in ln or "no rule" in ln]
    print("\n".join(bad[:40]))
    print(f"{worst}\n{len(bad)} flagged of {len(report)} lines; report in {a.out}")


if __name__ == "__main__":
    main()
