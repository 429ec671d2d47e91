#!/usr/bin/env python3
"""Teacher-forced parity of the conditioning prologue (hd_prepare, launch program 1: FPG, ResNet-50, HCA gates, idc_conv): every
launch against the CPU oracle ON THE LAUNCH'S OWN INPUTS.

Checks, bounds, the prefix runs and the rules of the FPG's NAF blocks (the LayerNorm affine is the static FiLM row, scale = shift = 0:
the plain block) and down / up convs: tools/forced.py.  What launch i reads is read back after launches 0 .. i - 1 -- named buffers
(the level buffers, `prior*`, `id_emb`) and, for the rotating ResNet buffers and the gate temporaries, the output of the producing
launch (intact while its consumer is next).  Here: the ResNet-50 table (every idc.* conv against the oracle's BN-folded, bf16-rounded
conv, bf16-stored: <= 3e-3; idc.input (layout + bf16 rounding) and idc.max_pool (a max of bf16 values) differ in 0 elements), the HCA
gates and idc_conv (fp32 outputs: <= 3e-4), and what has no bf16 operand (fpg.intro, hcas.*.pool, hcas.*.spatial_mlp.3, idc.avgpool)
against float64.  Every rel-L2 is also taken PER FACE (Check with the batch).
For every GEMM launch the dispatch tuple (loader, epilogue, mode, xcd_tile_affine, w_nt, M % tile rows != 0) is read with
hd_debug_op_info and recorded.  (Test infrastructure: uses oracle/.)
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from forced import (BF16_BOUND, F64_MARGIN, FP32_BOUND, STAT_BOUND, Check, LaunchIO, NafRules, PrefixRun, conv, down_rule, intro_rule,      # noqa: E402,F401
                    naf_gemm_rows, nchw, op_names, q, rows, up_rule)
from hifidiff_amd import _lib                                  # noqa: E402
from oracle import hifidiff_oracle as O                         # noqa: E402

PR = O.BF16
# FPG 1 + 4 x 2 + 12 x 5 + 4 + 5, ResNet-50 56, gates 5 x 5, idc_conv.  Latent 64: the four blocks of levels 0 / 1 (64 x 64 and 32 x 32 faces)
# take the unfused depthwise path, conv1 / conv2_gate_pool / pool_finish / the chain kernel: 4 x 4 launches instead of 4 x 2
PROLOGUE_OPS = {16: 160, 32: 160, 64: 168}
LOADERS = ("F32", "LN", "BF16", "BF16S", "CONV_F32", "CONV_F32G", "CONV_BF16")
EPILOGUES = ("BIASF32", "RESID", "GATE", "PIXSHUF", "BIASBF16", "DWGATE", "SCA")
TILE_ROWS = {0: 128, 1: 64, 2: 64, 3: 32, 4: 32, 5: 128, 6: 256}
F64_KINDS = ("fpg.intro", "gate.pool", "gate.spatial_mlp.3", "idc.avgpool", "pool_finish")
EXACT_KINDS = ("bf16_copy", "idc.input", "idc.max_pool")
BF16_KINDS = ("conv2_gate_pool.fused", "conv2_gate_pool.strips", "conv2_gate_pool.unfused", "sca.scale_G", "conv4", "idc.conv7x7", "idc.1x1", "idc.3x3", "idc.3x3s2",
              "idc.downsample", "idc.downsample.s2", "idc.conv3")
KINDS_GATES = {"gate.pool", "gate.channel_mlp.0", "gate.channel_mlp.2", "gate.spatial_mlp.0", "gate.spatial_mlp.3", "idc_conv"}
KINDS_FPG16 = {"fpg.intro", "conv2_gate_pool.fused", "conv5.chain", "sca.prescale", "sca.scale_G", "conv3", "conv4", "conv5", "down", "up", "stats", "bf16_copy"}
KINDS_FPG32 = KINDS_FPG16 | {"conv2_gate_pool.strips", "sca.bf16"}            # 32 x 32 / 16 x 16 faces by strips, level 2 with the row scale in conv3's loader
# latent 64: levels 0 / 1 unfused (64 x 64 / 32 x 32 faces), levels 2 / 3 (256 / 64 pixels per face) with the row scale in conv3's loader: no level of the FPG
# has few enough pixels for the SCA launch to rescale G
KINDS_FPG64 = (KINDS_FPG16 - {"sca.prescale", "sca.scale_G"}) | {"conv1", "conv2_gate_pool.unfused", "pool_finish", "sca.bf16"}
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
        return naf_gemm_rows(p[4], B, latent >> int(p[2]))
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
    tile = TILE_ROWS.get(t[2] & 15)
    return t + (int(tile is not None and gemm_rows(name, B, latent) % tile != 0),)


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
    return {n: op_tuple(L, engine.ctx, i, n, B, engine.latent_res) for i, n in enumerate(op_names(engine.ctx, 1))}


def _folded(P, cv, bn):
    """conv -> BatchNorm(eval) folded as O._conv_bn does in emulation mode (fp32, before rounding)."""
    s, o = O._bn_affine(P, bn)
    b = P.get(cv + ".bias")
    return P[cv + ".weight"] * s.view(-1, 1, 1, 1), (o if b is None else b * s + o)


class _Scan:
    def __init__(self, engine, P, crl, crf, ck):
        self.L, self.ctx, self.P, self.ck = _lib.lib(), engine.ctx, P, ck
        self.B, self.lat, self.crl, self.crf = crl.shape[0], engine.latent_res, crl, crf
        crl_d, crf_d = crl.cuda(), crf.cuda()
        self.run = PrefixRun(self.ctx, lambda: engine.prepare(crl_d, cr_face=crf_d), 1)
        self.run_to, self.buf = self.run.run_to, self.run.buf
        self.run_to(0)                                          # builds the program for this batch
        self.names = self.run.names()
        self.index = {n: i for i, n in enumerate(self.names)}
        self.res = self._resnet_table()
        self.naf = NafRules(P, ck, extras=True, own_t1=True)

    def op(self, which):
        """The output of a launch, by index or name: the rotating ResNet buffers and the gate temporaries have no name of their own, the
        output is intact while its consumer is next."""
        return self.run.op(which if isinstance(which, int) else self.index[which])

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

    # ---- the rules ----
    def rule(self, i):
        name = self.names[i]
        p = name.split(".")
        self.run_to(i)
        if name == "fpg.intro":
            self.intro(i, name)
        elif p[0] == "fpg" and p[1] == "encoders":              # the LayerNorm affine is the FiLM row (scale = shift = 0): the plain block
            l = int(p[2])
            self.naf.launch(i, self.names, ".".join(p[:4]), l, self.B, 128 << l, self.lat >> l, None, LaunchIO(self.run, i))
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
            self.ck.no_rule(i, name)

    def intro(self, i, name):
        self.run_to(i + 1)
        out = self.op(i)
        intro_rule(self.ck, i, name, "fpg.intro", "X0", out, self.crl, self.P["fpg.intro.weight"], self.P["fpg.intro.bias"])
        self.ck.copy_and_stats(i, name, self.buf, 0, "x", out, 128, 1, 128)

    def down(self, i, name, l):
        B, C, H = self.B, 128 << l, self.lat >> l
        xb = nchw(self.buf(f"Xb{l}"), B, C, H)                  # gathers the bf16 copy conv5 wrote
        self.run_to(i + 1)
        out = self.op(i)
        down_rule(self.ck, i, name, f"X{l + 1}", out, xb, self.P[f"fpg.downs.{l}.weight"], self.P[f"fpg.downs.{l}.bias"])
        self.ck.copy_and_stats(i, name, self.buf, l + 1, "x", out, 2 * C, 2 * C // 32, 32)

    def up(self, i, name, k):
        """fpg.convs.k: 1x1 conv, PixelShuffle(2) and the encoder skip (k = 0: no shuffle, no skip) -> prior k."""
        B = self.B
        hi = 4 if k == 0 else 5 - k
        src = nchw(self.buf("X4" if k == 0 else f"prior{k - 1}"), B, 128 << hi, self.lat >> hi)
        skip = None if k == 0 else nchw(self.buf(f"X{4 - k}"), B, 128 << (4 - k), self.lat >> (4 - k))
        self.run_to(i + 1)
        out = self.op(i)
        up_rule(self.ck, i, name, f"prior{k}", out, src, self.P[f"fpg.convs.{k}.0.weight"], skip, 2 if k else 1, "P-skip")
        assert torch.equal(out, self.buf(f"prior{k}", out.numel()))          # the named buffer is the launch's output

    def resconv(self, i, name):
        B = self.B
        src, cin, Hin, cout, Hout, k, st, pad, cv, bn, idn, relu, kind = self.res[name]
        x = self.op(src)
        x = x.reshape(B, 128, 128, 8)[..., :3].permute(0, 3, 1, 2).contiguous() if name == "idc.conv1" else nchw(x, B, cin, Hin)
        identity = nchw(self.op(idn), B, cout, Hout) if idn else 0.0
        self.run_to(i + 1)
        w, b = _folded(self.P, cv, bn)

        def want(halves=False):
            y = conv(x, w, b, stride=st, padding=pad, halves=halves) + identity
            return rows(PR.q(torch.relu(y) if relu else y))
        self.ck.rel(i, name, kind, "out", self.op(i), want(), True, lambda: want(True))

    def resnet_other(self, i, name):
        B = self.B
        if name == "idc.input":
            self.run_to(i + 1)
            want = torch.zeros(B, 128, 128, 8)
            want[..., :3] = q(self.crf.permute(0, 2, 3, 1))
            self.ck.exact(i, name, "idc.input", "face8", self.op(i), want.reshape(-1))
        elif name == "idc.max_pool":
            x = nchw(self.op("idc.conv1"), B, 64, 64)
            self.run_to(i + 1)
            self.ck.exact(i, name, "idc.max_pool", "out", self.op(i), rows(F.max_pool2d(x, 3, 2, 1)))
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
            ck.rel(i, name, "gate." + leaf, "out", out, act(conv(x, w, b)), False, lambda: act(conv(x, w, b, halves=True)))
            if leaf == "channel_mlp.2":
                assert torch.equal(out, self.buf(f"wc{k}", B * C))
        elif leaf == "spatial_mlp.0":
            pr = nchw(self.buf(f"prior{k}"), B, C, H)
            self.run_to(i + 1)
            w, b = _folded(P, q + ".spatial_mlp.0", q + ".spatial_mlp.1")
            ck.rel(i, name, "gate.spatial_mlp.0", "out", self.op(i)[:B * H * H * (C // 2)], rows(torch.relu(conv(pr, w, b))), False,
                   lambda: rows(torch.relu(conv(pr, w, b, halves=True))))
        elif leaf == "spatial_mlp.3":
            h = nchw(self.op(n + ".spatial_mlp.0"), B, C // 2, H)
            self.run_to(i + 1)
            w, b = _folded(P, q + ".spatial_mlp.3", q + ".spatial_mlp.4")       # an fp32 VALU kernel on the folded weights (O._conv_bn, gemm=False)
            out = self.op(i)[:B * H * H]
            ck.against64(i, name, "gate.spatial_mlp.3", "w_s", out, torch.sigmoid(F.conv2d(h.double(), w.double(), b.double())), torch.sigmoid(F.conv2d(h, w, b)))
            assert torch.equal(out, self.buf(f"ws{k}", B * H * H))
        else:
            ck.no_rule(i, name)

    def idc_conv(self, i, name):
        B, s = self.B, self.lat // 16
        emb = self.buf("id_emb", B * 2048).reshape(B, 2048, 1, 1)
        self.run_to(i + 1)
        w, b = self.P["denoiser.idc_conv.weight"], self.P["denoiser.idc_conv.bias"]
        rows = lambda t: t.reshape(B, 2048, s, s).permute(0, 2, 3, 1).reshape(-1)      # noqa: E731  (sub-pixel major, as the packer lays the columns out)
        out = self.op(i)
        self.ck.rel(i, name, "idc_conv", "idc", out, rows(conv(emb, w, b)), False, lambda: rows(conv(emb, w, b, halves=True)))
        assert torch.equal(out, self.buf("idc", out.numel()))


def prologue_scan(model, P, crl, crf, report, select=None, info=None):
    """The launches of hd_prepare(crl [B,4,L,L], crf [B,3,128,128]) for which select(name, tuple) holds (None: every launch).  Returns
    {launch kind: worst whole-tensor rel-L2 (exact kinds: differing elements)} plus "launches" (of the program) and "scanned"; info (a
    dict) receives "face" {kind: worst per-face rel-L2}, "f64" {fp32-only kind: (kernel max-abs, torch fp32 max-abs)}, "tuples"
    {launch name: (loader, epilogue, mode, affine, nt, ragged) or None} of the whole program and "scanned" (the names)."""
    info = info if info is not None else {}
    ck = Check(report, crl.shape[0])
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
        sc.run.reset()
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
