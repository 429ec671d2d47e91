#!/usr/bin/env python3
"""Teacher-forced op parity: every launch of one denoiser evaluation against the CPU oracle ON THE LAUNCH'S OWN INPUTS.

The chained scan (tools/op_parity.py) compares launch i with the oracle's tap i; both sides then carry the drift of everything
before them (the bf16-operand emulation is chaotic at the level of operand rounding: DESIGN.md §2), so its bound at the deep
levels is 2e-2 and a 1-2 % kernel error would pass.  Here the state the HIP path itself has reached BEFORE launch i is read
back (hd_debug_read), the oracle's arithmetic for that one launch is applied to exactly those values on the CPU (bf16-operand
emulation: same rounding points), and the launch's output is compared with that: what is left is accumulation order and the
few rounding flips it causes.  Checks, bounds, prefix runs and the NAF block's rules: tools/forced.py; here the step's other
launches, the gated HCA input `Xg` and the stepping of the persistent stages.  Run at batch 2 and at the benchmark batch 64 (the
tile shapes differ).  Needs the program with one launch per GEMM (model created under HD_NO_XCD=1); the XCD-local persistent
stages are tied to these launches bit for bit by their own test.  (Test infrastructure: uses oracle/.)
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from forced import BF16_BOUND, FP32_BOUND, Check, LaunchIO, NafRules, PrefixRun, down_rule, naf_gemm_rows, nchw, rows, up_rule     # noqa: E402
from hifidiff_amd import _lib                                  # noqa: E402
from oracle import hifidiff_oracle as O                         # noqa: E402

PR = O.BF16
# launches of one eps evaluation in the program with one launch per GEMM: intro, 4 downs, 4 ups, 5 HCA convs, ending, 8 x 5 at the middle
# level, 16 x 5 at levels 2 / 3 and 8 blocks at levels 0 / 1 -- 2 launches each (fused conv1 or strips + the chain kernel), 4 at latent 64
# (conv1, the unfused depthwise conv, pool_finish, the chain kernel)
DENOISER_OPS = {16: 151, 32: 151, 64: 167}
GATED_LAST = {"denoiser.middle_blks.7": 0, "denoiser.decoders.0.1": 1, "denoiser.decoders.1.1": 2, "denoiser.decoders.2.1": 3, "denoiser.decoders.3.1": 4}


def level_of(name, latent):
    p = name.split(".")
    if p[1] == "encoders":
        l = int(p[2])
    elif p[1] == "middle_blks":
        l = 4
    else:
        l = 3 - int(p[2])
    return l, 128 << l, latent >> l


class _Step:
    """What the two scans share: the prepared engine, the prefix runs of one eps evaluation (state: the limits that stop one persistent
    stage), the conditioning the HIP path itself computed (its parity is the prologue scan's business) and the rules both have."""

    def __init__(self, model, P, x, crl, crf, t, report, fp32_bound, bf16_bound):
        self.e, self.P, self.x, self.B, self.latent = model.engine, P, x, x.shape[0], model.engine.latent_res
        self.ck = Check(report, None, fp32_bound, bf16_bound, 42, 8)
        self.e.prepare(crl.cuda(), cr_face=crf.cuda())
        xd = x.cuda()
        self.run = PrefixRun(self.e.ctx, lambda *limits: (self.limits(*limits), self.e.eps(xd, t)))
        self.names = self.run.names()
        self.temb = O.time_embedding(P, O.normalize_timesteps(t, self.B))
        self.idc = self.run.buf("idc")
        self.gate_c = {i: self.run.buf(f"wc{i}") for i in range(5)}
        self.gate_s = {i: self.run.buf(f"ws{i}") for i in range(5)}

    def limits(self, face_limit=0, phase_limit=0, first=-1):
        L, ctx = _lib.lib(), self.e.ctx
        _lib.check(L.hd_set_option(ctx, b"stage_limit_first", first), ctx)          # the limits stop THIS stage only
        _lib.check(L.hd_set_option(ctx, b"face_block_limit", face_limit), ctx)
        _lib.check(L.hd_set_option(ctx, b"xcd_phase_limit", phase_limit), ctx)

    def reset(self):
        self.limits()
        self.run.reset()

    def level(self, l):
        return self.B, 128 << l, self.latent >> l

    def size(self, l):
        return self.B * (128 << l) * (self.latent >> l) ** 2

    def intro(self, i, name, got):
        P = self.P
        self.ck.rel(i, name, "intro", "X0" if name == "intro" else "X", got, rows(F.conv2d(self.x, P["denoiser.intro.weight"], P["denoiser.intro.bias"], padding=1)), False)

    def down(self, i, name, l, src, got):
        down_rule(self.ck, i, name, "X", got, src, self.P[f"denoiser.downs.{l}.weight"], self.P[f"denoiser.downs.{l}.bias"])

    def up(self, i, name, k, src, skip, got):
        up_rule(self.ck, i, name, "X", got[:skip.numel()], src, self.P[f"denoiser.ups.{k}.0.weight"], skip)

    def up_source(self, hi):
        """X holds the encoder's skip, the level above its (HCA) output."""
        return nchw(self.run.buf(("Y" if self.e.conditional else "X") + str(hi)), *self.level(hi))

    def gated(self, i, name, p, l, x):
        """The gated HCA conv input a block's last launch / a stage emits, against its own fp32 output x: the gate multiply alone."""
        B, C, H = self.level(l)
        gi = GATED_LAST[p]
        add = nchw(self.idc, B, C, H) if gi == 0 else 0.0
        wc = self.gate_c[gi][:B * C].reshape(B, C, 1, 1)
        ws = self.gate_s[gi][:B * H * H].reshape(B, 1, H, H)
        self.ck.rel(i, name, "Xg", "Xg", self.run.buf(f"Xg{l}", B * H * H * C), rows(PR.q((x + add) * (1.0 + wc + ws))), True)


def forced_scan(model, P, x, crl, crf, t, report, fp32_bound=FP32_BOUND, bf16_bound=BF16_BOUND, info=None):
    """model: FacialRefiner built under HD_NO_XCD=1 (151 launches at latent 16; latent 32 / 64 have no other program).  Returns the worst
    rel-L2 over fp32 outputs and over bf16-stored outputs; report lines carry `<<<<<<` where a bound is exceeded.  info (a dict) receives
    "kinds" {launch kind: worst rel-L2} and "launches" (of the program)."""
    st = _Step(model, P, x, crl, crf, t, report, fp32_bound, bf16_bound)
    ck, run, names, B, latent = st.ck, st.run, st.names, st.B, st.latent
    naf = NafRules(P, ck)
    try:
        for i, name in enumerate(names):
            parts = name.split(".")
            kind = parts[0]
            io = LaunchIO(run, i)
            if kind == "denoiser":
                p = ".".join(parts[:-1])
                l, C, H = level_of(name, latent)
                film = O.film_vectors(P, p, st.temb)
                naf.launch(i, names, p, l, B, C, H, lambda which: (film[2 * which - 2], film[2 * which - 1]), io)
                if parts[-1] == "conv5" and st.e.conditional and p in GATED_LAST:     # the launch also emits the HCA conv's gated input
                    st.gated(i, name, p, l, nchw(io.out(), B, C, H))
            elif kind == "intro":
                st.intro(i, name, io.after("X0")[:st.size(0)])
            elif kind == "downs":
                l = int(parts[1])
                st.down(i, name, l, nchw(io.before(f"X{l}"), *st.level(l)), io.after(f"X{l + 1}")[:st.size(l + 1)])
            elif kind == "ups":
                k = int(parts[1])
                run.run_to(i)
                st.up(i, name, k, st.up_source(4 - k), nchw(run.buf(f"X{3 - k}"), *st.level(3 - k)), io.after(f"X{3 - k}"))
            elif kind == "hcas":
                l = 4 - int(parts[1])
                xg = nchw(io.before(f"Xg{l}"), *st.level(l))
                q = f"denoiser.hcas.{parts[1]}"
                want = torch.relu(O._conv_bn(xg, P, q + ".fused_mlp.0", q + ".fused_mlp.1", PR, padding=1))
                ck.rel(i, name, "hcas", "Y", io.after(f"Y{l}")[:want.numel()], rows(want), False)
            elif kind == "ending":
                src = nchw(io.before("Y0" if st.e.conditional else "X0"), B, 128, latent)
                want = F.conv2d(src, P["denoiser.ending.weight"], P["denoiser.ending.bias"], padding=1)
                ck.rel(i, name, "ending", "eps", io.after("eps")[:want.numel()], want, False)
            else:
                ck.no_rule(i, name)
    finally:
        st.reset()
    if info is not None:
        info["kinds"], info["launches"] = ck.worst, len(names)
    return ck.stored


def denoiser_gemm_rows(name, B, latent):
    """Rows M of the GEMM launch `name` of the denoiser program at batch B (None: the intro / ending convs, which are no GEMMs)."""
    lv = lambda l: B * (latent >> l) ** 2                       # noqa: E731
    p = name.split(".")
    if p[0] == "denoiser":
        return naf_gemm_rows(p[-1], B, level_of(name, latent)[2])
    if p[0] == "downs":
        return lv(int(p[1]) + 1)
    if p[0] in ("ups", "hcas"):                                  # the up conv's rows are those of its input, the level above
        return lv(4 - int(p[1]))
    return None


def stage_forced_scan(model, P, x, crl, crf, t, report, fp32_bound=FP32_BOUND, bf16_bound=BF16_BOUND):
    """The persistent stages of the DEFAULT program (59 launches at latent 16, batch <= 64: hd_face.hpp levels 0 / 1, hd_xcd.hpp /
    hd_xcd2.hpp levels 2 / 3), block by block: the stage is stopped after b blocks (`face_block_limit` / `xcd_phase_limit`
    = 5 b), the residual stream it has reached is read back, the oracle's arithmetic for block b + 1 alone
    (conditional_naf.py:108-136, bf16-operand emulation) is applied to exactly those values and compared with what the stage
    holds after b + 1 blocks.  The stages therefore need not share a single bit with the per-GEMM launches.  At the end of a
    stage the bf16 copy / the gated HCA input it emits are checked against the stage's own fp32 output."""
    st = _Step(model, P, x, crl, crf, t, report, fp32_bound, bf16_bound)
    ck, run, names, B, latent = st.ck, st.run, st.names, st.B, st.latent
    n, nstages = len(names), 0
    enc_blocks = [2, 2, 4, 8]
    try:
        for i, name in enumerate(names):
            parts = name.split(".")
            if parts[0] != "denoiser" or parts[-1] != "conv5" or parts[1] == "middle_blks":
                continue
            if i > 0 and names[i - 1].startswith(".".join(parts[:-1]) + "."):
                continue                                              # a per-GEMM conv5 launch, not a stage
            l, C, H = level_of(name, latent)
            M = B * H * H
            nblk = enc_blocks[l] if parts[1] == "encoders" else 2
            assert int(parts[3]) == nblk - 1, name
            grp = ".".join(parts[:3])
            first = sum(enc_blocks[:l]) if parts[1] == "encoders" else 16 + 8 + 2 * int(parts[2])     # index of the stage's first block
            nstages += 1
            # the launch that produces this stage's input: its own op, or -- folded -- the stage's ENTRY (intro conv at level 0, the down conv of
            # level 0 at level 1): the stage run with NO block (face_block_limit < 0) then leaves the entry's x, which is held against the
            # oracle's arithmetic for that conv on ITS inputs
            producer = ("intro" if l == 0 else f"downs.{l - 1}") if parts[1] == "encoders" else f"ups.{parts[2]}"
            run.run_to(i)
            if (names[i - 1] if i > 0 else "") != producer:
                entry = producer + " (stage entry)"
                if producer.startswith("downs"):
                    src0 = nchw(run.buf(f"X{l - 1}"), *st.level(l - 1))
                elif producer.startswith("ups"):
                    src0, skip0 = st.up_source(l + 1), nchw(run.buf(f"X{l}"), B, C, H)
                run.run_to(i + 1, -1, 0, first)
                got = run.buf(f"X{l}", M * C)
                if producer == "intro":
                    st.intro(i, entry, got)
                elif producer.startswith("downs"):
                    st.down(i, entry, l - 1, src0, got)
                else:
                    st.up(i, entry, int(parts[2]), src0, skip0, got)
                cur = nchw(got, B, C, H)
            else:
                cur = nchw(run.buf(f"X{l}"), B, C, H)
            for b in range(nblk):
                p = f"{grp}.{b}"
                want = O.cond_naf_block(P, p, cur, st.temb, prec=PR)
                lim = 0 if b == nblk - 1 else b + 1
                run.run_to(i + 1, lim, 5 * lim, first)
                got = run.buf(f"X{l}", M * C)
                ck.rel(i, p + " (stage)", "stage", "X", got, rows(want), False)
                # the block's own contribution x' - x (the residual carries most of the norm of x'): passes through the bf16-stored
                # gate tiles, hence the bf16 bound
                ck.rel(i, p + " (stage)", "stage", "X'-X", got - rows(cur), rows(want - cur), True)
                cur = nchw(got, B, C, H)
            # exit copies of the whole stage
            if st.e.conditional and f"{grp}.{nblk - 1}" in GATED_LAST:
                st.gated(i, name, f"{grp}.{nblk - 1}", l, cur)
            else:
                ck.rel(i, name, "Xb", "Xb", run.buf(f"Xb{l}", M * C), rows(PR.q(cur)), True)
        # the step's last launch when it is the last HCA conv + the ending conv in one (hd_end.hpp): on ITS input, the gated decoder output
        if names[-1] == "ending" and st.e.conditional and (n < 2 or names[-2] != "hcas.4"):
            run.run_to(n - 1)
            xg = nchw(run.buf("Xg0"), B, 128, latent)
            run.run_to(n)
            q = "denoiser.hcas.4"
            y0 = torch.relu(O._conv_bn(xg, P, q + ".fused_mlp.0", q + ".fused_mlp.1", PR, padding=1))
            want = F.conv2d(y0, P["denoiser.ending.weight"], P["denoiser.ending.bias"], padding=1)
            ck.rel(n - 1, "hcas.4 + ending (one launch)", "ending", "eps", run.buf("eps", want.numel()), want, False)
    finally:
        st.reset()
    return dict(ck.stored, stages=nstages)


def main():
    import argparse
    from hifidiff_amd import synth
    from hifidiff_amd.refiner import FacialRefiner
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--latent", type=int, default=16)
    ap.add_argument("--t", type=float, default=500.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "op_forced.txt"))
    ap.add_argument("--stages", action="store_true", help="the persistent stages of the default program, block by block (stage_forced_scan)")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    P = synth.refiner_state_dict(a.latent)
    if not a.stages:
        os.environ["HD_NO_XCD"] = "1"
    m = FacialRefiner(a.latent); m.load_state_dict(P); m.to("cuda")
    x, crl, crf = synth.sample_inputs(a.batch, a.latent)
    report = []
    worst = (stage_forced_scan if a.stages else forced_scan)(m, P, x, crl, crf, a.t, report)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"teacher-forced {'stage (block by block)' if a.stages else 'op'} parity, batch {a.batch}, latent {a.latent}, t {a.t}: worst fp32 {worst['fp32']:.3e}, worst bf16-stored {worst['bf16']:.3e}\n")
        f.write("\n".join(report) + "\n")
    bad = [r for r in report if "<<<<<<" in r or "no rule" in r]
    print("\n".join(bad[:40]))
    print(f"worst fp32 {worst['fp32']:.3e}  worst bf16-stored {worst['bf16']:.3e}; {len(bad)} flagged of {len(report)} checks; report in {a.out}")


if __name__ == "__main__":
    main()
