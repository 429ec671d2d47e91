"""CoarseRestoration (hd_cr_forward), launch by launch: every one of its 175 launches against the CPU oracle on the launch's own
inputs (tools/cr_forced.py), at the bounds of the denoiser's teacher-forced scan -- 3e-4 rel-L2 for fp32 outputs, 3e-3 for
bf16-stored outputs, bit-exact for the bf16 copies and pure data movement -- with the launches that have no bf16 operand held
against float64 at 4 x torch's own fp32 error, and the LayerNorm partials every producer writes checked on their own.
test_coarse_restoration_* (test_gpu_parity.py) keep the end-to-end view.  Figures: profiles/r12_cr_ops.txt."""
import os
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def weight_sets():
    import cr_forced
    from hifidiff_amd import synth
    torch.set_grad_enabled(False)
    made = {}

    def get(which):
        if which not in made:
            made[which] = {"plain": synth.cr_state_dict, "per-face": lambda: cr_forced.per_face_state_dict(synth.cr_state_dict(wild=True)),
                           "offset": lambda: cr_forced.offset_state_dict(synth.cr_state_dict())}[which]()
        return made[which]
    return get


@pytest.fixture(scope="module")
def models(gpu, weight_sets):
    """One CoarseRestoration per weight set, made when first asked for."""
    from hifidiff_amd.cr import CoarseRestoration
    made = {}

    def get(which):
        if which not in made:
            m = CoarseRestoration()
            m.load_state_dict(weight_sets(which))
            made[which] = m.to("cuda:0")
        return made[which]
    return get


@pytest.mark.parametrize("weights,B", [("plain", 1), ("plain", 3), ("per-face", 3)])
def test_every_cr_launch_against_oracle_on_its_own_inputs(models, weight_sets, weights, B):
    """Full scan at batch 1 (64 rows at level 4, one row for the SCA GEMMs, one face for the strip kernels) and 3 (odd, 192 rows);
    the side is fixed at 128 by the network.  Every launch has a rule and is within its bound, the launch count is CR_OPS and
    every launch kind was seen.  The `per-face` set (strong warps, fc_loc.2.weight scaled per STN, faces of amplitude 1 / 30 / -30)
    must give, on the thetas read back, any two faces a difference >= 0.25 in some entry at every one of the nine STNs and
    10 % .. 60 % of the output sampled from outside the map at four STNs or more: a kernel that read `theta`, `loc1` or `loc2` of
    another face fails the grid-sample / localisation / theta rule there.
    Measured (profiles/r12_cr_ops.txt), worst rel-L2 over the three scans: conv2_gate_pool G 1.8e-4 unfused (band seams and borders included) /
    2.2e-4 strips / 2.4e-4 fused, conv4 1.4e-4 (bf16 bound); the chain's X 8.3e-5 and X'-X 2.3e-4, conv1 2.6e-5, every other GEMM launch
    <= 1.2e-5 (fp32 bound); bf16 copies, skip copy and skip add differ in 0 elements; LayerNorm partials 1.1e-7.  fp32-only launches, max-abs
    kernel / torch fp32: intro 4.2e-7 / 3.2e-7, outro 1.8e-7 / 1.6e-7, localisation convs 4.5e-8 / 5.1e-8 and 3.2e-8 / 2.8e-8, grid sample
    7.8e-6 / 7.8e-6, theta 1.1e-7 / 3.6e-8 (ratio 2.9), pool_finish 4.5e-8 / 1.5e-8 (the worst ratio, 3.0).  Per-face thetas read back: smallest
    pair difference 0.311, six STNs 18 - 58 % outside.  The per-face scan runs on faces of amplitude 1 / 30 / -30, the plain scans on the
    faces as they are."""
    import cr_forced
    report, info = [], {}
    worst = cr_forced.cr_scan(models(weights), weight_sets(weights), cr_forced.faces(B, weights == "per-face"), report, info)
    diff, n_in, per = cr_forced.theta_conditions(info["theta"])
    print(f"---- {weights} batch {B}\n" + "\n".join(report) + f"\nworst {worst}\nfp32-only kinds (kernel, torch fp32): {info['f64']}\n"
          f"max |row mean| / row std: {max(info['ratio'].values()):.2f}\nthetas: smallest pair difference {diff:.3f}, {n_in} STNs 10-60 % outside, {per}")
    if weights == "per-face":
        assert len(info["theta"]) == 9
        if not (diff >= cr_forced.THETA_MIN_DIFF and n_in >= cr_forced.OUTSIDE_MIN_STNS):
            pytest.fail(f"input error: the per-face weights do not separate the faces' thetas (smallest pair difference {diff:.3f}, wanted >= "
                        f"{cr_forced.THETA_MIN_DIFF}) or leave {n_in} < {cr_forced.OUTSIDE_MIN_STNS} STNs sampling 10-60 % outside: {per}")
    assert worst["launches"] == cr_forced.CR_OPS                # a new launch cannot go unchecked
    flagged = [ln for ln in report if "<<<<<<" in ln or "no rule" in ln]
    assert not flagged, "\n".join(flagged)
    assert set(worst) - {"launches"} == cr_forced.KINDS
    for kind, w in worst.items():
        if kind in cr_forced.EXACT_KINDS:
            assert w == 0, (kind, w)
        elif kind == "stats":
            assert w <= cr_forced.STAT_BOUND, (kind, w)
        elif kind != "launches":
            assert w <= (cr_forced.BF16_BOUND if kind.startswith("conv2_gate_pool") or kind == "conv4" else cr_forced.FP32_BOUND), (kind, w)
    for kind in cr_forced.F64_KINDS:
        err, err32 = info["f64"][kind]
        assert err <= cr_forced.F64_MARGIN * err32, (kind, err, err32)


def test_cr_debug_buffers_follow_the_workspace(models):
    """The debug names of the CR workspace belong to the batch in use: batch 1, then 3, then 1 again (the first workspace is parked
    and taken back); `X0` and `theta` read back with the sizes of the current batch, and the first and third outputs are
    bit-identical."""
    import cr_forced
    m = models("plain")
    x3 = cr_forced.faces(3)
    outs = []
    for B in (1, 3, 1):
        outs.append(m(x3[:B].cuda()).cpu())
        assert cr_forced.read_buffer(m._ctx, "X0").numel() == B * 128 * 128 * 32
        assert cr_forced.read_buffer(m._ctx, "theta").numel() == B * 6
        assert cr_forced.read_buffer(m._ctx, "skip4").numel() == B * 64 * 512
    assert torch.equal(outs[0].view(torch.int32), outs[2].view(torch.int32))
    assert torch.isfinite(outs[1]).all()


def test_cr_statistics_far_from_centred(models, weight_sets):
    """add_rows_stats_kernel forms M2 as s2 - s1 * mean in one pass.  With encoders.3.sampling.bias offset by BIAS_OFFSET the decoder
    input (middle + skip, 1 x 512 partials) has max |row mean| / row std >= 30 (read back; an input error otherwise); its mean and
    1 / sqrt(M2 / 512 + 1e-6) stay within 3e-4 of float64 and the launch that consumes the partials (the first decoder block's fused
    conv1 -> depthwise -> gate) stays within the bf16 bound.
    Measured: ratio 38.7, mean error / row std 3.1e-6, rstd relative error 1.2e-4, next launch's G 1.4e-3."""
    import cr_forced
    report = []
    mean_err, rstd_err, ratio, g_rel = cr_forced.skip_add_prefix(models("offset"), weight_sets("offset"), cr_forced.faces(3), report)
    print("\n".join(report) + f"\nmean err / row std {mean_err:.3e}, rstd rel err {rstd_err:.3e}, max |row mean| / row std {ratio:.1f}, next G rel {g_rel:.3e}")
    if not ratio >= cr_forced.RATIO_MIN:
        pytest.fail(f"input error: max |row mean| / row std at decoders.0.skip_add is {ratio:.1f} < {cr_forced.RATIO_MIN}")
    flagged = [ln for ln in report if "<<<<<<" in ln]
    assert not flagged, "\n".join(flagged)
    assert mean_err <= cr_forced.STAT_BOUND and rstd_err <= cr_forced.STAT_BOUND, (mean_err, rstd_err)
    assert g_rel <= cr_forced.BF16_BOUND, g_rel
