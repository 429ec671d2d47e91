"""The conditioning prologue (hd_prepare, launch program 1), launch by launch: every launch against the CPU oracle on the launch's
own inputs (tools/prologue_forced.py), at the bounds of the other teacher-forced scans -- 3e-4 rel-L2 for fp32 outputs, 3e-3 for
bf16-stored outputs, bit-exact for idc.input, idc.max_pool and the bf16 copies, float64 at 4 x torch's own fp32 error for the launches
without a bf16 operand, LayerNorm partials at 3e-4 -- for the whole tensor and for the rows of every single face.  The prologue's GEMM
shapes scale with the batch, so the batches are chosen by what `choose_mode` makes of them (test_scanned_batches_cover_...).
test_op_by_op_against_oracle (test_gpu_parity.py) keeps the drift view at batch 2.  Figures: profiles/r16_prologue_ops.txt."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
FULL_BATCHES = (3, 8, 32, 33)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


def make_model(weights, latent=16):
    from hifidiff_amd.refiner import FacialRefiner
    m = FacialRefiner(latent)
    m.load_state_dict(weights)
    m.to("cuda:0")
    return m


@pytest.fixture(scope="module")
def model16(gpu, weights16):
    return make_model(weights16)


@pytest.fixture(scope="module")
def inputs64():
    """cr_latent, cr_face of 64 faces, generated per face: the first n are the inputs of a batch of n."""
    from hifidiff_amd import synth
    _, crl, crf = synth.sample_inputs(64, 16)
    return crl, crf


@pytest.fixture(scope="module")
def tuples16(model16, inputs64):
    """{batch: {launch name: dispatch tuple or None}} of the real programs at latent 16, read once."""
    import prologue_forced as PF
    crl, crf = inputs64
    return {B: PF.program_tuples(model16.engine, crl[:B], crf[:B]) for B in FULL_BATCHES + (64,)}


def _assert_scan(PF, worst, info, report, kinds):
    flagged = [ln for ln in report if "<<<<<<" in ln or "no rule" in ln]
    assert not flagged, "\n".join(flagged)
    seen = set(worst) - {"launches", "scanned"}
    assert kinds <= seen, kinds - seen
    for kind in seen:
        w, f = worst[kind], info["face"].get(kind, 0.0)
        if kind in PF.EXACT_KINDS:
            assert w == 0, (kind, w)
        elif kind == "stats":
            assert w <= PF.STAT_BOUND, (kind, w)
        else:
            lim = PF.BF16_BOUND if kind in PF.BF16_KINDS else PF.FP32_BOUND
            assert w <= lim and f <= lim, (kind, w, f)
    for kind in PF.F64_KINDS:
        if kind in info["f64"]:
            err, err32 = info["f64"][kind]
            assert err <= PF.F64_MARGIN * err32, (kind, err, err32)


def _print(PF, B, latent, worst, info, report):
    print("\n".join(PF.summary(B, latent, worst, info) + report))


@pytest.mark.parametrize("B", FULL_BATCHES)
def test_every_prologue_launch_against_oracle_on_its_own_inputs(model16, weights16, inputs64, B):
    """Full scans at latent 16: batch 3 (small, odd: every ResNet GEMM on 32-row skinny tiles), 8 (the tall 128 / 64-row tiles, modes 0 / 1),
    33 (modes 2 - 6; 2112 and 528 rows at layers 3 / 4 leave ragged last tiles for the 128 / 256-row M-split workgroups) and 32 (the same
    modes with full last tiles, as batch 64 has them: without it two ResNet tuples of batch 64 occur in no scan).  The launch count is
    PROLOGUE_OPS, every launch has a rule and is within its bound for the whole tensor and for every single face, and every launch kind
    was seen.
    Measured (profiles/r16_prologue_ops.txt), worst over the four scans as whole tensor / worst single face.  bf16 bound 3e-3: fused
    conv1 -> depthwise -> gate G 2.5e-4 / 9.9e-4, conv4 2.0e-4 / 6.4e-4, the SCA launch's G * s 3.0e-5 / 1.4e-4; idc.* 1x1 1.3e-4 / 2.4e-4,
    3x3 6.5e-5 / 1.5e-4, 3x3 stride 2 7.4e-5 / 1.2e-4, 7x7 stride 2 9.2e-6 / 3.2e-5, conv3 + identity 4.9e-5 / 7.8e-5, downsample 1.4e-5 /
    3.3e-5 and 6.3e-5 / 9.1e-5 at stride 2.  fp32 bound 3e-4: the chain kernel's X 7.0e-6 / 2.0e-5 and X' - X 8.2e-5 / 2.5e-4 (the closest:
    one face of 33 at level 1), hcas.*.spatial_mlp.0 9.6e-6 / 1.3e-5, every other GEMM launch <= 7.4e-7 / 8.4e-7.  idc.input, idc.max_pool
    and every bf16 copy differ in 0 elements; LayerNorm partials 1.2e-7.  fp32-only launches, max-abs kernel / torch fp32: fpg.intro
    5.7e-7 / 4.9e-7, hcas.*.pool 1.7e-7 / 1.3e-7, hcas.*.spatial_mlp.3 4.6e-8 / 4.2e-8, idc.avgpool 9.3e-10 / 9.3e-10 (worst ratio 1.4).
    No launch exceeded a bound on a single face, so no reordering-noise comparison was needed."""
    import prologue_forced as PF
    crl, crf = inputs64
    report, info = [], {}
    worst = PF.prologue_scan(model16, weights16, crl[:B], crf[:B], report, None, info)
    _print(PF, B, 16, worst, info, report)
    assert worst["launches"] == PF.PROLOGUE_OPS[16] == worst["scanned"]     # a new launch cannot go unchecked
    _assert_scan(PF, worst, info, report, PF.KINDS_FULL16)


def test_scanned_batches_cover_the_kernels_of_the_benchmark_batch(tuples16):
    """The coverage condition on the real programs (hd_debug_op_info): every dispatch tuple (loader, epilogue, mode, xcd_tile_affine,
    w_nt, ragged last row tile) of an idc.* launch at batch 64 occurs among the idc.* launches of the full scans, and those contain
    kernel modes 0 - 6, modes 5 and 6 with a ragged last tile.  A failure means the scanned batches are the wrong ones, not that a
    kernel is."""
    idc = lambda B: {t for n, t in tuples16[B].items() if n.startswith("idc.") and t is not None}      # noqa: E731
    union = set().union(*(idc(B) for B in FULL_BATCHES))
    print("\n".join(f"batch {B}: modes {sorted({t[2] for t in idc(B)})}, {len(idc(B))} tuples" for B in FULL_BATCHES + (64,)))
    missing = idc(64) - union
    modes = {t[2] for t in union}
    ragged = {t[2] for t in union if t[5]}
    if missing or not set(range(7)) <= modes or not {5, 6} <= ragged:
        pytest.fail(f"input error: the scans at batches {FULL_BATCHES} miss ResNet tuples of batch 64 {sorted(missing)}, or modes "
                    f"{sorted(set(range(7)) - modes)}, or a ragged last tile for modes {sorted({5, 6} - ragged)}")


def test_benchmark_batch_launches_outside_resnet_and_fpg_blocks(model16, weights16, inputs64, tuples16):
    """Batch 64: the gates, fpg.downs.*, fpg.convs.* and idc_conv (mode 4 on the LK_F32 loader at hcas.4.spatial_mlp.0: 16384 rows), and
    any other launch whose dispatch tuple none of the three full scans produced.  The ResNet and FPG-block launches the coverage
    condition shows to be the same kernels are left out: the CPU oracle of 64 faces is what would take the time.
    Measured: 41 launches, the six beyond the listed ones being fpg.encoders.0.*.conv2_gate_pool (LN / DWGATE on mode 4, 3.0e-4 on the
    worst face) and fpg.encoders.2.*.conv4 (mode 3 without the XCD-affine tile map, 4.5e-4); gates, downs, convs and idc_conv as at the
    smaller batches (hcas.4.spatial_mlp.0 on mode 4: 9.3e-6 / 1.7e-5)."""
    import prologue_forced as PF
    crl, crf = inputs64
    covered = set().union(*(set(tuples16[B].values()) for B in FULL_BATCHES))
    outside = lambda n: n.startswith(("hcas.", "fpg.downs.", "fpg.convs.")) or n == "idc_conv"         # noqa: E731
    report, info = [], {}
    worst = PF.prologue_scan(model16, weights16, crl, crf, report, lambda n, t: outside(n) or (t is not None and t not in covered), info)
    _print(PF, 64, 16, worst, info, report)
    assert worst["launches"] == PF.PROLOGUE_OPS[16]
    assert {n for n in info["tuples"] if outside(n)} <= set(info["scanned"]) and worst["scanned"] >= 4 + 5 + 25 + 1
    assert info["tuples"]["hcas.4.spatial_mlp.0"][:3] == (0, 0, 4)           # LK_F32, EK_BIASF32, mode 4
    _assert_scan(PF, worst, info, report, PF.KINDS_GATES | {"down", "up", "stats", "bf16_copy"})


def test_latent32_fpg_gates_and_idc_term(gpu):
    """Latent 32, batch 3: 32 x 32 / 16 x 16 faces (the strip kernel with the static LayerNorm row, the chain kernel adding the strip sums
    up), level 2 with the row scale in conv3's loader, the gates and idc_conv with S = 2.  The ResNet shapes are those of latent 16.
    Measured: strips G 1.7e-4 / 2.4e-4, the chain's X' - X 1.2e-4 / 1.2e-4 and its pooled sums within 3e-4, sca on the bf16 pooled vector
    1.7e-7, idc_conv 1.3e-7; fpg.intro 5.5e-7 / 5.3e-7, hcas.*.pool 2.8e-7 / 1.3e-7 (ratio 2.1, the worst of all scans)."""
    import prologue_forced as PF
    from hifidiff_amd import synth
    P = synth.refiner_state_dict(32)
    m = make_model(P, 32)
    _, crl, crf = synth.sample_inputs(3, 32)
    report, info = [], {}
    worst = PF.prologue_scan(m, P, crl, crf, report, lambda n, t: not n.startswith("idc.") or n == "idc_conv", info)
    _print(PF, 3, 32, worst, info, report)
    assert worst["launches"] == PF.PROLOGUE_OPS[32] and worst["scanned"] == PF.PROLOGUE_OPS[32] - 56
    _assert_scan(PF, worst, info, report, PF.KINDS_FPG32 | PF.KINDS_GATES)


def test_pool_prepare_holds_what_the_scans_held(model16, inputs64):
    """hd_pool_prepare(n) on a batch-64 context runs the same program at batch n on a staging chain sized for 64 (stage_prologue): for
    n = 8 and 33 the entries, committed to the first n slots, equal bit for bit what hd_prepare(n) leaves in prior*, wc*, ws*, idc and
    id_emb -- the tensors the scans above held against the oracle."""
    from test_slots import BUFS, Ctx
    crl, crf = inputs64
    c = Ctx(model16)
    want = {}
    for n in (8, 33):
        c.prep(crf[:n], crl[:n])
        torch.cuda.synchronize()
        want[n] = {k: c.read(k, n) for k in BUFS}
    c.prep(crf[33:].repeat(3, 1, 1, 1)[:64], crl[33:].repeat(3, 1, 1, 1)[:64])      # other faces in every slot
    c.e.enable_pool(33)
    try:
        for n in (8, 33):
            ent = list(range(n))
            c.e.pool_prepare(ent, crl[:n].cuda(), cr_face=crf[:n].cuda())
            c.e.pool_commit(ent, ent)
            torch.cuda.synchronize()
            for k in BUFS:
                assert np.array_equal(c.read(k, 64)[:n].view(np.int32), want[n][k].view(np.int32)), (n, k)
    finally:
        c.e.disable_pool()
