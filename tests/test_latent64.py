"""Latent 64 (64 -> 512 px, FacialRefiner(64)): the (channels, side) pairs no latent-16 or latent-32 test reaches -- the unfused depthwise
path at 128 x 64 x 64 and 256 x 32 x 32 behind the chain kernel, the fused conv1 -> depthwise -> gate epilogue at 256 pixels per face with
C = 512 (64 with C = 1024, 16 with C = 2048), the gather form of the HCA conv at all five levels, the ending conv on 4096-pixel faces,
idc_conv with 16 sub-pixels (2048 -> 32768), the FPG at twice the side, guided_update_kernel at its LDS maximum (48 KB).  The persistent
stages are tied to the latent-16 geometry, so the default program is the one with a launch per GEMM (167 launches per eps, 168 in the
prologue: levels 0 / 1 take four launches per block instead of two).

One model for the module, at batches 1, 2 and 3; the weights are the latent-16 ones plus idc_conv.  Every bound is the one the same
comparison carries at latent 16 / 32 (named at each test); the figures are those of profiles/r19_latent64.txt."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, psnr, psnr_pp, rel_l2, weights16  # noqa: F401  (weights16: session fixture)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
L64 = 64


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def weights64(weights16):
    from hifidiff_amd import synth
    return synth.refiner_state_dict(L64, reuse=(weights16, 16))


@pytest.fixture(scope="module")
def model64(gpu, weights64):
    from test_mask import free, make_model
    m = make_model(weights64, L64)
    yield m
    free(m)


@pytest.fixture(scope="module")
def inputs3():
    """(x, cr_latent, cr_face) of three faces, generated per face: the first n are the inputs of a batch of n."""
    from hifidiff_amd import synth
    return synth.sample_inputs(3, L64)


@pytest.fixture(scope="module")
def cond3(weights64, inputs3):
    """The bf16-emulating oracle's conditioning of the three faces, computed once."""
    from oracle import hifidiff_oracle as O
    _, crl, crf = inputs3
    return O.Conditioning(weights64, crl, crf, prec=O.BF16)


@pytest.fixture(scope="module")
def cond2(weights64, inputs3):
    from oracle import hifidiff_oracle as O
    _, crl, crf = inputs3
    return O.Conditioning(weights64, crl[:2], crf[:2], prec=O.BF16)


def _eps(m, x, t, crf, crl):
    t = t.cuda() if torch.is_tensor(t) else t
    return m(x.cuda(), t, crf.cuda(), crl.cuda()).sample.cpu()


# ------------------------------------------------------------------------------------------------ a. eps against the emulating oracle
def test_eps_at_batch_3_against_oracle(model64, weights64, inputs3, cond3):
    """Three faces (odd: 48 rows at the middle level) against the bf16-emulating oracle at t in {999, 500, 0} for all faces and with a
    timestep per face (the LdF32LNFace kernels at these shapes): rel-L2 <= 6e-3, worst single face <= 8e-3, as
    test_eps_at_the_benchmark_batch_against_oracle; face 0 alone against face 0 of the batch <= 6e-3, as test_ragged_batches_against_oracle;
    a repeated evaluation is bit-identical.
    Measured: 2.21e-3 / 2.19e-3 / 2.22e-3 at t = 999 / 500 / 0 (worst face 2.24e-3), per-face timesteps 2.21e-3 (worst face 2.22e-3); face 0
    alone against face 0 of the batch 2.20e-3 (other tile shapes at a third of the rows: as far apart as either is from the oracle)."""
    from oracle import hifidiff_oracle as O
    x, crl, crf = inputs3
    cases = [(t, t) for t in (999, 500, 0)] + [("per face", torch.tensor([980.0, 37.0, 500.0]))]
    batch = {}
    for name, t in cases:
        ref = O.fused_denoiser(weights64, x, t, cond=cond3, prec=O.BF16)
        e = _eps(model64, x, t, crf, crl)
        r, rf = rel_l2(e, ref), max(rel_l2(e[f], ref[f]) for f in range(3))
        print(f"latent 64, batch 3, t = {name}: rel-L2 vs emulating oracle {r:.3e}, worst face {rf:.3e}")
        assert bool(torch.isfinite(e).all()) and r <= 6e-3 and rf <= 8e-3, (name, r, rf)
        assert torch.equal(_eps(model64, x, t, crf, crl), e), name            # replays are bit-identical
        batch[name] = e
    e1 = _eps(model64, x[:1], 500, crf[:1], crl[:1])
    r1 = rel_l2(e1, batch[500][:1])
    print(f"latent 64, face 0 alone against face 0 of the batch of 3: rel-L2 {r1:.3e}")
    assert r1 <= 6e-3, r1
    assert torch.equal(_eps(model64, x[:1], 500, crf[:1], crl[:1]), e1)
    model64.check()


# ------------------------------------------------------------------------------------------------ b. against the reference goldens
def test_eps_and_ddim_against_reference_goldens(model64, inputs3):
    """One face against the reference's own outputs (oracle/make_golden.py --only l64): eps at t = 500 rel-L2 <= 1e-2; the first 5 steps of
    the 50-step DDIM (eta 0, clip 3.0), graph-replayed, rel-L2 <= 3e-2 and >= 40 dB on the golden's peak-to-peak -- the bounds of
    test_latent32_against_reference_golden.  Measured: eps 3.16e-3; DDIM 4.99e-3, 58.4 dB."""
    from hifidiff_amd import sampling, schedulers
    x, crl, crf = (t[:1] for t in inputs3)
    e = _eps(model64, x, torch.full((1,), 500), crf, crl)
    r = rel_l2(e, golden("refiner_eps_L64.npz")["eps_t500"])
    print(f"latent 64, batch 1, eps t = 500 vs reference golden: rel-L2 {r:.3e}")
    assert r <= 1e-2, r
    sch = schedulers.DDIMScheduler(clip_sample_range=3.0)
    sch.set_timesteps(50)
    sch.timesteps = sch.timesteps[:5]
    lat = sampling.sample(model64, x.cuda(), crf.cuda(), crl.cuda(), sch).cpu()
    g5 = golden("ddim50_first5_L64.npz")["final"]
    r5, p5 = rel_l2(lat, g5), psnr_pp(lat, g5)
    print(f"latent 64, batch 1, first 5 of 50 DDIM steps vs reference golden: rel-L2 {r5:.3e}, PSNR {p5:.1f} dB on the golden's peak-to-peak")
    assert r5 <= 3e-2 and p5 >= 40.0, (r5, p5)


# ------------------------------------------------------------------------------------------------ c. every denoiser launch on its own inputs
@pytest.mark.parametrize("B", [1, 3])
def test_every_denoiser_launch_against_oracle_on_its_own_inputs(model64, weights64, inputs3, B):
    """tools/op_forced.py at latent 64: each of the 167 launches of one eps evaluation against the oracle's arithmetic for that launch on
    the values the HIP path itself had reached before it; fp32 outputs <= 3e-4, bf16-stored outputs <= 3e-3 (test_teacher_forced_op_parity).
    Every launch has a rule and a report line, so a new launch cannot go unchecked.
    Measured, worst fp32 / bf16-stored: batch 1 3.3e-5 / 4.2e-4, batch 3 2.2e-5 / 2.8e-4 (both the fused conv1 -> depthwise -> gate G; the
    unfused depthwise G 1.8e-4, conv4 2.2e-4, the HCA gather convs 1.0e-5, the chain kernel 1.2e-5, pool_finish 4.2e-6)."""
    import op_forced
    from hifidiff_amd import _lib
    x, crl, crf = (t[:B] for t in inputs3)
    rep = []
    worst = op_forced.forced_scan(model64, weights64, x, crl, crf, 500.0, rep)
    print("\n".join(rep))
    print(f"latent 64, batch {B}: worst fp32 {worst['fp32']:.3e}, worst bf16-stored {worst['bf16']:.3e}, {len(rep)} lines")
    n = _lib.lib().hd_num_ops(model64.engine.ctx, 0)
    assert n == op_forced.DENOISER_OPS[L64], n
    assert {int(r[:3]) for r in rep} == set(range(n))                          # every launch left at least one line
    assert not [r for r in rep if "no rule" in r], [r for r in rep if "no rule" in r][:3]
    assert not [r for r in rep if "<<<<<<" in r], [r for r in rep if "<<<<<<" in r][:8]
    assert worst["fp32"] <= 3e-4 and worst["bf16"] <= 3e-3, (B, worst)


# ------------------------------------------------------------------------------------------------ d. the prologue's FPG / gate / idc_conv launches
@pytest.mark.parametrize("B", [1, 3])
def test_prologue_fpg_gates_and_idc_term_on_their_own_inputs(model64, weights64, inputs3, B):
    """tools/prologue_forced.py at latent 64, everything but the idc.* ResNet launches (they read the 128-px cr_face at every latent size and
    are scanned at latent 16): the FPG with its levels 0 / 1 in the unfused form on their own T1 (band seams and borders, pool_finish against
    float64), levels 2 / 3 fused with the row scale in conv3's loader, the prior up-convs (PixelShuffle) at sides 4 .. 32, the gates and
    idc_conv with 16 sub-pixels.  Asserted by test_prologue_ops._assert_scan: whole tensor and worst single face.
    Measured, worst of both batches (whole tensor | worst face): unfused G 5.6e-5 | 7.6e-5, fused G 2.3e-4 | 3.7e-4, conv4 1.8e-4 | 2.0e-4,
    the chain kernel 7.8e-5 | 8.5e-5, conv1's T1 3.6e-5 | 3.7e-5, hcas.*.spatial_mlp.0 9.7e-6 | 1.0e-5, up 1.8e-7, down 2.0e-7, idc_conv
    1.8e-7, LayerNorm partials 1.2e-7, bf16 copies 0 elements; fp32-only launches, max-abs kernel / torch fp32: fpg.intro 7.0e-7 / 5.8e-7,
    pool_finish 1.3e-8 / 1.1e-8, hcas.*.pool 7.8e-8 / 4.1e-8.  This scan found hcas.4.pool (4096 pixels per face) over the float64 bound at
    batch 3, 4.67e-7 / 1.16e-7 = 4.03 x torch's error against 4: pool_avgmax_kernel kept one running sum; it now adds runs of 256 pixels."""
    import prologue_forced as PF
    from test_prologue_ops import _assert_scan
    _, crl, crf = (t[:B] for t in inputs3)
    report, info = [], {}
    worst = PF.prologue_scan(model64, weights64, crl, crf, report, lambda n, t: not n.startswith("idc.") or n == "idc_conv", info)
    print("\n".join(PF.summary(B, L64, worst, info) + report))
    assert worst["launches"] == PF.PROLOGUE_OPS[L64] and worst["scanned"] == PF.PROLOGUE_OPS[L64] - 56, worst
    assert {int(r[:3]) for r in report} >= {i for i, n in enumerate(info["tuples"]) if n in info["scanned"]}
    _assert_scan(PF, worst, info, report, PF.KINDS_FPG64 | PF.KINDS_GATES)


# ------------------------------------------------------------------------------------------------ e. the graph-replayed loop
def _oracle_loop64(P, cond, x, ts, coef):
    """The oracle's network (bf16 emulation) inside the float64 update of the table's rows."""
    from oracle import hifidiff_oracle as O
    from test_multistep import _update64
    xr, h = x.double(), None
    for i, t in enumerate(ts.tolist()):
        eps = O.fused_denoiser(P, xr.float(), torch.full((x.shape[0],), int(t)), prec=O.BF16, cond=cond).double()
        xr, h = _update64(xr, eps, coef[i].tolist() + [0.0] * (8 - coef.shape[1]), h)
    return xr


@pytest.mark.parametrize("kind,n", [("ddim", 50), ("dpm", 10)])
def test_graph_replayed_loop_against_eager_loop_and_oracle(model64, weights64, inputs3, cond2, kind, n):
    """Batch 2, the first 5 rows of the 50-step DDIM (clip 3.0) and of the 10-step DPM-Solver++ 2M table: the graph-replayed loop against
    one model(...) + scheduler.step(...) per iteration at >= 50 dB (test_multistep.py::test_eager_loop_against_graph), against the oracle's
    network inside the float64 update at rel-L2 <= 2e-2 (the *_against_the_oracle_network tests), and bit-identical when repeated.
    Measured: the eager loop gives the graph-replayed latents bit for bit in both (the program with a launch per GEMM is the only one at
    this size, and the ending launch's update is the scheduler step's arithmetic); oracle-network loop DDIM 4.0e-3, DPM 6.0e-4."""
    from test_mask import Runner, _tables
    x, crl, crf = (t[:2] for t in inputs3)
    run = Runner(model64, crf, crl)
    s, ts, coef = _tables(kind, n)
    graph = run.full(x, ts[:5], coef[:5])
    assert bool(torch.isfinite(graph).all())
    assert torch.equal(run.full(x, ts[:5], coef[:5]), graph)
    xe, crfd, crld = x.cuda(), crf.cuda(), crl.cuda()
    s.set_timesteps(n)                                                         # the scheduler's own history starts here
    for t in s.timesteps[:5]:
        xe = s.step(model64(xe, int(t), crfd, crld).sample, t, xe).prev_sample
    pe = psnr(xe.cpu(), graph)
    want = _oracle_loop64(weights64, cond2, x, ts[:5], coef[:5])
    ro = rel_l2(graph, want)
    print(f"latent 64, batch 2, first 5 rows of {kind}-{n}: eager loop {pe:.1f} dB, rel-L2 vs the oracle-network loop {ro:.3e}")
    assert pe >= 50.0, pe
    assert ro <= 2e-2, ro


def test_per_face_start_rows_against_the_tail_schedules(model64, inputs3):
    """The per-face form (hd_sample_rows) with rows = (0, 3) on the first 5 rows of DDIM-50: each face bit for bit what hd_sample gives on
    the tail of the schedule from its row, as test_start_rows.py::test_staggered_starts_against_the_tail_schedules."""
    from test_mask import Runner, _tables
    from test_start_rows import _check_staggered
    x, crl, crf = (t[:2] for t in inputs3)
    run = Runner(model64, crf, crl)
    _, ts, coef = _tables("ddim", 50)
    got = _check_staggered(run, x, ts[:5], coef[:5], [0, 3])
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, x.float())


# ------------------------------------------------------------------------------------------------ f. one row of the step, float64 formula
@pytest.fixture(scope="module")
def run2(model64, inputs3):
    """Batch 2 through the C-ABI calls (tests/test_guide.py's runner); guidance is switched on by the tests that need it."""
    from test_guide import GRunner
    _, crl, crf = (t[:2] for t in inputs3)
    return GRunner(model64, crf, crl)


def _prepared(run, inputs3):
    _, crl, crf = (t[:2] for t in inputs3)
    run.m.prepare(crf.cuda(), crl.cuda())                                      # another test of the module may have prepared another batch
    return inputs3[0][:2], crl


def test_one_unguided_row_against_the_float64_formula(run2, inputs3):
    """The plain update on the device's own eps, 4096-pixel planes: DDIM row 20 of 50 (clip 3.0), and DPM-Solver++ 2M row 5 of 20 resumed
    after five rows (the history term c7 * h, h read from the device) from a latent whose own x0 has the magnitude of a real one
    (test_guide._settled_latent), max abs <= BLEND_TOL.  Measured: DDIM 2.2e-7, DPM 2.4e-7 (history 1.3e-7, max |x0| 2.42)."""
    from test_guide import _settled_latent, _shape
    from test_mask import BLEND_TOL, _tables
    from test_multistep import _update64
    x, crl = _prepared(run2, inputs3)
    _, ts, coef = _tables("ddim", 50)
    got = run2.rows(x, ts, coef, [20, 20], 1)
    want, _ = _update64(x.double(), run2.read("eps", _shape(x)).double(), coef[20].tolist() + [0.0], None)
    err = float((got.double() - want).abs().max())
    print(f"latent 64, unguided ddim row 20 of 50: max abs {err:.3e} from the float64 formula")
    assert err <= BLEND_TOL and float((got - x).abs().max()) > 1e-3, err
    _, ts, coef = _tables("dpm", 20)
    assert float(coef[5, 7]) != 0.0
    g = torch.Generator().manual_seed(41)
    xs = _settled_latent(run2, x, (0.5 * torch.randn(_shape(x), generator=g) + 0.25).clamp(-3.0, 3.0), "dpm", 20, 5)
    run2.rows(x, ts, coef, [0, 0], 5)
    h = run2.read("x0_hist", _shape(x))
    got = run2.rows(xs, ts, coef, [5, 5], 1, resume=1)
    want, x0 = _update64(xs.double(), run2.read("eps", _shape(x)).double(), coef[5].tolist(), h.double())
    err = float((got.double() - want).abs().max())
    errh = float((run2.read("x0_hist", _shape(x)).double() - x0).abs().max())
    print(f"latent 64, unguided dpm row 5 of 20, resumed: max abs {err:.3e} from the float64 formula, history {errh:.3e} (max |x0| {float(x0.abs().max()):.2f})")
    assert float(x0.abs().max()) <= 5.0                                        # the premise of the bound
    assert err <= BLEND_TOL and errh <= BLEND_TOL, (err, errh)


def test_soft_mask_against_the_float64_formula(run2, inputs3):
    """One masked row with 0 < m < 1 (sampling.region_mask with feather 2 on the 64 x 64 grid of a 512-px image): the mask is indexed per
    face with ef & (L*L - 1) at L*L = 4096.  max abs <= BLEND_TOL, as test_mask.py::test_soft_mask_against_the_float64_formula.
    Measured: DDIM 2.8e-7, DPM 3.3e-7."""
    from hifidiff_amd import sampling
    from test_mask import BLEND_TOL, _kn64, _tables
    x, crl = _prepared(run2, inputs3)
    m1 = sampling.region_mask([(96, 64, 416, 384)], L64, image_res=512, feather=2)
    assert tuple(m1.shape) == (L64, L64) and 0.2 <= float(m1.mean()) <= 0.8 and bool(((m1 > 0) & (m1 < 1)).any())
    m = torch.stack([m1, m1.flip(0).contiguous()])                             # another mask per face: a wrong face offset shows
    for kind in ("ddim", "dpm"):
        _, ts, coef = _tables(kind, 20)
        u = run2.rows(x, ts, coef, [0, 0], 1)
        run2.mask(m, crl, x)
        try:
            got = run2.rows(x, ts, coef, [0, 0], 1)
        finally:
            run2.clear()
        md = m[:, None].double()
        want = md * u.double() + (1.0 - md) * _kn64(coef, 1, crl, x)
        err = float((got.double() - want).abs().max())
        print(f"latent 64, soft mask, one {kind} row: max abs {err:.3e} from the float64 formula")
        assert err <= BLEND_TOL, (kind, err)


def test_guided_row_and_untouched_unguided_path(run2, inputs3):
    """guided_update_kernel on 64 x 64 planes (3 x 16 KB of LDS, its maximum): DDIM row 20 of 50 through test_guide._check_row -- N in
    {1, 4, 64} x w in {0.3, 1.0}, N = 64 being the plane mean -- new latents and preview within GUIDE_TOL of the float64 formula on the
    device's own eps, with |x0g| <= 5 as the bound's premise.  Around it: the unguided loop and the per-face loop are bit-identical before
    guidance was switched on, while it is on with no face guided, after faces were guided and cleared, and after it was switched off.
    Measured: new latents 4.0e-7, preview 3.8e-7, max |x0g| 4.23."""
    from test_guide import GUIDE_TOL, _check_row
    from test_mask import _tables
    x, crl = _prepared(run2, inputs3)
    _, ts, coef = _tables("ddim", 50)
    loops = lambda: (run2.full(x, ts[:5], coef[:5]), run2.rows(x, ts[:5], coef[:5], [0, 3], 5))      # noqa: E731
    same = lambda a, b: torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                             # noqa: E731
    assert run2.opt("guide") == 0
    base = loops()
    run2.guide_config(1)
    try:
        assert same(loops(), base)
        worst = _check_row(run2, x, crl, "ddim", 50, 20)
        print(f"latent 64, guided ddim row 20 of 50: {worst}")
        assert max(worst["x"], worst["preview"]) <= GUIDE_TOL and worst["|x0g|"] <= 5.0, worst
        run2.guide(crl, 0.5, 4)
        assert run2.opt("guided_faces") == 2 and not same(loops(), base)
        run2.unguide()
        assert run2.opt("guided_faces") == 0 and same(loops(), base)
    finally:
        run2.guide_config(0)
    assert same(loops(), base)
