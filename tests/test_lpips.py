"""hd_lpips on the GPU: every launch on its own inputs (tools/lpips_forced.py), the scores against `metrics.lpips_reference` in float64 on
the CPU, the exact properties the reduction order gives, the reference loop's composition and the refusals.

Bounds.  Per launch: tools/forced.py's (3e-3 rel-L2 for bf16-stored outputs of bf16-operand launches, per face too; bit-exact data
movement; the distance kernel against float64 at 4 x torch's own fp32 error).  Scores: nothing absolute is fixed.  The yardstick is the
error of the contract's own number formats, `lpips_reference(emulate_bf16=True)` in float64 against plain float64, and the worst
|kernel - f64| over a set of >= 30 faces must stay within 4 x the worst yardstick error over the same set (tools/lpips_cases.py: 30
faces, perturbation amplitudes 0.3 / 0.05 / 0.005 of a smooth base image, scores 1e-5 .. 2.4e-2).  Absolute, not relative: at scores
near 1e-5 the emulation itself is off by several per cent.  The same rule holds for the per-layer d_k.
Measured on an MI355X (profiles/r23_lpips.txt; tools/lpips_bench.py records the figures from the same functions): lpips over the 30
faces worst |kernel - f64| 4.345e-06 against 4.346e-06 for the emulation (bound 1.738e-05; per case 0.93 - 1.04 x the yardstick); the
150 d_k 3.305e-06 against 3.306e-06; evaluate() over 30 faces 5.058e-06 against 5.060e-06; the decoded batch 8.9e-06 against 9.2e-06.
Per launch at B = 3 / 64 px and B = 2 / 128 px: convolutions rel-L2 <= 4.2e-05 (worst face 7.2e-05), input, pools and combine exact,
distance max-abs 6.4e-11 against torch fp32's 9.0e-11 .. 2.0e-10."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

HD_ERR_INVALID, HD_ERR_NOT_READY = -1, -4                            # include/hifidiff_hip.h


def _lc():
    import lpips_cases
    return lpips_cases


def _bits(*ts):
    return [t.cpu().numpy().tobytes() for t in ts]


# ------------------------------------------------------------------------------------------------ per launch
@pytest.mark.parametrize("B,R", [(3, 64), (2, 128)])
def test_every_launch_on_its_own_inputs(B, R):
    import forced
    import lpips_forced
    lc = _lc()
    img, ref = lc.family(0.05, B, R, R, tag="forced")
    report = []
    worst = lpips_forced.scan(lc.model(), lc.state(), img, ref, report)
    print("\n".join(report))
    print(worst)
    assert worst["launches"] == 10 and worst["no_rule"] == 0
    assert not [ln for ln in report if "<<<<<<" in ln or "no rule" in ln]
    assert worst["input"] == 0 and worst["input.pad"] == 0 and worst["pool"] == 0 and worst["combine"] == 0
    assert worst["conv"] <= forced.BF16_BOUND and worst["face"]["conv"] <= forced.BF16_BOUND
    err, err32 = worst["f64"]["distance"]
    assert err <= forced.F64_MARGIN * err32 and worst["distance"] <= forced.FP32_BOUND


# ------------------------------------------------------------------------------------------------ against float64
def _case_ids():
    import lpips_cases
    return [c.name for c in lpips_cases.CASES]


@pytest.mark.parametrize("name", _case_ids())
def test_case_runs_and_leaves_its_inputs(name):
    """One case of the set: shapes, dtypes, finite and positive, layers sum to the total, inputs only read.  Its error goes into the
    set-wide test below: a single face's error can be small by chance."""
    lc = _lc()
    case = next(c for c in lc.CASES if c.name == name)
    r = lc.run(case)
    assert r.got.dtype == torch.float64 and tuple(r.got.shape) == (case.B,) and tuple(r.got_layers.shape) == (case.B, 5)
    assert bool(torch.isfinite(r.got_layers).all()) and bool((r.got_layers > 0).all())
    k, y = float((r.got - r.ref.f64).abs().max()), float((r.ref.emu - r.ref.f64).abs().max())
    print(f"{name}: score {[float('%.4g' % v) for v in r.ref.f64]}, |kernel - f64| {k:.3e}, |emulation - f64| {y:.3e}")
    assert float(((r.got_layers.sum(dim=1) - r.got).abs() / r.got).max()) <= 1e-15
    assert r.inputs_unchanged


def test_scores_over_the_set():
    lc = _lc()
    for what, layers in (("lpips", False), ("d_k", True)):
        k, y, n, lo, hi = lc.score_errors(tuple(lc.CASES), layers)
        print(f"{what}, {n} values in [{lo:.2e}, {hi:.2e}]: worst |kernel - f64| {k:.3e}, worst |emulation - f64| {y:.3e} (bound {lc.FACTOR * y:.3e})")
        assert n >= 30 and k <= lc.FACTOR * y, (what, k, y)


# ------------------------------------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("B,R", [(1, 64), (3, 64), (1, 192)])
def test_identical_inputs_score_exactly_zero(B, R):
    lc = _lc()
    img = lc.family(0.3, B, R, R, tag="identical")[0].cuda()
    out, layers = lc.model()(img, img.clone(), per_layer=True)
    assert torch.equal(out.cpu(), torch.zeros(B, dtype=torch.float64)) and torch.equal(layers.cpu(), torch.zeros((B, 5), dtype=torch.float64))
    small = F.interpolate(img, 64, mode="bicubic", align_corners=False) if R != 64 else img      # the same through the normalised path
    out = lc.model()(small, small.clone(), input_normalize="face")
    assert torch.equal(out.cpu(), torch.zeros(B, dtype=torch.float64))


def test_symmetry_and_repeatability():
    lc = _lc()
    img, ref = (t.cuda() for t in lc.family(0.05, 3, 128, 128, tag="symmetry"))
    m = lc.model()
    ab, ba = m(img, ref, per_layer=True), m(ref, img, per_layer=True)
    assert _bits(*ab) == _bits(*ba)                                   # swapping images and ref: the same bits
    assert _bits(*m(img, ref, per_layer=True)) == _bits(*ab)          # and from call to call
    assert float(ab[0].min()) > 1e-4 and len({float(v) for v in ab[0]}) == 3


@pytest.mark.parametrize("R,Rb,norm", [(64, 64, None), (64, 128, "face")])
def test_batch_position(R, Rb, norm):
    """A face moved to another slot of a batch of the same size keeps its bits.  A face alone against the same face in a larger batch may
    run on another GEMM tile (the row count chooses it) and need not match in bits: that pair is held to the set's yardstick rule
    instead, against float64."""
    lc = _lc()
    img, ref = (t.cuda() for t in lc.family(0.05, 5, R, Rb, tag="position"))
    m = lc.model()
    full = m(img, ref, input_normalize=norm, per_layer=True)
    assert len({float(v) for v in full[0]}) == 5                      # the faces differ: the comparison below is not vacuous
    for i, slot in ((0, 4), (2, 0), (4, 1), (1, 3)):
        perm = list(range(5))
        perm[slot], perm[i] = perm[i], perm[slot]
        moved = m(img[perm].contiguous(), ref[perm].contiguous(), input_normalize=norm, per_layer=True)
        assert _bits(moved[0][slot], moved[1][slot]) == _bits(full[0][i], full[1][i]), (i, slot)
    from hifidiff_amd import metrics
    want = metrics.lpips_reference(lc.state(), img.cpu().double(), ref.cpu().double(), input_normalize=norm)
    emu = metrics.lpips_reference(lc.state(), img.cpu().double(), ref.cpu().double(), input_normalize=norm, emulate_bf16=True)
    alone = torch.cat([m(img[i:i + 1], ref[i:i + 1], input_normalize=norm) for i in range(5)]).cpu()
    k, y = float((alone - want).abs().max()), float((emu - want).abs().max())
    print(f"alone: |kernel - f64| {k:.3e}, in the batch {float((full[0].cpu() - want).abs().max()):.3e}, emulation {y:.3e}")
    assert k <= lc.FACTOR * y and float((full[0].cpu() - want).abs().max()) <= lc.FACTOR * y


def test_unit_range_flag_and_optional_layers():
    lc = _lc()
    img, ref = (t.cuda() for t in lc.family(0.05, 2, 64, 64, tag="unit"))
    m = lc.model()
    a = m(img, ref)
    b = m(2 * img - 1, 2 * ref - 1, normalize=False)                  # 2x - 1 is exact in fp32 for x in [0, 1] up to one rounding of x near 0
    assert float((a - b).abs().max()) <= 1e-4 * float(a.max())
    t, layers = m(img, ref, per_layer=True)
    assert _bits(t) == _bits(a) and tuple(m(img[:0], ref[:0]).shape) == (0,)


# ------------------------------------------------------------------------------------------------ the reference loop's composition
def test_evaluate_against_the_written_out_composition():
    """val_loop's lines in torch ops, float64: interpolate, batch min-max, LPIPS with normalize=True; `evaluate(..., lpips=model)` against
    them over 30 faces, under the set's yardstick rule.  Without a model, evaluate keeps the bits it had."""
    lc = _lc()
    from hifidiff_amd import metrics
    st, m = lc.state(), lc.model()

    def composition(result, target, emulate):
        r = F.interpolate(result, target.shape[-1], mode="bicubic") if result.shape[-1] != target.shape[-1] else result
        rn = (r - r.min()) / (r.max() - r.min())
        tn = (target - target.min()) / (target.max() - target.min())
        return metrics.lpips_reference(st, rn, tn, normalize=True, emulate_bf16=emulate)

    k = y = 0.0
    n = 0
    for amp in lc.AMPS:
        for R, Rb in ((64, 128), (128, 128)):
            result, target = lc.family(amp, 5, R, Rb, tag="evaluate")
            result = result * 2.2 - 0.6                                # a decoded image's range, not [0, 1]
            want, emu = composition(result.double(), target.double(), False), composition(result.double(), target.double(), True)
            ev = metrics.evaluate(result.cuda(), target.cuda(), lpips=m)
            plain = metrics.evaluate(result.cuda(), target.cuda())
            assert plain.lpips is None and _bits(plain.psnr, plain.ssim) == _bits(ev.psnr, ev.ssim)
            assert _bits(plain.psnr) == _bits(metrics.image_metrics(result.cuda(), target.cuda(), channels="rgb", normalize="batch").psnr)
            assert _bits(plain.ssim) == _bits(metrics.image_metrics(result.cuda(), target.cuda(), channels="y", normalize="batch").ssim)
            assert ev.lpips.dtype == torch.float64 and tuple(ev.lpips.shape) == (5,)
            k, y = max(k, float((ev.lpips.cpu() - want).abs().max())), max(y, float((emu - want).abs().max()))
            n += 5
    print(f"evaluate, lpips over {n} faces: worst |kernel - f64| {k:.3e}, emulation {y:.3e} (bound {lc.FACTOR * y:.3e})")
    assert n >= 30 and k <= lc.FACTOR * y, (k, y)


def test_scores_of_a_decoded_batch_on_the_same_stream():
    """decode_scaled then LPIPS.__call__ on one stream, nothing synchronised in between: the scores of the decoded tensor."""
    lc = _lc()
    from hifidiff_amd import metrics, synth
    from hifidiff_amd.vae import AutoencoderKL
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict())
    vae.to("cuda:0")
    z = torch.from_numpy(np.stack([np.float32(0.8) * synth.randn(f"metrics_z/{f}", (4, 16, 16)) for f in range(2)])).cuda()
    target = lc.family(0.05, 2, 128, 128, tag="decoded")[1].cuda()
    images = vae.decode_scaled(z)
    got = lc.model()(images, target, input_normalize="face")          # enqueued behind the decode
    dec = images.cpu()
    want = metrics.lpips_reference(lc.state(), dec.double(), target.cpu().double(), input_normalize="face")
    emu = metrics.lpips_reference(lc.state(), dec.double(), target.cpu().double(), input_normalize="face", emulate_bf16=True)
    k, y = float((got.cpu() - want).abs().max()), float((emu - want).abs().max())
    print(f"decoded batch: lpips {[round(float(v), 4) for v in want]}, |kernel - f64| {k:.3e}, emulation {y:.3e}")
    assert k <= lc.FACTOR * y
    assert torch.equal(images.cpu(), dec) and _bits(lc.model()(images, target, input_normalize="face")) == _bits(got)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_argument_and_launch_nothing():
    import ctypes
    from hifidiff_amd import _lib
    lc = _lc()
    L, m = _lib.lib(), lc.model()
    img, ref = (t.cuda() for t in lc.family(0.05, 2, 64, 64, tag="refusals"))
    rng = torch.tensor([[0.0, 1.0], [0.0, 1.0]], device="cuda")
    buf = torch.full((16,), -7.0, dtype=torch.float64, device="cuda")       # out [2] | layers_out [2,5] | spare
    s = torch.cuda.current_stream().cuda_stream
    I, Rf, G, O, Ly = img.data_ptr(), ref.data_ptr(), rng.data_ptr(), buf.data_ptr(), buf[2:].data_ptr()
    n_img = 2 * 3 * 64 * 64 * 4
    #        batch images res ref ref_res unit images_range ref_range out layers   the argument the message names
    bad = [((0, I, 64, Rf, 64, 1, None, None, O, Ly), "batch"), ((1025, I, 64, Rf, 64, 1, None, None, O, Ly), "batch"),
           ((2, I, 96, Rf, 64, 1, None, None, O, Ly), " res"), ((2, I, 576, Rf, 64, 1, None, None, O, Ly), " res"),
           ((2, I, 64, Rf, 32, 1, None, None, O, Ly), "ref_res"), ((2, I, 64, Rf, 100, 1, None, None, O, Ly), "ref_res"),
           ((2, I, 64, Rf, 64, 2, None, None, O, Ly), "unit_range"), ((2, I, 64, Rf, 64, -1, None, None, O, Ly), "unit_range"),
           ((2, None, 64, Rf, 64, 1, None, None, O, Ly), "images is NULL"), ((2, I, 64, None, 64, 1, None, None, O, Ly), "ref is NULL"),
           ((2, I, 64, Rf, 64, 1, None, None, None, Ly), "out is NULL"),
           ((2, I + 2, 64, Rf, 64, 1, None, None, O, Ly), "aligned to 4"), ((2, I, 64, Rf, 64, 1, G + 1, None, O, Ly), "aligned to 4"),
           ((2, I, 64, Rf, 64, 1, None, None, O + 4, Ly), "aligned to 8"), ((2, I, 64, Rf, 64, 1, None, None, O, Ly + 4), "aligned to 8"),
           ((2, I, 64, Rf, 64, 1, None, None, I + n_img - 8, Ly), "out overlaps images"), ((2, I, 64, Rf, 64, 1, None, None, O, Rf), "layers_out overlaps ref"),
           ((2, I, 64, Rf, 64, 1, G, None, G, Ly), "out overlaps images_range"), ((2, I, 64, Rf, 64, 1, None, G, G + 8, Ly), "out overlaps ref_range"),
           ((2, I, 64, Rf, 64, 1, None, None, O, O + 8), "out overlaps layers_out")]
    before = (img.clone(), ref.clone())
    for args, word in bad:
        rc = L.hd_lpips(m._ctx, *args, s)
        msg = L.hd_last_error(m._ctx).decode()
        assert rc == HD_ERR_INVALID and msg.startswith("hd_lpips:") and word in msg, (args, rc, msg)
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all()) and torch.equal(img, before[0]) and torch.equal(ref, before[1])      # nothing was launched
    # out may end exactly where layers_out begins
    _lib.check(L.hd_lpips(m._ctx, 2, I, 64, Rf, 64, 1, None, None, O, Ly, s), m._ctx)
    want = m(img, ref, per_layer=True)
    assert _bits(buf[:2], buf[2:12].reshape(2, 5)) == _bits(*want) and float(buf[12]) == -7.0
    # wrong context kinds, and weights that are not finalized
    from hifidiff_amd import synth
    from hifidiff_amd.vae import AutoencoderKL
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict())
    vae.to("cuda:0")
    assert L.hd_lpips(vae._ctx, 2, I, 64, Rf, 64, 1, None, None, O, Ly, s) == HD_ERR_INVALID and b"not an LPIPS context" in L.hd_last_error(vae._ctx)
    lat = torch.zeros((1, 4, 8, 8), device="cuda")
    assert L.hd_vae_decode(m._ctx, 1, 8, lat.data_ptr(), img.data_ptr(), s) == HD_ERR_INVALID
    raw = ctypes.c_void_p()
    _lib.check(L.hd_lpips_create(ctypes.byref(raw), 0))
    try:
        assert L.hd_lpips(raw, 2, I, 64, Rf, 64, 1, None, None, O, Ly, s) == HD_ERR_NOT_READY and b"finalized" in L.hd_last_error(raw)
        assert L.hd_finalize_weights(raw) == -3 and b"Missing key" in L.hd_last_error(raw)      # strict: nothing was loaded
    finally:
        L.hd_destroy(raw)
    torch.cuda.synchronize()
    assert float(buf[12]) == -7.0
