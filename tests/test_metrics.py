"""hd_image_metrics / hd_image_range on the GPU against the float64 formulas of hifidiff_amd.metrics on the CPU.

Bounds.  Nothing absolute is fixed except where it can be derived: the yardstick is the error of the same formula evaluated in fp32 by
torch on the same inputs, times the project's factor 4 (tools/metrics_cases.py holds the cases and recomputes the yardsticks).
  SSIM map, per case:  max over pixels |kernel - f64| <= 4 x max over pixels |torch fp32 - f64| (the cancellation in E[x^2] - mu^2 over flat
                       regions dominates both)
  per-face SSIM (absolute), MSE in the y / resampled / normalised cases (relative), hd_image_range with resampling (absolute): the worst
                       error over the whole set (>= 30 values each) <= 4 x the worst torch-fp32 error over the same set -- a single face's
                       signed mean error can be tiny by chance
  MSE, rgb without resampling or normalisation:  relative error <= 8 * 2^-24: one rounding in a - b, up to two more in the square, and the
                       fp64 sums are negligible
  hd_image_range without resampling: the bits of amin / amax.
Measured on an MI355X (profiles/r22_metrics.txt; tools/metrics_bench.py records the figures from the same functions): SSIM map 0.77 - 1.16 x
the yardstick (1.6e-6 on noise .. 2.3e-4 on the flat patch); per-face SSIM 1.3e-6 against 1.5e-6; MSE 1.6e-6 against 1.6e-6 relative;
range 1.6e-7 against 1.4e-7; plain rgb MSE 1e-10 .. 7e-10 relative; identical inputs |1 - SSIM| <= 1.3e-8."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


def _mc():
    import metrics_cases
    return metrics_cases


def _case_ids():
    import metrics_cases
    return [c.name for c in metrics_cases.CASES]


def _bits(m):
    return [None if t is None else t.cpu().numpy().tobytes() for t in (m.mse, m.ssim, m.ssim_map)]


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("name", _case_ids())
def test_ssim_map(name):
    mc = _mc()
    case = next(c for c in mc.CASES if c.name == name)
    r = mc.run(case)
    P, V = 3 if case.channels == "rgb" else 1, case.Rb - 10
    assert r.got.ssim_map.dtype == torch.float32 and tuple(r.got.ssim_map.shape) == (case.B, P, V, V)
    assert r.got.mse.dtype == torch.float64 and tuple(r.got.mse.shape) == (case.B,) and tuple(r.got.ssim.shape) == (case.B,)
    k, y = mc.map_errors(r)
    print(f"{name}: SSIM map max abs {k:.3e}, torch fp32 {y:.3e} (bound {mc.FACTOR * y:.3e}); SSIM {[round(float(v), 4) for v in r.f64.ssim]}")
    assert bool(torch.isfinite(r.got.ssim_map).all())
    assert k <= mc.FACTOR * y, (name, k, y)
    assert r.inputs_unchanged                                          # images and ref are only read
    # the face's score is the mean of the map it returned
    assert float((r.got.ssim - r.got.ssim_map.double().mean(dim=(1, 2, 3))).abs().max()) <= 1e-12
    assert float((r.got.psnr - 10 * torch.log10(case.L * case.L / r.got.mse)).abs().max()) <= 1e-9


def test_scores_over_the_set():
    mc = _mc()
    k, y, n = mc.score_errors(mc.CASES, "ssim")
    print(f"per-face SSIM, {n} values: worst abs {k:.3e}, torch fp32 {y:.3e} (bound {mc.FACTOR * y:.3e})")
    assert n >= 30 and k <= mc.FACTOR * y, (k, y)
    k, y, n = mc.score_errors(mc.OTHER_MSE, "mse")
    print(f"MSE (y / resampled / normalised), {n} values: worst rel {k:.3e}, torch fp32 {y:.3e} (bound {mc.FACTOR * y:.3e})")
    assert n >= 30 and k <= mc.FACTOR * y, (k, y)


def test_plain_rgb_mse():
    mc = _mc()
    assert len(mc.PLAIN_MSE) >= 3
    for c in mc.PLAIN_MSE:
        r = mc.run(c)
        rel = float(((r.got.mse - r.f64.mse).abs() / r.f64.mse).max())
        print(f"{c.name}: MSE rel {rel:.3e} (bound {mc.PLAIN_MSE_BOUND:.3e})")
        assert rel <= mc.PLAIN_MSE_BOUND, (c.name, rel)


def test_range():
    mc = _mc()
    from hifidiff_amd import metrics
    for fam, B, R in (("noise", 1, 64), ("patch", 3, 128), ("smooth", 5, 192)):
        img = mc.family(fam, B, R, R, tag="range")[0] * 3 - 1
        d = img.cuda()
        got = metrics.image_range(d)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, 2)
        assert torch.equal(got.cpu(), metrics.range_reference(img)) and torch.equal(metrics.image_range(d, R), got)      # the bits of amin / amax
        assert torch.equal(d.cpu(), img)
        assert torch.equal(metrics.image_range(d[B - 1:]), got[B - 1:])
    k, y, n = mc.range_errors()
    print(f"hd_image_range with resampling, {n} values: worst abs {k:.3e}, torch fp32 {y:.3e} (bound {mc.FACTOR * y:.3e})")
    assert n >= 30 and k <= mc.FACTOR * y, (k, y)


# ------------------------------------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("channels,L,R", [("rgb", 1.0, 64), ("y", 255.0, 192)])
def test_identical_inputs(channels, L, R):
    mc = _mc()
    from hifidiff_amd import metrics
    img = mc.family("patch", 2, R, R, L, tag="identical")[0].cuda()
    m = metrics.image_metrics(img, img.clone(), channels=channels, data_range=L, ssim_map=True)
    assert torch.equal(m.mse.cpu(), torch.zeros(2, dtype=torch.float64))
    assert bool(torch.isinf(m.psnr).all()) and bool((m.psnr > 0).all())
    err = float((1 - m.ssim).abs().max())
    print(f"identical inputs, {channels}, L = {L}: |1 - SSIM| {err:.3e}, map min {float(m.ssim_map.min()):.7f}")
    assert err <= 1e-6


@pytest.mark.parametrize("channels,normalize,R,Rb", [("rgb", None, 192, 192), ("y", "face", 64, 128)])
def test_batch_position_and_repeatability(channels, normalize, R, Rb):
    """Face i alone, at slot 0 and at slot 4 of a batch of five: the same bits, scores and map; and two calls give the same bits."""
    mc = _mc()
    from hifidiff_amd import metrics
    img, ref = (t.cuda() for t in mc.family("patch", 5, R, Rb, tag="position"))
    kw = dict(channels=channels, normalize=normalize, ssim_map=True)
    full = metrics.image_metrics(img, ref, **kw)
    assert _bits(metrics.image_metrics(img, ref, **kw)) == _bits(full)
    for i in (0, 2, 4):
        alone = metrics.image_metrics(img[i:i + 1], ref[i:i + 1], **kw)
        for slot in (0, 4):
            perm = list(range(5))
            perm[slot], perm[i] = perm[i], perm[slot]
            moved = metrics.image_metrics(img[perm].contiguous(), ref[perm].contiguous(), **kw)
            assert _bits(metrics.Metrics(moved.mse[slot:slot + 1], None, moved.ssim[slot:slot + 1], moved.ssim_map[slot:slot + 1])) == \
                _bits(alone), (i, slot)
        assert _bits(metrics.Metrics(full.mse[i:i + 1], None, full.ssim[i:i + 1], full.ssim_map[i:i + 1])) == _bits(alone), i
    assert len({float(v) for v in full.ssim}) == 5                     # the faces differ: the comparison above is not vacuous


def test_map_is_optional():
    mc = _mc()
    from hifidiff_amd import metrics
    img, ref = (t.cuda() for t in mc.family("smooth", 3, 128, 128, tag="optional"))
    for channels in ("rgb", "y"):
        a = metrics.image_metrics(img, ref, channels=channels)
        b = metrics.image_metrics(img, ref, channels=channels, ssim_map=True)
        assert a.ssim_map is None and b.ssim_map is not None
        assert _bits(a)[:2] == _bits(b)[:2]
    assert tuple(metrics.image_metrics(img[:0], ref[:0]).ssim.shape) == (0,)


def test_adjacent_buffers_and_refusals():
    """out may end exactly where an input begins; an overlapping out is refused and nothing runs."""
    from hifidiff_amd import _lib, metrics
    mc = _mc()
    img, ref = (t.cuda() for t in mc.family("noise", 2, 64, 64, tag="adjacent"))
    want = metrics.image_metrics(img, ref, channels="rgb")
    L = _lib.lib()
    n = L.hd_image_metrics_workspace(2, 64, 1)
    buf = torch.zeros((4 + n // 8,), dtype=torch.float64, device="cuda")             # out [2,2] directly followed by the workspace
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(L.hd_image_metrics(img.data_ptr(), 64, ref.data_ptr(), 64, 2, 1, 1.0, None, None, buf.data_ptr(), None, buf[4:].data_ptr(), n, s))
    assert torch.equal(buf[:4].reshape(2, 2)[:, 0], want.mse) and torch.equal(buf[:4].reshape(2, 2)[:, 1], want.ssim)
    rc = L.hd_image_metrics(img.data_ptr(), 64, ref.data_ptr(), 64, 2, 1, 1.0, None, None, buf.data_ptr(), None, buf[3:].data_ptr(), n, s)
    assert rc == -1 and b"out overlaps workspace" in L.hd_last_error(None)
    rc = L.hd_image_metrics(img.data_ptr(), 64, ref.data_ptr(), 64, 2, 1, 1.0, None, None, buf.data_ptr(), None, buf[4:].data_ptr(), n - 8, s)
    assert rc == -1 and b"workspace_bytes" in L.hd_last_error(None)


# ------------------------------------------------------------------------------------------------ the reference loop's composition
def test_evaluate_against_the_written_out_composition():
    """val_loop's lines in torch ops, float64; normalize="batch" through image_metrics and evaluate() against them, with the same
    composition in fp32 as the yardstick, over 30 faces."""
    mc = _mc()
    from hifidiff_amd import metrics

    def composition(result, target):
        r = F.interpolate(result, target.shape[-1], mode="bicubic") if result.shape[-1] != target.shape[-1] else result
        rn = (r - r.min()) / (r.max() - r.min())
        tn = (target - target.min()) / (target.max() - target.min())
        y = lambda t: ((65.481 * t[:, 0] + 128.553 * t[:, 1] + 24.966 * t[:, 2] + 16.0) / 255.0)[:, None]   # noqa: E731
        return ((rn - tn) ** 2).mean(dim=(1, 2, 3)), metrics.ssim_map_reference(y(rn), y(tn)).mean(dim=(1, 2, 3))

    worst = {"mse": [0.0, 0.0], "ssim": [0.0, 0.0]}
    n = 0
    for fam in ("noise", "smooth", "patch"):
        for R, Rb in ((64, 128), (128, 128)):
            result, target = mc.family(fam, 5, R, Rb, tag="evaluate")
            result = result * 2.2 - 0.6                                # a decoded image's range, not [0, 1]
            mse64, ssim64 = composition(result.double(), target.double())
            mse32, ssim32 = composition(result, target)
            ev = metrics.evaluate(result.cuda(), target.cuda())
            rgb = metrics.image_metrics(result.cuda(), target.cuda(), channels="rgb", normalize="batch")
            lum = metrics.image_metrics(result.cuda(), target.cuda(), channels="y", normalize="batch")
            assert torch.equal(ev.psnr, rgb.psnr) and torch.equal(ev.ssim, lum.ssim)
            assert float((ev.psnr.cpu() - 10 * torch.log10(1.0 / rgb.mse.cpu())).abs().max()) <= 1e-9
            worst["mse"][0] = max(worst["mse"][0], float(((rgb.mse.cpu() - mse64).abs() / mse64).max()))
            worst["mse"][1] = max(worst["mse"][1], float(((mse32.double() - mse64).abs() / mse64).max()))
            worst["ssim"][0] = max(worst["ssim"][0], float((lum.ssim.cpu() - ssim64).abs().max()))
            worst["ssim"][1] = max(worst["ssim"][1], float((ssim32.double() - ssim64).abs().max()))
            n += 5
    for what, (k, y) in worst.items():
        print(f"evaluate, {what} over {n} faces: worst {k:.3e}, torch fp32 {y:.3e} (bound {mc.FACTOR * y:.3e})")
        assert n >= 30 and k <= mc.FACTOR * y, (what, k, y)


def test_scores_of_a_decoded_batch_on_the_same_stream():
    """decode_scaled then image_metrics on one stream, nothing synchronised in between: the scores of the decoded tensor."""
    mc = _mc()
    from hifidiff_amd import metrics, synth
    from hifidiff_amd.vae import AutoencoderKL
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict())
    vae.to("cuda:0")
    z = torch.from_numpy(np.stack([np.float32(0.8) * synth.randn(f"metrics_z/{f}", (4, 16, 16)) for f in range(2)])).cuda()
    target = mc.family("smooth", 2, 128, 128, tag="decoded")[1].cuda()
    images = vae.decode_scaled(z)
    got = metrics.image_metrics(images, target, channels="rgb", normalize="face", ssim_map=True)     # enqueued behind the decode
    dec = images.cpu()
    want = metrics.image_metrics_reference(dec.double(), target.cpu().double(), channels="rgb", normalize="face", ssim_map=True)
    yard = metrics.image_metrics_reference(dec, target.cpu(), channels="rgb", normalize="face", ssim_map=True)
    k, y = float((got.ssim_map.cpu().double() - want.ssim_map).abs().max()), float((yard.ssim_map.double() - want.ssim_map).abs().max())
    print(f"decoded batch: SSIM {[round(float(v), 4) for v in want.ssim]}, map max abs {k:.3e}, torch fp32 {y:.3e}")
    assert k <= mc.FACTOR * y
    assert torch.equal(images.cpu(), dec) and _bits(metrics.image_metrics(images, target, channels="rgb", normalize="face", ssim_map=True)) == _bits(got)
