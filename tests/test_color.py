"""hd_color_fix on the GPU against the float64 reference formulas of hifidiff_amd.color on the CPU.

Bounds.  Wavelet: max-abs <= 1e-5 * max(1, max|s - c|): one subtraction, 2n passes of at most two roundings each on convex
combinations with exact power-of-two weights, one multiply-add: <= 23 roundings of 2^-24 relative at magnitude <= max|s - c| + |c|,
about 2.6e-6 * max|s - c|; the bound allows 4 x.  With a resampled reference the bicubic's own fp32 error is added: 4 x the max-abs
error of torch's fp32 CPU bicubic against its float64 bicubic on the same input (tools/vae_forced.bicubic_errors, the rule of
tests/test_vae_ops.py::test_bicubic_alone).  AdaIN: max-abs <= 2e-5 * max|a|: the statistics are accumulated in fp64 (error below
1e-7), the apply is a handful of fp32 roundings.
Measured on an MI355X: wavelet 6e-8 .. 1.4e-7 on uniform images (resampled references included), 0 on the +-1 step images and on every
impulse (all weights are powers of two); AdaIN 8e-8 .. 1.4e-7."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

WAVELET_TOL = 1e-5
ADAIN_TOL = 2e-5


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _rand(tag, B, R):
    from hifidiff_amd import synth
    return T(np.stack([synth.rand(f"{tag}/{f}", (3, R, R)) for f in range(B)]))


def _images(tag, B, R):
    """c and s: uniform images mapped to [-1, 1]."""
    return _rand(tag + "/c", B, R) * 2 - 1, _rand(tag + "/s", B, R) * 2 - 1


def _steps(tag, B, R):
    return (torch.where(_rand(tag + "/cs", B, R) < 0.5, -1.0, 1.0).to(torch.float32),
            torch.where(_rand(tag + "/ss", B, R) < 0.5, -1.0, 1.0).to(torch.float32))


def _fix(c, s, **kw):
    from hifidiff_amd import color
    return color.color_fix(c.cuda(), s.cuda(), **kw).cpu()


def _wavelet_want(c, s, n=5, weight=None):
    from hifidiff_amd import color
    return color.wavelet_color_fix_reference(c.double(), s.double(), levels=n, weight=weight)


def _wavelet_check(what, got, c, s, n=5, weight=None, extra=0.0):
    want = _wavelet_want(c, s, n, weight)
    err = float((got.double() - want).abs().max())
    bound = WAVELET_TOL * max(1.0, float((s.double() - c.double()).abs().max())) + extra
    print(f"wavelet {what}: max abs {err:.3e} (bound {bound:.3e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(c.shape)
    assert err <= bound, (what, err, bound)
    return want


# ------------------------------------------------------------------------------------------------ wavelet
@pytest.mark.parametrize("R", [64, 128, 192])
def test_wavelet_same_size(R):
    """64: one tile, halo clipped on all four sides; 128: the smallest size with seams; 192: the smallest with a tile whose whole halo
    lies inside the image."""
    for what, (c, s) in (("uniform", _images(f"wavelet{R}", 2, R)), ("steps", _steps(f"wavelet{R}", 2, R))):
        c0, s0 = c.clone(), s.clone()
        cd, sd = c.cuda(), s.cuda()
        from hifidiff_amd import color
        got = color.color_fix(cd, sd)
        _wavelet_check(f"{R} px, {what}", got.cpu(), c, s)
        assert torch.equal(cd.cpu(), c0) and torch.equal(sd.cpu(), s0)          # the inputs are only read
        assert got.data_ptr() not in (cd.data_ptr(), sd.data_ptr())


def _impulse_positions(R):
    m, e = R // 2, R - 1
    pos = [(0, 0), (0, e), (e, 0), (e, e), (0, m), (e, m), (m, 0), (m, e), (m, m)]
    seams = list(range(64, R, 64))
    q = R // 2 - 17                                                   # a coordinate away from every seam
    for k in seams:
        pos += [(k - 1, q), (k, q), (q, k - 1), (q, k)]
        for j in seams:
            pos += [(k - 1, j - 1), (k, j), (k - 1, j), (k, j - 1)]
    return pos


@pytest.mark.parametrize("R", [64, 128, 192])
def test_wavelet_impulses(R):
    """c = 0, s = a single 1: at the corners, the middle of each edge, the centre and both sides of every tile seam, one impulse per plane.
    A per-level clamping or halo error shows as an error of a whole tap: the smallest tap of the n = 5 response is 2^-10."""
    pos = _impulse_positions(R)
    B = (len(pos) + 2) // 3
    s = torch.zeros((B * 3, R, R))
    for i, (y, x) in enumerate(pos):
        s[i, y, x] = 1.0
    s = s.reshape(B, 3, R, R)
    c = torch.zeros_like(s)
    got = _fix(c, s)
    want = _wavelet_check(f"{R} px, {len(pos)} impulses", got, c, s)
    per = (got.double() - want).abs().reshape(B * 3, -1).max(dim=1).values
    worst = int(per.argmax())
    assert float(per.max()) <= WAVELET_TOL, ("impulse at", pos[min(worst, len(pos) - 1)], float(per.max()))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_wavelet_levels(n):
    c, s = _images(f"levels{n}", 1, 128)
    _wavelet_check(f"128 px, n = {n}", _fix(c, s, levels=n), c, s, n)


def test_wavelet_tiling_independence():
    """The 128-px case per 64-px quadrant, each against the float64 formula on the full image: a failure names the seam."""
    c, s = _images("quadrants", 2, 128)
    got = _fix(c, s).double()
    want = _wavelet_want(c, s)
    bound = WAVELET_TOL * max(1.0, float((s - c).abs().max()))
    for qy in (0, 1):
        for qx in (0, 1):
            sl = (Ellipsis, slice(64 * qy, 64 * qy + 64), slice(64 * qx, 64 * qx + 64))
            err = float((got[sl] - want[sl]).abs().max())
            print(f"tile ({qy}, {qx}): max abs {err:.3e}")
            assert err <= bound, ((qy, qx), err, bound)


@pytest.mark.parametrize("Rr,R,vae_range", [(128, 256, False), (128, 64, False), (128, 64, True), (128, 256, True)])
def test_wavelet_resampled_reference(Rr, R, vae_range):
    import vae_forced
    from hifidiff_amd import color
    c = _images(f"resampled{R}", 1, R)[0]
    s = _rand(f"resampled{R}/ref", 1, Rr) * 1.4 - 0.2                 # [-0.2, 1.2]: the range mapping clamps on both sides
    mapped = color.to_vae_range(s.double()) if vae_range else s.double()
    sp = F.interpolate(mapped, size=(R, R), mode="bicubic", align_corners=False)
    _, err32 = vae_forced.bicubic_errors(sp, mapped.float(), R)       # the resampler's own fp32 error on this input
    got = _fix(c, s, ref_vae_range=vae_range)
    want = color.wavelet_color_fix_reference(c.double(), s.double(), ref_vae_range=vae_range)
    assert float((want - _wavelet_want(c, sp)).abs().max()) <= 1e-12  # the reference resamples after the range mapping
    err = float((got.double() - want).abs().max())
    bound = WAVELET_TOL * max(1.0, float((sp - c.double()).abs().max())) + 4.0 * err32
    print(f"wavelet {Rr} -> {R}, vae_range {vae_range}: max abs {err:.3e} (bound {bound:.3e}, torch fp32 bicubic {err32:.3e})")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ AdaIN
def _adain_inputs(tag, B, R, Rr):
    return _rand(tag + "/c", B, R) * 2 - 1, 0.5 * _rand(tag + "/s", B, Rr) + 0.2


def _adain_check(what, got, c, s, weight=None, **kw):
    from hifidiff_amd import color
    a = color.adain_color_fix_reference(c.double(), s.double(), **kw)
    want = color.adain_color_fix_reference(c.double(), s.double(), weight=weight, **kw)
    err = float((got.double() - want).abs().max())
    bound = ADAIN_TOL * float(a.abs().max())
    print(f"AdaIN {what}: max abs {err:.3e} (bound {bound:.3e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(c.shape)
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("B,R,Rr", [(2, 64, 64), (2, 128, 128), (1, 256, 128)])
def test_adain(B, R, Rr):
    c, s = _adain_inputs(f"adain{R}", B, R, Rr)
    cd, sd = c.cuda(), s.cuda()
    from hifidiff_amd import color
    got = color.color_fix(cd, sd, mode="adain", levels=99)            # levels is ignored in this mode
    _adain_check(f"{Rr} -> {R}, batch {B}", got.cpu(), c, s)
    assert torch.equal(cd.cpu(), c) and torch.equal(sd.cpu(), s)


def test_adain_vae_range():
    c, s = _adain_inputs("adain_range", 1, 64, 128)
    s = s * 2.8 - 0.76                                                # [-0.2, 1.2]
    _adain_check("vae_range", _fix(c, s, mode="adain", ref_vae_range=True), c, s, ref_vae_range=True)


def test_adain_constant_plane():
    """Variance 0 leaves only the 1e-5 term: the result is finite and the plane takes mean(s)."""
    c, s = _adain_inputs("adain_const", 1, 64, 64)
    c[0, 1] = 0.3
    got = _fix(c, s, mode="adain")
    assert bool(torch.isfinite(got).all())
    err = float((got[0, 1].double() - s[0, 1].double().mean()).abs().max())
    print(f"AdaIN constant plane: off mean(s) by {err:.3e}")
    assert err <= 1e-5
    _adain_check("constant plane", got, c, s)


# ------------------------------------------------------------------------------------------------ weights, both modes
@pytest.mark.parametrize("mode", ["wavelet", "adain"])
def test_weights(mode):
    if mode == "wavelet":
        c, s = _images("weights", 3, 128)
    else:
        c, s = _adain_inputs("weights", 3, 128, 128)
    w = torch.tensor([0.0, 0.5, 1.0])
    got = _fix(c, s, mode=mode, weight=w.cuda())
    plain = _fix(c, s, mode=mode)
    assert torch.equal(got[0], c[0])                                  # w = 0: the image, bit for bit
    assert torch.equal(got[2], plain[2])                              # w = 1: the unweighted call, bit for bit
    assert torch.equal(_fix(c, s, mode=mode, weight=1.0), plain) and torch.equal(_fix(c, s, mode=mode, weight=0.0), c)
    if mode == "wavelet":
        _wavelet_check("weights", got, c, s, weight=w.double())
    else:
        _adain_check("weights", got, c, s, weight=w.double())
    assert not torch.equal(got[1], plain[1]) and not torch.equal(got[1], c[1])


@pytest.mark.parametrize("mode", ["wavelet", "adain"])
def test_repeatable_and_adjacent_buffers(mode):
    """Two calls on the same inputs give equal bits; and `out` may end exactly where `images` begins (no overlap)."""
    from hifidiff_amd import _lib, color
    c, s = _images("repeat", 2, 128) if mode == "wavelet" else _adain_inputs("repeat", 2, 128, 128)
    cd, sd = c.cuda(), s.cuda()
    a, b = color.color_fix(cd, sd, mode=mode), color.color_fix(cd, sd, mode=mode)
    assert torch.equal(a, b)
    both = torch.empty((2,) + tuple(c.shape), device="cuda")
    both[1].copy_(cd)
    args = (2, 128, sd.data_ptr(), 128, 0, color.MODES[mode], 5, None, torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().hd_color_fix(both[1].data_ptr(), both[0].data_ptr(), *args))
    assert torch.equal(both[0], a) and torch.equal(both[1], cd)
    rc = _lib.lib().hd_color_fix(both[1].data_ptr(), both[1].data_ptr(), *args)          # in place: refused, nothing launched
    assert rc == -1 and b"out overlaps images" in _lib.lib().hd_last_error(None)
    torch.cuda.synchronize()
    assert torch.equal(both[1], cd)


# ------------------------------------------------------------------------------------------------ decode with a colour reference
def test_decode_with_a_colour_reference():
    from hifidiff_amd import color, synth
    from hifidiff_amd.vae import AutoencoderKL
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict())
    vae.to("cuda:0")
    z = T(np.stack([np.float32(0.8) * synth.randn(f"color_z/{f}", (4, 16, 16)) for f in range(2)])).cuda()
    r = (_rand("color_ref", 2, 128) * 2 - 1).cuda()
    plain = vae.decode_scaled(z)
    for kw in (dict(), dict(color_mode="adain"), dict(color_levels=3, color_weight=torch.tensor([0.25, 1.0]))):
        fixed = vae.decode_scaled(z, color_ref=r, **kw)
        want = color.color_fix(plain, r, mode=kw.get("color_mode", "wavelet"), levels=kw.get("color_levels", 5), weight=kw.get("color_weight"))
        assert torch.equal(fixed, want) and not torch.equal(fixed, plain)
        assert torch.equal(vae.decode_scaled(z), plain)               # the default path: the same bits before and after
    assert tuple(vae.decode_scaled(z[:0], color_ref=r[:0]).shape) == (0, 3, 128, 128)
    with pytest.raises(ValueError):
        vae.decode_scaled(z, color_ref=r[:1])
