"""Host side of the colour correction (no GPU): the export, the argument checks of hd_color_fix that come before any HIP call, and the
reference formulas of hifidiff_amd.color in float64 -- StableSR's decomposition form against the linear form c + B_n(s - c) the kernel
evaluates."""
import pytest
import torch

from hifidiff_amd import _lib, color

HD_ERR_INVALID = -1                                                   # include/hifidiff_hip.h
TOL = 1e-12                                                           # float64 against float64, values of magnitude <= 3


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _pair(seed, B=2, R=64, Rr=None):
    c = torch.rand((B, 3, R, R), generator=_g(seed), dtype=torch.float64) * 2 - 1
    s = torch.rand((B, 3, Rr or R, Rr or R), generator=_g(seed + 1), dtype=torch.float64) * 2 - 1
    return c, s


def _B(x, n):
    for i in range(n):
        x = color.wavelet_blur(x, 2 ** i)
    return x


# ------------------------------------------------------------------------------------------------ export and argument checks
def test_the_entry_point_is_exported():
    with open(_lib.HEADER) as fh:
        header = fh.read()
    assert "hd_color_fix" in _lib.EXPORTS
    assert "int hd_color_fix(" in header
    assert hasattr(_lib.lib(), "hd_color_fix")


IMG, OUT, REF, WGT = 0x10000000, 0x20000000, 0x30000000, 0x40000000    # made-up addresses, far enough apart for batch 2 at 512 px
N64 = 2 * 3 * 64 * 64 * 4                                             # bytes of [2,3,64,64] fp32

#        images out  batch res ref  ref_res vae mode levels   the argument the message names
BAD = [
    ((IMG, OUT, 0, 64, REF, 64, 0, 1, 5), "batch"),
    ((IMG, OUT, -3, 64, REF, 64, 0, 2, 5), "batch"),
    ((IMG, OUT, 2, 0, REF, 64, 0, 1, 5), " res"),
    ((IMG, OUT, 2, 32, REF, 64, 0, 1, 5), " res"),
    ((IMG, OUT, 2, 96, REF, 64, 0, 1, 5), " res"),
    ((IMG, OUT, 2, 576, REF, 64, 0, 2, 5), " res"),
    ((IMG, OUT, 2, 64, REF, 0, 0, 1, 5), "ref_res"),
    ((IMG, OUT, 2, 64, REF, 100, 0, 2, 5), "ref_res"),
    ((IMG, OUT, 2, 64, REF, 1024, 0, 1, 5), "ref_res"),
    ((IMG, OUT, 2, 64, REF, 64, 0, 0, 5), "mode"),
    ((IMG, OUT, 2, 64, REF, 64, 0, 3, 5), "mode"),
    ((IMG, OUT, 2, 64, REF, 64, 0, 1, 0), "levels"),
    ((IMG, OUT, 2, 64, REF, 64, 0, 1, 6), "levels"),
    ((IMG, OUT, 2, 64, REF, 64, 0, 1, -1), "levels"),
    ((None, OUT, 2, 64, REF, 64, 0, 1, 5), "images"),
    ((IMG, None, 2, 64, REF, 64, 0, 1, 5), "out"),
    ((IMG, OUT, 2, 64, None, 64, 0, 2, 5), "ref"),
    ((IMG, IMG, 2, 64, REF, 64, 0, 1, 5), "out overlaps images"),                 # in place
    ((IMG, IMG + N64 - 16, 2, 64, REF, 64, 0, 1, 5), "out overlaps images"),      # the last bytes of images
    ((IMG + N64 - 16, IMG, 2, 64, REF, 64, 0, 2, 5), "out overlaps images"),      # the last bytes of out
    ((IMG, REF, 2, 64, REF, 64, 0, 1, 5), "out overlaps ref"),
    ((IMG, REF + 4 * N64 - 16, 2, 64, REF, 128, 0, 2, 5), "out overlaps ref"),    # ref is four times as long here
    ((IMG, REF - N64 + 16, 2, 64, REF, 128, 0, 1, 5), "out overlaps ref"),
    ((IMG, OUT, 2, 64, REF, 64, 2, 1, 5), "ref_vae_range"),
    ((IMG, OUT, 2, 64, REF, 64, -1, 2, 5), "ref_vae_range"),
]


@pytest.mark.parametrize("args,names", BAD, ids=["%d-%s" % (i, n.strip().replace(" ", "_")) for i, (_, n) in enumerate(BAD)])
def test_bad_arguments_are_refused_before_any_device_work(args, names):
    L = _lib.lib()
    rc = L.hd_color_fix(*args, WGT, None)
    msg = L.hd_last_error(None).decode()
    assert rc == HD_ERR_INVALID, (rc, msg)
    assert msg.startswith("hd_color_fix:") and names in msg, msg


def test_python_argument_checks():
    c, s = torch.zeros((2, 3, 64, 64)), torch.zeros((2, 3, 64, 64))
    for kw in (dict(mode="histogram"), dict(levels=0), dict(levels=6), dict(levels=2.0), dict(weight=[0.5]), dict(weight=1.5), dict(weight=[0.5, -0.1])):
        with pytest.raises(ValueError):
            color.color_fix(c, s, **kw)
    for ci, si in ((c[:, :2], s), (c, s[:1]), (torch.zeros((2, 3, 96, 96)), s), (c, torch.zeros((2, 3, 64, 128))), (c[0], s)):
        with pytest.raises(ValueError):
            color.color_fix(ci, si)
    with pytest.raises(RuntimeError):                                 # well-formed, but no CPU path exists
        color.color_fix(c, s)
    with pytest.raises(ValueError):
        color.wavelet_color_fix_reference(c, s, levels=6)
    with pytest.raises(ValueError):
        color.wavelet_color_fix_reference(c, s, weight=[1.0, 1.0, 1.0])


# ------------------------------------------------------------------------------------------------ the formulas, float64
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_decomposition_form_is_the_linear_form(n):
    c, s = _pair(10 + n)
    got = color.wavelet_color_fix_reference(c, s, levels=n)
    want = c + _B(s - c, n)
    err = float((got - want).abs().max())
    print(f"levels = {n}: high(c) + low(s) against c + B_n(s - c): max abs {err:.2e}")
    assert got.dtype == torch.float64 and err <= TOL
    high, low = color.wavelet_decomposition(c, n)
    assert float((high + low - c).abs().max()) <= TOL                 # the decomposition is exact: high telescopes to c - B_n(c)


def test_blur_is_a_separable_three_tap_pass_with_clamped_taps():
    """The evaluation order the kernel uses: a horizontal then a vertical [1/4 1/2 1/4] pass with tap coordinates clamped to the image."""
    x = _pair(3, B=1)[0]
    R = x.shape[-1]
    for r in (1, 2, 4, 8, 16):
        i = torch.arange(R)
        lo, hi = (i - r).clamp(0, R - 1), (i + r).clamp(0, R - 1)
        h = 0.5 * x + 0.25 * (x[..., lo] + x[..., hi])
        v = 0.5 * h + 0.25 * (h[..., lo, :] + h[..., hi, :])
        assert float((v - color.wavelet_blur(x, r)).abs().max()) <= TOL, r


def test_wavelet_fixed_points():
    c, _ = _pair(20)
    # s == c: the linear form returns c exactly (B_n(0) = 0); the decomposition form adds high and low back up and may round
    assert torch.equal(c + _B(c.clone() - c, 5), c)
    assert float((color.wavelet_color_fix_reference(c, c.clone()) - c).abs().max()) <= TOL
    shifted = color.wavelet_color_fix_reference(c, c + 0.375)
    assert float((shifted - (c + 0.375)).abs().max()) <= TOL          # the blur of a constant under replicate padding is the constant


@pytest.mark.parametrize("fn", [color.wavelet_color_fix_reference, color.adain_color_fix_reference])
def test_weight_scales_the_correction(fn):
    c, s = _pair(30, B=3)
    full = fn(c, s)
    got = fn(c, s, weight=torch.tensor([0.0, 0.25, 1.0]))
    assert torch.equal(got[0], c[0])                                  # w = 0: the image itself
    assert float((got[1] - (c[1] + 0.25 * (full[1] - c[1]))).abs().max()) <= TOL
    assert float((got[2] - full[2]).abs().max()) <= TOL
    half = fn(c, s, weight=0.5)
    assert float(((half - c) * 2 - (full - c)).abs().max()) <= TOL    # linear in w
    assert torch.equal(fn(c, s, weight=0.0), c)


def test_adain_moves_the_statistics():
    c, s = _pair(40, B=2, R=64, Rr=128)
    s = 0.5 * s + 0.2
    a = color.adain_color_fix_reference(c, s)
    assert tuple(a.shape) == tuple(c.shape)
    dm = float((a.mean(dim=(-2, -1)) - s.mean(dim=(-2, -1))).abs().max())
    # std(a) = std(c) * sqrt(var(s) + eps) / sqrt(var(c) + eps): equal to std(s) up to eps / var terms, here 1e-5 / 0.08
    ds = float((a.std(dim=(-2, -1)) - s.std(dim=(-2, -1))).abs().max())
    print(f"AdaIN: mean off by {dm:.2e}, std off by {ds:.2e}")
    assert dm <= 1e-9
    want = c.std(dim=(-2, -1)) * ((s.var(dim=(-2, -1)) + 1e-5) / (c.var(dim=(-2, -1)) + 1e-5)).sqrt()
    assert float((a.std(dim=(-2, -1)) - want).abs().max()) <= 1e-9
    big = color.adain_color_fix_reference(c * 1e3, s * 1e3)           # sigma(c)^2 >> 1e-5: the planes take sigma(s) itself
    assert float((big.std(dim=(-2, -1)) / (s * 1e3).std(dim=(-2, -1)) - 1).abs().max()) <= 1e-9


def test_reference_preparation():
    c, s = _pair(50, B=1, R=64, Rr=128)
    s = s * 0.7 + 0.5                                                 # leaves [0, 1] on both sides
    import torch.nn.functional as F
    mapped = s.clamp(0, 1) * 2 - 1
    assert torch.equal(color.to_vae_range(s), mapped)
    got = color.wavelet_color_fix_reference(c, s, ref_vae_range=True)
    want = c + _B(F.interpolate(mapped, 64, mode="bicubic", align_corners=False) - c, 5)
    assert float((got - want).abs().max()) <= TOL
    got = color.adain_color_fix_reference(c, s, ref_vae_range=True)
    assert float((got.mean(dim=(-2, -1)) - mapped.mean(dim=(-2, -1))).abs().max()) <= 1e-9


def test_references_keep_dtype_and_device():
    c, s = _pair(60, B=1)
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        for fn in (color.wavelet_color_fix_reference, color.adain_color_fix_reference):
            y = fn(c.to(dt), s.to(dt))
            assert y.dtype == dt and tuple(y.shape) == tuple(c.shape)
