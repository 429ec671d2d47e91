"""Host side of the image metrics (no GPU): the exports, the argument checks of hd_image_metrics / hd_image_range that come before any
HIP call, the Python argument checks, and the reference formulas of hifidiff_amd.metrics in float64 against independent statements."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hifidiff_amd import _lib, metrics

HD_ERR_INVALID = -1                                                   # include/hifidiff_hip.h
TOL = 1e-12                                                           # float64 against float64, values of magnitude <= 1


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rand(seed, shape):
    return torch.rand(shape, generator=_g(seed), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ exports and argument checks
def test_the_entry_points_are_exported():
    with open(_lib.HEADER) as fh:
        header = fh.read()
    for name, decl in (("hd_image_range", "int hd_image_range("), ("hd_image_metrics", "int hd_image_metrics("),
                       ("hd_image_metrics_workspace", "int64_t hd_image_metrics_workspace(")):
        assert name in _lib.EXPORTS
        assert decl in header
        assert hasattr(_lib.lib(), name)


def test_workspace_size():
    L = _lib.lib()
    assert L.hd_image_metrics_workspace(1, 64, 2) == 16               # one tile, one plane: two fp64 sums
    assert L.hd_image_metrics_workspace(5, 192, 1) == 5 * 3 * 9 * 16
    assert L.hd_image_metrics_workspace(64, 512, 2) == 64 * 64 * 16
    for args, name in (((0, 64, 1), "batch"), ((1, 96, 1), "ref_res"), ((1, 64, 3), "channels")):
        assert L.hd_image_metrics_workspace(*args) == HD_ERR_INVALID
        msg = L.hd_last_error(None).decode()
        assert msg.startswith("hd_image_metrics_workspace:") and name in msg, msg


# made-up addresses, far enough apart for batch 2 at 512 px (12 MiB per tensor)
IMG, REF, IRG, RRG, OUT, MAP, WS = 0x10000000, 0x20000000, 0x30000000, 0x30001000, 0x40000000, 0x50000000, 0x60000000
N64 = 2 * 3 * 64 * 64 * 4                                             # bytes of [2,3,64,64] fp32
WSB = 2 * 3 * 1 * 16                                                  # workspace of batch 2, 64 px, rgb
NAN, INF = float("nan"), float("inf")

#         images res ref  ref_res batch ch  L    images_range ref_range out  map  ws  ws_bytes    the argument the message names
M_BAD = [
    ((IMG, 64, REF, 64, 0, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "batch"),
    ((IMG, 64, REF, 64, -2, 2, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "batch"),
    ((IMG, 64, REF, 64, 70000, 2, 1.0, IRG, RRG, OUT, MAP, WS, 1 << 40), "batch"),
    ((IMG, 0, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), " res"),
    ((IMG, 96, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), " res"),
    ((IMG, 576, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), " res"),
    ((IMG, 64, REF, 32, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "ref_res"),
    ((IMG, 64, REF, 100, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "ref_res"),
    ((IMG, 64, REF, 1024, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, 1 << 30), "ref_res"),
    ((IMG, 64, REF, 64, 2, 0, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "channels"),
    ((IMG, 64, REF, 64, 2, 3, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "channels"),
    ((IMG, 64, REF, 64, 2, 1, 0.0, IRG, RRG, OUT, MAP, WS, WSB), "data_range"),
    ((IMG, 64, REF, 64, 2, 1, -1.0, IRG, RRG, OUT, MAP, WS, WSB), "data_range"),
    ((IMG, 64, REF, 64, 2, 2, NAN, IRG, RRG, OUT, MAP, WS, WSB), "data_range"),
    ((IMG, 64, REF, 64, 2, 2, INF, IRG, RRG, OUT, MAP, WS, WSB), "data_range"),
    ((None, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "images is NULL"),
    ((IMG, 64, None, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "ref is NULL"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, None, MAP, WS, WSB), "out is NULL"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, None, WSB), "workspace is NULL"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB - 1), "workspace_bytes"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, 0), "workspace_bytes"),
    ((IMG, 64, REF, 128, 2, 2, 1.0, IRG, RRG, OUT, MAP, WS, 2 * 4 * 16 - 16), "workspace_bytes"),    # sized by ref_res, not res
    ((IMG + 2, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "4 bytes"),
    ((IMG, 64, REF + 1, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS, WSB), "4 bytes"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG + 2, RRG, OUT, MAP, WS, WSB), "4 bytes"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG + 3, OUT, MAP, WS, WSB), "4 bytes"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP + 2, WS, WSB), "4 bytes"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT + 4, MAP, WS, WSB), "8 bytes"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, WS + 4, WSB), "8 bytes"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, IMG, MAP, WS, WSB), "out overlaps images"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, IMG + N64 - 8, MAP, WS, WSB), "out overlaps images"),    # the last bytes of images
    ((IMG, 64, REF, 128, 2, 1, 1.0, IRG, RRG, REF + 4 * N64 - 8, MAP, WS, 2 * 3 * 4 * 16), "out overlaps ref"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, IRG + 8, MAP, WS, WSB), "out overlaps images_range"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, RRG - 24, MAP, WS, WSB), "out overlaps ref_range"),      # the last bytes of out
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, IMG, WS, WSB), "ssim_map_out overlaps images"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, REF - 2 * 3 * 54 * 54 * 4 + 4, WS, WSB), "ssim_map_out overlaps ref"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, IMG + 64, WSB), "workspace overlaps images"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, REF + N64 - 8, WSB), "workspace overlaps ref"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, RRG, WSB), "workspace overlaps ref_range"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, MAP, OUT + 8, WSB), "out overlaps workspace"),
    ((IMG, 64, REF, 64, 2, 1, 1.0, IRG, RRG, OUT, OUT, WS, WSB), "out overlaps ssim_map_out"),
]


@pytest.mark.parametrize("args,names", M_BAD, ids=["%d-%s" % (i, n.strip().replace(" ", "_")) for i, (_, n) in enumerate(M_BAD)])
def test_bad_metrics_arguments_are_refused_before_any_device_work(args, names):
    L = _lib.lib()
    rc = L.hd_image_metrics(*args, None)
    msg = L.hd_last_error(None).decode()
    assert rc == HD_ERR_INVALID, (rc, msg)
    assert msg.startswith("hd_image_metrics:") and names in msg, msg


#         images batch res out_res range_out
R_BAD = [
    ((IMG, 0, 64, 64, OUT), "batch"),
    ((IMG, -1, 64, 64, OUT), "batch"),
    ((IMG, 2, 32, 64, OUT), " res"),
    ((IMG, 2, 640, 64, OUT), " res"),
    ((IMG, 2, 64, 0, OUT), "out_res"),
    ((IMG, 2, 64, 100, OUT), "out_res"),
    ((None, 2, 64, 64, OUT), "images is NULL"),
    ((IMG, 2, 64, 64, None), "range_out is NULL"),
    ((IMG + 4, 2, 64, 64, OUT), "16 bytes"),                          # float4 loads when nothing is resampled
    ((IMG + 2, 2, 128, 64, OUT), "4 bytes"),
    ((IMG, 2, 64, 64, OUT + 2), "4 bytes"),
    ((IMG, 2, 64, 64, IMG), "range_out overlaps images"),
    ((IMG, 2, 64, 64, IMG + N64 - 4), "range_out overlaps images"),
    ((IMG, 2, 64, 128, IMG - 12), "range_out overlaps images"),
]


@pytest.mark.parametrize("args,names", R_BAD, ids=["%d-%s" % (i, n.strip().replace(" ", "_")) for i, (_, n) in enumerate(R_BAD)])
def test_bad_range_arguments_are_refused_before_any_device_work(args, names):
    L = _lib.lib()
    rc = L.hd_image_range(*args, None)
    msg = L.hd_last_error(None).decode()
    assert rc == HD_ERR_INVALID, (rc, msg)
    assert msg.startswith("hd_image_range:") and names in msg, msg


def test_python_argument_checks():
    a, b = torch.zeros((2, 3, 64, 64)), torch.zeros((2, 3, 128, 128))
    for kw in (dict(channels="luma"), dict(channels=1), dict(data_range=0), dict(data_range=-1.0), dict(data_range=float("nan")),
               dict(data_range=float("inf")), dict(data_range="1"), dict(data_range=True), dict(normalize="tensor"), dict(normalize=True)):
        with pytest.raises(ValueError):
            metrics.image_metrics(a, b, **kw)
        with pytest.raises(ValueError):
            metrics.image_metrics_reference(a, b, **kw)
    for ai, bi in ((a[:, :2], b), (a, b[:1]), (torch.zeros((2, 3, 96, 96)), b), (a, torch.zeros((2, 3, 64, 128))), (a[0], b), (a.numpy(), b),
                   (torch.zeros((2, 3, 576, 576)), b)):
        with pytest.raises(ValueError):
            metrics.image_metrics(ai, bi)
    for size in (0, 96, 1024, 64.0, True):
        with pytest.raises(ValueError):
            metrics.image_range(a, size)
    with pytest.raises(ValueError):
        metrics.image_range(a[:, :1])
    with pytest.raises(RuntimeError):                                 # well-formed, but no CPU path exists
        metrics.image_metrics(a, b)
    with pytest.raises(RuntimeError):
        metrics.image_range(a)
    with pytest.raises(RuntimeError):
        metrics.evaluate(a, b)
    with pytest.raises(ValueError):
        metrics.ssim_map_reference(a, b)                              # the references score equal shapes
    with pytest.raises(ValueError):
        metrics.rgb_to_y(a[:, :2])


# ------------------------------------------------------------------------------------------------ the formulas, float64
def test_window():
    g = metrics.gaussian_window()
    assert g.dtype == torch.float64 and tuple(g.shape) == (11,)
    want = [math.exp(-((k - 5) ** 2) / (2 * 1.5 ** 2)) for k in range(11)]
    assert float((g - torch.tensor(want, dtype=torch.float64) / sum(want)).abs().max()) <= 1e-16
    assert abs(float(g.sum()) - 1.0) <= 1e-15 and torch.equal(g, g.flip(0))
    assert metrics.gaussian_window(torch.float32).dtype == torch.float32


def test_blur_is_scipys_gaussian_filter_on_the_interior():
    """The same eleven taps: sigma 1.5 truncated at 3.5 sigma = radius 5.  scipy pads the border; the valid positions are its interior."""
    from scipy.ndimage import gaussian_filter
    x = _rand(1, (2, 3, 48, 40))
    got = metrics.window_blur(x)
    assert tuple(got.shape) == (2, 3, 38, 30)
    for f in range(2):
        for c in range(3):
            want = gaussian_filter(x[f, c].numpy(), 1.5, truncate=3.5)[5:-5, 5:-5]
            err = float(np.abs(got[f, c].numpy() - want).max())
            assert err <= TOL, (f, c, err)


@pytest.mark.parametrize("L", [1.0, 255.0])
def test_constant_images(L):
    c1, c2 = 0.25 * L, 0.75 * L
    a, b = torch.full((1, 3, 32, 32), c1, dtype=torch.float64), torch.full((1, 3, 32, 32), c2, dtype=torch.float64)
    C1 = (0.01 * L) ** 2
    want = (2 * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1)
    m = metrics.ssim_map_reference(a, b, L)
    assert tuple(m.shape) == (1, 3, 22, 22)
    assert float((m - want).abs().max()) <= TOL                       # sigma terms vanish up to the rounding of E[x^2] - mu^2
    assert abs(float(metrics.ssim_reference(a, b, L)) - want) <= TOL
    assert abs(float(metrics.mse_reference(a, b)) / (c1 - c2) ** 2 - 1) <= TOL


def test_identity_and_offset():
    a = _rand(2, (2, 3, 64, 64))
    assert float((metrics.ssim_reference(a, a.clone()) - 1).abs().max()) <= TOL
    assert torch.equal(metrics.mse_reference(a, a.clone()), torch.zeros(2, dtype=torch.float64))
    p = metrics.psnr_reference(a, a.clone())
    assert bool(torch.isinf(p).all()) and bool((p > 0).all())
    for L, delta in ((1.0, 0.125), (255.0, 2.0), (1.0, 1e-3)):
        got = metrics.psnr_reference(a * L, a * L + delta, L)
        assert float((got - 20 * math.log10(L / delta)).abs().max()) <= 1e-9, (L, delta)


def test_ssim_symmetry_and_scale_invariance():
    a, b = _rand(3, (2, 3, 64, 64)), _rand(4, (2, 3, 64, 64))
    m = metrics.ssim_map_reference(a, b)
    assert float((m - metrics.ssim_map_reference(b, a)).abs().max()) <= TOL
    assert float((m - metrics.ssim_map_reference(a * 255, b * 255, 255.0)).abs().max()) <= 1e-11
    assert float((metrics.ssim_reference(a, b) - metrics.ssim_reference(a * 7, b * 7, 7.0)).abs().max()) <= 1e-11
    assert float(m.max()) <= 1 + TOL
    y = metrics.rgb_to_y(a)
    assert tuple(y.shape) == (2, 1, 64, 64)
    assert float((y - (65.481 * a[:, 0] + 128.553 * a[:, 1] + 24.966 * a[:, 2] + 16) [:, None] / 255).abs().max()) <= TOL
    assert float((metrics.rgb_to_y(a * 255, 255.0) - 255 * y).abs().max()) <= 1e-10     # luma scales with L
    one = torch.ones((1, 3, 8, 8), dtype=torch.float64)
    assert abs(float(metrics.rgb_to_y(one).max()) - 235 / 255) <= TOL and abs(float(metrics.rgb_to_y(0 * one).max()) - 16 / 255) <= TOL


def test_ssim_map_from_the_definition():
    """One map position from a dense 11 x 11 window, without any convolution."""
    a, b = _rand(5, (1, 1, 24, 24)), _rand(6, (1, 1, 24, 24))
    g = metrics.gaussian_window()
    W = g[:, None] * g[None, :]
    m = metrics.ssim_map_reference(a, b)
    for (y, x) in ((0, 0), (13, 0), (7, 9), (13, 13)):
        pa, pb = a[0, 0, y:y + 11, x:x + 11], b[0, 0, y:y + 11, x:x + 11]
        mua, mub = (W * pa).sum(), (W * pb).sum()
        va, vb, cab = (W * pa * pa).sum() - mua ** 2, (W * pb * pb).sum() - mub ** 2, (W * pa * pb).sum() - mua * mub
        want = (2 * mua * mub + 1e-4) * (2 * cab + 9e-4) / ((mua ** 2 + mub ** 2 + 1e-4) * (va + vb + 9e-4))
        assert abs(float(m[0, 0, y, x] - want)) <= TOL, (y, x)


def test_range_reference():
    x = _rand(7, (3, 3, 128, 128)) * 3 - 1
    r = metrics.range_reference(x)
    assert tuple(r.shape) == (3, 2)
    assert torch.equal(r[:, 0], x.amin(dim=(1, 2, 3))) and torch.equal(r[:, 1], x.amax(dim=(1, 2, 3)))
    assert torch.equal(metrics.range_reference(x, 128), r)
    for size in (64, 192):
        y = F.interpolate(x, size, mode="bicubic", align_corners=False)
        r = metrics.range_reference(x, size)
        assert torch.equal(r[:, 0], y.amin(dim=(1, 2, 3))) and torch.equal(r[:, 1], y.amax(dim=(1, 2, 3)))
    n = metrics.normalize_reference(x, metrics.range_reference(x))
    assert float(n.amin()) == 0.0 and abs(float(n.amax()) - 1.0) <= TOL
    flat = torch.full((1, 3, 8, 8), 0.5, dtype=torch.float64)
    assert torch.equal(metrics.normalize_reference(flat, metrics.range_reference(flat)), torch.zeros_like(flat))   # hi <= lo: 0, not NaN


def test_evaluate_is_the_reference_loops_composition():
    result, target = _rand(8, (3, 3, 64, 64)) * 2.4 - 1.2, _rand(9, (3, 3, 128, 128))
    r = F.interpolate(result, 128, mode="bicubic")
    rn = (r - r.min()) / (r.max() - r.min())
    tn = (target - target.min()) / (target.max() - target.min())
    psnr = 10 * torch.log10(1.0 / ((rn - tn) ** 2).mean(dim=(1, 2, 3)))
    y = lambda t: ((65.481 * t[:, 0] + 128.553 * t[:, 1] + 24.966 * t[:, 2] + 16) / 255)[:, None]   # noqa: E731
    ssim = metrics.ssim_map_reference(y(rn), y(tn)).mean(dim=(1, 2, 3))
    for got in (metrics.evaluate_reference(result, target),
                (metrics.image_metrics_reference(result, target, "rgb", normalize="batch").psnr,
                 metrics.image_metrics_reference(result, target, "y", normalize="batch").ssim)):
        assert float((got[0] - psnr).abs().max()) <= 1e-10 and float((got[1] - ssim).abs().max()) <= TOL
    face = metrics.image_metrics_reference(result, target, "rgb", normalize="face", ssim_map=True)
    rf = torch.stack([(r[i] - r[i].min()) / (r[i].max() - r[i].min()) for i in range(3)])
    tf = torch.stack([(target[i] - target[i].min()) / (target[i].max() - target[i].min()) for i in range(3)])
    assert float((face.mse - ((rf - tf) ** 2).mean(dim=(1, 2, 3))).abs().max()) <= TOL
    assert tuple(face.ssim_map.shape) == (3, 3, 118, 118)
    assert float((face.ssim_map - metrics.ssim_map_reference(rf, tf)).abs().max()) <= TOL


def test_references_keep_dtype():
    a, b = _rand(10, (1, 3, 64, 64)), _rand(11, (1, 3, 64, 64))
    for dt in (torch.float32, torch.float64):
        m = metrics.image_metrics_reference(a.to(dt), b.to(dt), "y", ssim_map=True)
        assert m.mse.dtype == dt and m.ssim.dtype == dt and m.ssim_map.dtype == dt and tuple(m.ssim_map.shape) == (1, 1, 54, 54)
        assert metrics.range_reference(a.to(dt)).dtype == dt
