"""The inputs and error measurements that tests/test_metrics.py asserts on and tools/metrics_bench.py records: hd_image_metrics /
hd_image_range on the GPU against the float64 formulas of hifidiff_amd.metrics on the CPU, with the same formulas evaluated in fp32 by
torch on the same inputs as the yardstick.  Every tensor is made once, from fixed seeds, and never changed."""
import collections
import functools

import torch
import torch.nn.functional as F

from hifidiff_amd import metrics

Case = collections.namedtuple("Case", "name family B R Rb channels L normalize")

# Rb 64: one tile; 128: a seam; 192: three tiles per side (a tile with neighbours all round).  B 1, 3, 5.  Both channel modes.  L 1 and 255
# (inputs scaled; with a normalisation the values are in [0, 1], so L = 1).  128 -> 64, 64 -> 128, 192 -> 64.  None / face / batch.
CASES = [
    Case("noise-1x64-rgb", "noise", 1, 64, 64, "rgb", 1.0, None),
    Case("noise-3x128-y-255", "noise", 3, 128, 128, "y", 255.0, None),
    Case("smooth-5x192-rgb", "smooth", 5, 192, 192, "rgb", 1.0, None),
    Case("patch-3x128-rgb-255", "patch", 3, 128, 128, "rgb", 255.0, None),
    Case("patch-1x192-y", "patch", 1, 192, 192, "y", 1.0, None),
    Case("smooth-5x128-y", "smooth", 5, 128, 128, "y", 1.0, None),
    Case("smooth-3x128to64-y", "smooth", 3, 128, 64, "y", 1.0, None),
    Case("noise-3x64to128-rgb-255", "noise", 3, 64, 128, "rgb", 255.0, None),
    Case("patch-5x192to64-y-face", "patch", 5, 192, 64, "y", 1.0, "face"),
    Case("smooth-3x64-rgb-face", "smooth", 3, 64, 64, "rgb", 1.0, "face"),
    Case("noise-3x128-y-batch", "noise", 3, 128, 128, "y", 1.0, "batch"),
    Case("patch-5x64to128-rgb-batch", "patch", 5, 64, 128, "rgb", 1.0, "batch"),
]
PLAIN_MSE = [c for c in CASES if c.channels == "rgb" and c.R == c.Rb and c.normalize is None]      # the derived 8 * 2^-24 bound
OTHER_MSE = [c for c in CASES if c not in PLAIN_MSE]                                                # y, resampled or normalised
FACTOR = 4.0                                                          # the project's factor on a torch-fp32 yardstick
PLAIN_MSE_BOUND = 8.0 * 2.0 ** -24                                    # one rounding in a - b, up to two more in the square; fp64 sums


def _seed(*key):
    h = 0
    for ch in "/".join(str(k) for k in key):
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def family(name, B, R, Rb, L=1.0, tag=""):
    """(images [B,3,R,R], ref [B,3,Rb,Rb]) in fp32, values in [0, L].  The pair is made at Rb; images of another size are its bicubic
    resampling (any input will do: the kernel resamples it back).
      noise:  uniform noise against noise + 0.1 N clipped
      smooth: an 8x-upsampled random grid against itself + 0.05 N
      patch:  the smooth image with a constant 32 x 32 patch, and noise on the right half only: a sigma ~ 0 region and a seam"""
    g = _seed(name, B, R, Rb, tag)
    if name == "noise":
        ref = torch.rand((B, 3, Rb, Rb), generator=g)
        img = (ref + 0.1 * torch.randn((B, 3, Rb, Rb), generator=g)).clamp(0, 1)
    else:
        grid = torch.rand((B, 3, Rb // 8, Rb // 8), generator=g)
        ref = F.interpolate(grid, Rb, mode="bicubic", align_corners=False).clamp(0, 1)
        n = 0.05 * torch.randn((B, 3, Rb, Rb), generator=g)
        if name == "patch":
            ref[:, :, 8:40, 12:44] = 0.375
            n[..., : Rb // 2] = 0
        img = (ref + n).clamp(0, 1)
    if R != Rb:
        img = F.interpolate(img, R, mode="bicubic", align_corners=False)
    return (img * L).contiguous(), (ref * L).contiguous()


Run = collections.namedtuple("Run", "case images ref got f64 f32 inputs_unchanged")


@functools.lru_cache(maxsize=None)
def run(case):
    """The case on the GPU (map included), its float64 reference and the fp32 yardstick, computed once."""
    img, ref = family(case.family, case.B, case.R, case.Rb, case.L, tag=case.name)
    kw = dict(channels=case.channels, data_range=case.L, normalize=case.normalize, ssim_map=True)
    a, b = img.cuda(), ref.cuda()
    got = metrics.image_metrics(a, b, **kw)
    got = metrics.Metrics(*(None if t is None else t.cpu() for t in got))
    same = torch.equal(a.cpu(), img) and torch.equal(b.cpu(), ref)
    return Run(case, img, ref, got, metrics.image_metrics_reference(img.double(), ref.double(), **kw),
               metrics.image_metrics_reference(img, ref, **kw), same)


def map_errors(r):
    """(max |kernel - f64|, max |torch fp32 - f64|) over the map's pixels."""
    return float((r.got.ssim_map.double() - r.f64.ssim_map).abs().max()), float((r.f32.ssim_map.double() - r.f64.ssim_map).abs().max())


def score_errors(cases, what):
    """Worst error of the kernel and of torch fp32 over every face of `cases`: "ssim" absolute, "mse" relative; and the number of values."""
    k, y, n = 0.0, 0.0, 0
    for c in cases:
        r = run(c)
        want = getattr(r.f64, what)
        scale = want if what == "mse" else torch.ones_like(want)
        k = max(k, float(((getattr(r.got, what).double() - want).abs() / scale).max()))
        y = max(y, float(((getattr(r.f32, what).double() - want).abs() / scale).max()))
        n += int(want.numel())
    return k, y, n


RANGE_SETS = [(fam, R, Ro) for fam in ("noise", "smooth", "patch") for (R, Ro) in ((128, 64), (64, 128), (192, 64))]


@functools.lru_cache(maxsize=None)
def range_errors():
    """hd_image_range with resampling: worst absolute error of the kernel and of torch fp32 against float64 over the set (36 values)."""
    k, y, n = 0.0, 0.0, 0
    for fam, R, Ro in RANGE_SETS:
        img, _ = family(fam, 2, R, R, 1.0, tag="range")
        img = img * 1.5 - 0.25                                        # some values outside [0, 1]
        want = metrics.range_reference(img.double(), Ro)
        k = max(k, float((metrics.image_range(img.cuda(), Ro).cpu().double() - want).abs().max()))
        y = max(y, float((metrics.range_reference(img, Ro).double() - want).abs().max()))
        n += int(want.numel())
    return k, y, n


def report():
    """The measured errors against their yardsticks, as the lines tools/metrics_bench.py records."""
    lines = ["errors against the float64 formulas (kernel | torch fp32 on the same inputs = the yardstick; the bound is %g x the yardstick):" % FACTOR,
             "%-28s %-12s %-12s %s" % ("SSIM map, per case", "kernel", "torch fp32", "kernel / yardstick")]
    for c in CASES:
        k, y = map_errors(run(c))
        lines.append("%-28s %-12.3e %-12.3e %.2f" % (c.name, k, y, k / y if y else float("inf")))
    for label, cases, what in (("per-face SSIM (abs)", CASES, "ssim"), ("MSE, y / resampled / normalised (rel)", OTHER_MSE, "mse")):
        k, y, n = score_errors(tuple(cases), what)
        lines.append("%s, worst of %d values: kernel %.3e, torch fp32 %.3e" % (label, n, k, y))
    k, y, n = range_errors()
    lines.append("hd_image_range with resampling (abs), worst of %d values: kernel %.3e, torch fp32 %.3e" % (n, k, y))
    for c in PLAIN_MSE:
        r = run(c)
        lines.append("MSE, plain rgb, %s: kernel rel %.3e (bound 8 * 2^-24 = %.3e), torch fp32 rel %.3e" % (
            c.name, float(((r.got.mse - r.f64.mse).abs() / r.f64.mse).max()), PLAIN_MSE_BOUND, float(((r.f32.mse.double() - r.f64.mse).abs() / r.f64.mse).max())))
    return lines
