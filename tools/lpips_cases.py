"""The inputs, yardsticks and set-wide error functions that tests/test_lpips.py and tests/test_lpips_host.py assert on and
tools/lpips_bench.py records: hd_lpips on the GPU against `metrics.lpips_reference` in float64 on the CPU.  The yardstick is the error
of the contract's own number formats: the same reference with `emulate_bf16=True` (float64 arithmetic, rounded to bf16 where the
kernels round) against plain float64 on the same inputs, times the project's factor 4.  Errors are absolute: near-identical pairs score
about 1e-5, where a relative figure says nothing.  Every tensor is made once, from fixed seeds, and never changed."""
import collections
import functools

import torch
import torch.nn.functional as F

from hifidiff_amd import metrics, synth

Case = collections.namedtuple("Case", "name amp B R Rb input_normalize")

AMPS = (0.3, 0.05, 0.005)                                             # perturbation of the smooth base image
# B 1 at 64: the last three convolutions run 18 rows, less than one row tile; B 3 at 64: ragged last tiles everywhere (conv1: 1350 rows);
# 128: more than one block per face in the distance kernel; 192: tap sides 47 / 23 / 11, all odd; 64 -> 128 with per-face ranges
SHAPES = ((1, 64, 64, None), (3, 64, 64, None), (2, 128, 128, None), (1, 192, 192, None), (3, 64, 128, "face"))
CASES = [Case("amp%g-%dx%d%s" % (amp, B, R, "" if R == Rb else "to%d-%s" % (Rb, norm)), amp, B, R, Rb, norm)
         for amp in AMPS for (B, R, Rb, norm) in SHAPES]
FACTOR = 4.0                                                          # the project's factor on a yardstick


def _seed(*key):
    h = 0
    for ch in "/".join(str(k) for k in key):
        h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def family(amp, B, R, Rb, tag=""):
    """(images [B,3,R,R], ref [B,3,Rb,Rb]) in fp32, values in [0, 1]: ref is an 8x-upsampled random grid, images = ref + amp N clipped.
    The pair is made at Rb; images of another size are its bicubic resampling."""
    g = _seed(amp, B, R, Rb, tag)
    grid = torch.rand((B, 3, Rb // 8, Rb // 8), generator=g)
    ref = F.interpolate(grid, Rb, mode="bicubic", align_corners=False).clamp(0, 1)
    img = (ref + amp * torch.randn((B, 3, Rb, Rb), generator=g)).clamp(0, 1)
    if R != Rb:
        img = F.interpolate(img, R, mode="bicubic", align_corners=False)
    return img.contiguous(), ref.contiguous()


@functools.lru_cache(maxsize=None)
def state():
    return synth.lpips_state_dict()


@functools.lru_cache(maxsize=None)
def model():
    m = metrics.LPIPS()
    m.load_state_dict(state())
    return m.to("cuda:0")


def inputs(case):
    return family(case.amp, case.B, case.R, case.Rb, tag=case.name)


Ref = collections.namedtuple("Ref", "f64 f64_layers emu emu_layers")


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64 and the bf16 emulation of the case, on the CPU, computed once."""
    img, ref = inputs(case)
    kw = dict(normalize=True, input_normalize=case.input_normalize, per_layer=True)
    t, l = metrics.lpips_reference(state(), img.double(), ref.double(), **kw)
    te, le = metrics.lpips_reference(state(), img.double(), ref.double(), emulate_bf16=True, **kw)
    return Ref(t, l, te, le)


Run = collections.namedtuple("Run", "case got got_layers ref inputs_unchanged")


@functools.lru_cache(maxsize=None)
def run(case):
    """The case on the GPU next to its references, computed once."""
    img, ref = inputs(case)
    a, b = img.cuda(), ref.cuda()
    t, l = model()(a, b, normalize=True, input_normalize=case.input_normalize, per_layer=True)
    same = torch.equal(a.cpu(), img) and torch.equal(b.cpu(), ref)
    return Run(case, t.cpu(), l.cpu(), reference(case), same)


def score_errors(cases, layers=False):
    """Worst absolute error of the kernel and of the bf16 emulation against float64 over every face (layers: every d_k) of `cases`;
    the number of values; the smallest and largest float64 score."""
    k, y, n, lo, hi = 0.0, 0.0, 0, float("inf"), 0.0
    for c in cases:
        r = run(c)
        want, got, emu = (r.ref.f64_layers, r.got_layers, r.ref.emu_layers) if layers else (r.ref.f64, r.got, r.ref.emu)
        k = max(k, float((got - want).abs().max()))
        y = max(y, float((emu - want).abs().max()))
        n += int(want.numel())
        lo, hi = min(lo, float(want.min())), max(hi, float(want.max()))
    return k, y, n, lo, hi


def activity(case, st=None):
    """Per tapped layer the fraction of positive activations over both images of the case, and each layer's share of the mean score
    (float64, CPU): what makes the synthetic weights a test and not a formality."""
    st = state() if st is None else st
    img, ref = inputs(case)
    a, b = metrics.resample(img.double(), case.Rb), ref.double()
    x = torch.cat([metrics.lpips_prepare(st, a, None, True), metrics.lpips_prepare(st, b, None, True)])
    pos = [float((f > 0).double().mean()) for f in metrics.lpips_features(st, x)]
    _, layers = metrics.lpips_reference(st, img.double(), ref.double(), per_layer=True)
    share = layers.mean(dim=0) / layers.mean(dim=0).sum()
    return pos, [float(v) for v in share]


def report():
    """The measured errors against their yardsticks, as the lines tools/lpips_bench.py records."""
    lines = ["errors against lpips_reference in float64 (absolute; kernel | bf16 emulation in float64 = the yardstick; the bound is %g x the yardstick):" % FACTOR,
             "%-28s %-12s %-12s %-12s %s" % ("case (worst face)", "score f64", "kernel", "emulation", "kernel / yardstick")]
    for c in CASES:
        r = run(c)
        k, y = float((r.got - r.ref.f64).abs().max()), float((r.ref.emu - r.ref.f64).abs().max())
        lines.append("%-28s %-12.3e %-12.3e %-12.3e %.2f" % (c.name, float(r.ref.f64.max()), k, y, k / y if y else float("inf")))
    for label, layers in (("lpips", False), ("per-layer d_k", True)):
        k, y, n, lo, hi = score_errors(tuple(CASES), layers)
        lines.append("%s, worst of %d values in [%.2e, %.2e]: kernel %.3e, emulation %.3e (bound %.3e)" % (label, n, lo, hi, k, y, FACTOR * y))
    return lines
