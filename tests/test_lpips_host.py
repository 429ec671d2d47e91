"""Host side of LPIPS (no GPU): the manifest and the exports, the state-dict plumbing of `metrics.LPIPS`, `metrics.lpips_reference` in
float64 against an independently written AlexNet, and that the synthetic weights make the GPU tests a test: on the families of
tools/lpips_cases.py every tapped layer is about half active and contributes to the score."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

from hifidiff_amd import _lib, arch, metrics, synth      # noqa: E402

TOL = 1e-12                                               # float64 against float64, scores of magnitude <= 1


def _lc():
    import lpips_cases
    return lpips_cases


def _pair(seed, B, R, Rb=None, amp=0.1):
    g = torch.Generator().manual_seed(seed)
    ref = torch.rand((B, 3, Rb or R, Rb or R), generator=g, dtype=torch.float64)
    img = (F.interpolate(ref, R, mode="bicubic", align_corners=False) if Rb and Rb != R else ref) + amp * torch.randn((B, 3, R, R), generator=g, dtype=torch.float64)
    return img, ref


# ------------------------------------------------------------------------------------------------ manifest, exports, state dict
def test_manifest_and_exports():
    man, sd = arch.lpips_manifest(), synth.lpips_state_dict()
    assert list(man) == list(sd) and len(man) == 15
    for k, (shape, _, _) in man.items():
        assert tuple(sd[k].shape) == tuple(shape) and sd[k].dtype == torch.float32, k
    want = {"net.slice1.0.weight": (64, 3, 11, 11), "net.slice2.3.weight": (192, 64, 5, 5), "net.slice3.6.weight": (384, 192, 3, 3),
            "net.slice4.8.weight": (256, 384, 3, 3), "net.slice5.10.weight": (256, 256, 3, 3), "net.slice2.3.bias": (192,),
            "lin0.model.1.weight": (1, 64, 1, 1), "lin2.model.1.weight": (1, 384, 1, 1), "lin4.model.1.weight": (1, 256, 1, 1)}
    for k, shape in want.items():
        assert tuple(man[k][0]) == shape, k
    for k in range(5):
        w, C = sd["lin%d.model.1.weight" % k], man["lin%d.model.1.weight" % k][0][1]
        assert float(w.min()) >= 0.0 and float(w.max()) < 4.0 / C and float(w.mean()) > 1.0 / C      # non-negative, uniform on [0, 4 / C)
    with open(_lib.HEADER) as fh:
        header = fh.read()
    for name, decl in (("hd_lpips_create", "int hd_lpips_create("), ("hd_lpips", "int hd_lpips(")):
        assert name in _lib.EXPORTS and decl in header and hasattr(_lib.lib(), name)
    assert arch.lpips_sides(64) == (15, 7, 3) and arch.lpips_sides(128) == (31, 15, 7) and arch.lpips_sides(192) == (47, 23, 11)


def test_load_state_dict_is_strict():
    sd = synth.lpips_state_dict()
    m = metrics.LPIPS()
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys and set(m.state_dict()) == set(sd)
    short = dict(sd); del short["lin3.model.1.weight"]
    with pytest.raises(RuntimeError, match=r"Missing key\(s\): \['lin3.model.1.weight'\]"):
        metrics.LPIPS().load_state_dict(short)
    extra = dict(sd); extra["net.slice6.12.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match=r"Unexpected key\(s\): \['net.slice6.12.weight'\]"):
        metrics.LPIPS().load_state_dict(extra)
    bad = dict(sd); bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(RuntimeError, match="size mismatch for net.slice2.3.weight"):
        metrics.LPIPS().load_state_dict(bad)
    half = dict(sd); half["scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)          # the scaling constants: both or neither
    with pytest.raises(RuntimeError, match="scaling_layer.scale"):
        metrics.LPIPS().load_state_dict(half)
    loose = metrics.LPIPS().load_state_dict(short, strict=False)
    assert loose.missing_keys == ["lin3.model.1.weight"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.to("cpu")


def test_aliases_load_to_the_same_state(tmp_path):
    sd = synth.lpips_state_dict()
    feats = {"features.%s" % k.split(".", 2)[2]: v for k, v in sd.items() if k.startswith("net.")}        # a torchvision AlexNet file
    assert set(feats) == {"features.%d.%s" % (i, p) for i in (0, 3, 6, 8, 10) for p in ("weight", "bias")}
    feats["classifier.1.weight"] = torch.zeros(8, 8)
    feats["classifier.1.bias"] = torch.zeros(8)
    lins = {"lins.%s" % k[3:]: v for k, v in sd.items() if k.startswith("lin")}
    assert "lins.0.model.1.weight" in lins
    a, b, c = metrics.LPIPS(), metrics.LPIPS(), metrics.LPIPS()
    a.load_state_dict(sd)
    b.load_state_dict({**feats, **lins})
    c.load_state_dict({**feats, **{k: v for k, v in sd.items() if k.startswith("lin")}})
    for other in (b, c):
        got = other.state_dict()
        assert list(got) == list(a.state_dict()) and all(torch.equal(got[k], sd[k]) for k in sd)
    pa, pl = str(tmp_path / "alexnet.pth"), str(tmp_path / "lin.pth")
    torch.save(feats, pa); torch.save(lins, pl)
    d = metrics.LPIPS.from_files(pa, pl).state_dict()
    assert all(torch.equal(d[k], sd[k]) for k in sd) and len(d) == len(sd)


# ------------------------------------------------------------------------------------------------ the reference formula
def test_reference_properties():
    sd = synth.lpips_state_dict()
    img, ref = _pair(1, 2, 64)
    t, layers = metrics.lpips_reference(sd, img, ref, per_layer=True)
    assert t.dtype == torch.float64 and tuple(t.shape) == (2,) and tuple(layers.shape) == (2, 5)
    assert bool((layers > 0).all()) and float((layers.sum(dim=1) - t).abs().max()) <= TOL * float(t.max())
    assert torch.equal(metrics.lpips_reference(sd, img, ref), t)
    for emulate in (False, True):
        z, zl = metrics.lpips_reference(sd, img, img.clone(), per_layer=True, emulate_bf16=emulate)
        assert torch.equal(z, torch.zeros(2, dtype=torch.float64)) and torch.equal(zl, torch.zeros((2, 5), dtype=torch.float64))
        assert torch.equal(metrics.lpips_reference(sd, ref, img, emulate_bf16=emulate), metrics.lpips_reference(sd, img, ref, emulate_bf16=emulate))
    u = metrics.lpips_reference(sd, 2 * img - 1, 2 * ref - 1, normalize=False)
    assert float((u - t).abs().max()) <= TOL
    e = metrics.lpips_reference(sd, img, ref, emulate_bf16=True)
    assert 0 < float((e - t).abs().max()) < 0.02 * float(t.max())                     # it rounds, and only that
    own = dict(sd); own["scaling_layer.shift"] = torch.tensor([0.1, 0.0, -0.1]).reshape(1, 3, 1, 1); own["scaling_layer.scale"] = torch.full((1, 3, 1, 1), 0.5)
    assert float((metrics.lpips_reference(own, img, ref) - t).abs().max()) > 1e-6      # the state dict's own constants are used
    with pytest.raises(ValueError, match="input_normalize"):
        metrics.lpips_reference(sd, img, ref, input_normalize="image")


class _Scaling(nn.Module):
    def forward(self, x):
        return (x - torch.tensor([-.030, -.088, -.188], dtype=x.dtype)[None, :, None, None]) / torch.tensor([.458, .448, .450], dtype=x.dtype)[None, :, None, None]


def _independent_lpips(sd, x0, x1, ranges=None):
    """torchvision's AlexNet `features` as an nn.Sequential, tapped after each ReLU, and Zhang et al.'s distance, written without
    hifidiff_amd.metrics."""
    net = nn.Sequential(nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(), nn.MaxPool2d(3, 2), nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(), nn.MaxPool2d(3, 2),
                        nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(), nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(), nn.Conv2d(256, 256, 3, padding=1), nn.ReLU()).double()
    net.load_state_dict({k.split(".", 2)[2]: v.double() for k, v in sd.items() if k.startswith("net.")})
    taps, total = (1, 4, 7, 9, 11), 0
    if ranges is not None:
        x0, x1 = ((x - lo) / (hi - lo) for x, (lo, hi) in zip((x0, x1), ranges))
    h0, h1 = _Scaling()(2 * x0 - 1), _Scaling()(2 * x1 - 1)
    with torch.no_grad():
        for i, layer in enumerate(net):
            h0, h1 = layer(h0), layer(h1)
            if i in taps:
                k = taps.index(i)
                n0 = h0 / (torch.sqrt(torch.sum(h0 ** 2, dim=1, keepdim=True)) + 1e-10)
                n1 = h1 / (torch.sqrt(torch.sum(h1 ** 2, dim=1, keepdim=True)) + 1e-10)
                lin = F.conv2d((n0 - n1) ** 2, sd["lin%d.model.1.weight" % k].double())
                total = total + lin.mean(dim=(2, 3))[:, 0]
    return total


@pytest.mark.parametrize("R", [64, 128])
def test_reference_against_an_independent_alexnet(R):
    sd = synth.lpips_state_dict()
    img, ref = _pair(R, 2, R)
    want = _independent_lpips(sd, img, ref)
    got = metrics.lpips_reference(sd, img, ref)
    assert float(want.min()) > 1e-3 and float((got - want).abs().max()) <= TOL
    # resampled, batch-normalised: val_loop's lines
    small, _ = _pair(R + 1, 2, 64, R)
    up = F.interpolate(small, R, mode="bicubic", align_corners=False) if R != 64 else small
    want = _independent_lpips(sd, up, ref, ranges=((up.min(), up.max()), (ref.min(), ref.max())))
    got = metrics.lpips_reference(sd, small, ref, input_normalize="batch")
    assert float((got - want).abs().max()) <= TOL


# ------------------------------------------------------------------------------------------------ the synthetic weights are a test
def test_synthetic_weights_are_not_vacuous():
    lc = _lc()
    assert len(lc.CASES) == 15 and sum(c.B for c in lc.CASES) >= 30 and {c.amp for c in lc.CASES} == {0.3, 0.05, 0.005}
    assert {(c.B, c.Rb) for c in lc.CASES if c.R == c.Rb} == {(1, 64), (3, 64), (2, 128), (1, 192)}
    for c in lc.CASES:
        pos, share = lc.activity(c)
        print(c.name, "positive", ["%.2f" % p for p in pos], "share", ["%.3f" % s for s in share])
        assert all(0.25 <= p <= 0.75 for p in pos), (c.name, pos)
        assert all(s >= 0.01 for s in share), (c.name, share)


# ------------------------------------------------------------------------------------------------ what stays as it was
def test_metrics_tuple_and_evaluate_reference_are_unchanged():
    m = metrics.Metrics(1, 2, 3, 4)
    assert m.lpips is None and tuple(m)[:4] == (1, 2, 3, 4) and m.ssim_map == 4
    assert metrics.Metrics(1, 2, 3, 4, 5).lpips == 5 and metrics.Metrics._fields == ("mse", "psnr", "ssim", "ssim_map", "lpips")
    e = metrics.Evaluation(1, 2)
    assert e.lpips is None and (e.psnr, e.ssim) == (1, 2)
    img, ref = _pair(5, 2, 64)
    ev = metrics.evaluate_reference(img, ref)
    rn, tn = (img - img.min()) / (img.max() - img.min()), (ref - ref.min()) / (ref.max() - ref.min())
    assert ev.lpips is None
    assert float((ev.psnr - metrics.psnr_reference(rn, tn)).abs().max()) <= 1e-9
    assert float((ev.ssim - metrics.ssim_reference(metrics.rgb_to_y(rn), metrics.rgb_to_y(tn))).abs().max()) <= TOL
    r = metrics.image_metrics_reference(img, ref)
    assert r.lpips is None and len(r) == 5
