"""CPU side of per-face schedule positions: sampling.img2img_start against diffusers' img2img convention restated in float64, and an ISA
lint of the per-face instantiations (hd_sample_rows*) of the persistent stages and the step's last launch (xcd_rows_stage_kernel<512, 16>
carries 1 spilled register, as its shared-row form carries 3: test_isa_lint.py leaves that form out too)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


def _sched(n):
    from hifidiff_amd import schedulers
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(n)
    return s


def _want(s, cr, noise, strength):
    """float64: init = min(int(n * s), n), start = n - init, sqrt(abar_t) x0 + sqrt(1 - abar_t) z at t = timesteps[start]."""
    n = s.timesteps.numel()
    ac = s.alphas_cumprod.double()
    starts, out = [], cr.double().clone()
    for f, st in enumerate(strength):
        start = n - min(int(n * float(st)), n)
        starts.append(start)
        if start < n:
            a = ac[int(s.timesteps[start])]
            out[f] = a.sqrt() * cr[f].double() + (1 - a).sqrt() * noise[f].double()
    return starts, out


@pytest.mark.parametrize("n", [10, 20, 50])
def test_img2img_start_per_face_strength(n):
    from hifidiff_amd import sampling
    g = torch.Generator().manual_seed(n)
    cr, z = torch.randn((6, 4, 16, 16), generator=g), torch.randn((6, 4, 16, 16), generator=g)
    s = _sched(n)
    strength = torch.tensor([0.0, 1.0, 0.6, 0.25, 0.999, 0.5])
    lat, start = sampling.img2img_start(s, cr, strength, noise=z)
    ws, wl = _want(s, cr, z, strength.tolist())
    assert start.dtype == torch.int64 and start.tolist() == ws
    assert start[0] == n and start[1] == 0                          # strength 0: no rows; strength 1: the whole schedule
    assert torch.equal(lat[0], cr[0])                               # returned unchanged
    np.testing.assert_allclose(lat.double().numpy(), wl.numpy(), rtol=1e-6, atol=1e-6)


def test_img2img_start_scalar_strength_and_generator():
    from hifidiff_amd import sampling
    s = _sched(50)
    cr = torch.randn((3, 4, 16, 16), generator=torch.Generator().manual_seed(1))
    lat, start = sampling.img2img_start(s, cr, 0.6, generator=torch.Generator().manual_seed(2))
    assert start.tolist() == [20, 20, 20]
    z = torch.randn(cr.shape, generator=torch.Generator().manual_seed(2))
    _, wl = _want(s, cr, z, [0.6] * 3)
    np.testing.assert_allclose(lat.double().numpy(), wl.numpy(), rtol=1e-6, atol=1e-6)
    lat0, start0 = sampling.img2img_start(s, cr, 0.0)
    assert start0.tolist() == [50] * 3 and torch.equal(lat0, cr)
    with pytest.raises(ValueError):
        sampling.img2img_start(s, cr, torch.tensor([0.5, 0.5]))
    with pytest.raises(ValueError):
        sampling.img2img_start(s, cr, 1.5)


@pytest.fixture(scope="module")
def recs():
    import __graft_entry__ as g
    import isa_report
    g.build()
    if not os.path.isdir(isa_report.BUILD) or not [f for f in os.listdir(isa_report.BUILD) if f.endswith(".o")]:
        pytest.skip("object files of the in-tree build are not present (prebuilt .so only)")
    return isa_report.collect()


def _p(r):
    return r["pretty"].replace("void ", "").replace("hd::", "")


ROWS_KERNELS = ("naf_face_rows_stage_kernel<128, 32>", "naf_face_rows_stage_kernel<256, 16>", "xcd_rows_stage_kernel<1024, 4>", "hca_ending_conv_kernel<true>",
                "ending_conv_kernel<8, true>", "ending_conv_kernel<16, true>", "film_rows_gather_kernel")


def test_per_face_instantiations_have_no_scratch_and_no_flat(recs):
    import isa_report
    found = [r for r in recs if _p(r).startswith(ROWS_KERNELS)]
    assert {k for k in ROWS_KERNELS if any(_p(r).startswith(k) for r in found)} == set(ROWS_KERNELS)
    bad = [(_p(r)[:60], r["scratch"], r["vgpr_spill"], r["scratch_bytes"]) for r in found if r["scratch"] or r["vgpr_spill"] or r["scratch_bytes"]]
    assert not bad, bad
    flat = [(_p(r)[:60], r["flat"]) for r in found if r.get("flat")]
    assert not flat, flat
