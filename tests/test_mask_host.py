"""Host side of masked sampling (no GPU): sampling.region_mask, sampling.inpaint_start and the argument checks that come before any
device work."""
import pytest
import torch

from hifidiff_amd import _lib, sampling, schedulers
from hifidiff_amd.refiner import Denoiser, FacialRefiner


def test_the_entry_point_is_exported():
    assert "hd_mask_faces" in _lib.EXPORTS
    with open(_lib.HEADER) as fh:
        assert "int hd_mask_faces(" in fh.read()


# ------------------------------------------------------------------------------------------------ region_mask
def test_region_mask_aligned_box_is_binary():
    m = sampling.region_mask([(16, 32, 80, 96)], 16)                  # cells of 8 pixels: columns 2..9, rows 4..11
    want = torch.zeros(16, 16)
    want[4:12, 2:10] = 1.0
    assert m.dtype == torch.float32 and tuple(m.shape) == (16, 16) and torch.equal(m, want)
    assert torch.equal(sampling.region_mask([(0, 0, 128, 128)], 16), torch.ones(16, 16))
    assert torch.equal(sampling.region_mask([], 16), torch.zeros(16, 16))
    m32 = sampling.region_mask([(16, 32, 80, 96)], 32)                # cells of 4 pixels
    want32 = torch.zeros(32, 32)
    want32[8:24, 4:20] = 1.0
    assert torch.equal(m32, want32)


def test_region_mask_cell_fractions():
    m = sampling.region_mask([(16, 32, 20, 40)], 16)                  # the left half of cell (row 4, column 2)
    assert float(m[4, 2]) == 0.5 and float(m.sum()) == 0.5
    m = sampling.region_mask([(16, 32, 18, 34)], 16)                  # 2 x 2 of its 64 pixels
    assert float(m[4, 2]) == 4.0 / 64.0
    # overlapping boxes are a union, not a sum
    m = sampling.region_mask([(10, 10, 90, 90), (30, 30, 120, 70)], 16)
    assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0
    px = torch.zeros(128, 128)
    px[10:90, 10:90] = 1
    px[30:70, 30:120] = 1
    assert abs(float(m.mean()) - float(px.mean())) < 1e-6


def test_region_mask_feather_keeps_the_mean_of_an_interior_box():
    """A box blur with zero padding moves no mass out of the map while the box stays `feather` pixels inside it: the mean is the
    unfeathered mean exactly (up to fp32 rounding of the sums)."""
    box = [(40, 40, 88, 80)]                                          # latent columns 5..10, rows 5..9: >= 2 pixels from every edge
    m0 = sampling.region_mask(box, 16)
    for f in (1, 2):
        m = sampling.region_mask(box, 16, feather=f)
        assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0
        assert abs(float(m.double().mean()) - float(m0.double().mean())) <= 1e-6
        assert bool(((m > 0) & (m < 1)).any())
    # the blur's value at the box's corner pixel: the part of its (2f+1)^2 window that the box covers
    m = sampling.region_mask(box, 16, feather=1)
    assert abs(float(m[5, 5]) - 4.0 / 9.0) <= 1e-6 and abs(float(m[4, 4]) - 1.0 / 9.0) <= 1e-6


def test_region_mask_argument_checks():
    for bad in ([(0, 0, 129, 10)], [(-1, 0, 10, 10)], [(20, 0, 10, 10)], [(0, 0, 10)]):
        with pytest.raises(ValueError):
            sampling.region_mask(bad, 16)
    with pytest.raises(ValueError):
        sampling.region_mask([], 16, image_res=100)
    with pytest.raises(ValueError):
        sampling.region_mask([], 16, feather=-1)


# ------------------------------------------------------------------------------------------------ inpaint_start
def _add_noise64(s, known, noise, row):
    """scheduler.add_noise restated in float64 from the scheduler's alphas_cumprod."""
    a = s.alphas_cumprod.double()[int(s.timesteps[row])]
    return a.sqrt() * known.double() + (1.0 - a).sqrt() * noise.double()


@pytest.mark.parametrize("make", [lambda: schedulers.DDIMScheduler(clip_sample_range=3.0), lambda: schedulers.DDPMScheduler(clip_sample_range=3.0),
                                  lambda: schedulers.DPMSolverMultistepScheduler()])
def test_inpaint_start(make):
    s = make()
    s.set_timesteps(20)
    g = torch.Generator().manual_seed(3)
    known, noise = torch.randn((3, 4, 16, 16), generator=g), torch.randn((3, 4, 16, 16), generator=g)
    lat, start, nz = sampling.inpaint_start(s, known, 1.0, noise=noise)
    assert torch.equal(lat, noise) and start.tolist() == [0, 0, 0] and torch.equal(nz, noise)
    lat, start, nz = sampling.inpaint_start(s, known, 0.0, noise=noise)
    assert torch.equal(lat, known) and start.tolist() == [20, 20, 20] and torch.equal(nz, noise)
    lat, start, nz = sampling.inpaint_start(s, known, torch.tensor([1.0, 0.6, 0.25]), noise=noise)
    assert start.tolist() == [0, 8, 15] and torch.equal(nz, noise)
    assert torch.equal(lat[0], noise[0])
    for f in (1, 2):
        want = _add_noise64(s, known[f], noise[f], int(start[f]))
        assert float((lat[f].double() - want).abs().max()) <= 1e-5
    # the schedule contract the device blend relies on: (c1, c0) of a row are its signal and noise scale
    ts, coef = s.coefficient_table()
    for row in (0, 7, 19):
        want = _add_noise64(s, known[0], noise[0], row)
        got = float(coef[row, 1]) * known[0].double() + float(coef[row, 0]) * noise[0].double()
        assert float((got - want).abs().max()) <= 1e-5
    # drawn noise is returned
    lat, start, nz = sampling.inpaint_start(s, known, 1.0, generator=torch.Generator().manual_seed(9))
    assert torch.equal(lat, nz) and tuple(nz.shape) == tuple(known.shape)
    with pytest.raises(ValueError):
        sampling.inpaint_start(s, known, 1.5, noise=noise)


# ------------------------------------------------------------------------------------------------ argument checks before any device work
def _good(n=2, L=16):
    return torch.full((n, L, L), 0.5), torch.zeros((n, 4, L, L)), torch.zeros((n, 4, L, L))


@pytest.mark.parametrize("model", [lambda: FacialRefiner(16), lambda: Denoiser(16)])
def test_set_mask_argument_checks(model):
    m = model()
    mask, known, nz = _good()
    bad = [
        (torch.zeros((2, 8, 16)), known, nz),                         # wrong shapes
        (torch.zeros((2, 2, 16, 16)), known, nz),
        (mask, torch.zeros((2, 3, 16, 16)), nz),
        (mask, known, torch.zeros((1, 4, 16, 16))),
        (mask + 0.6, known, nz),                                      # outside [0, 1]
        (mask - 0.6, known, nz),
        (mask.clone().index_put_((torch.tensor(0), torch.tensor(0), torch.tensor(0)), torch.tensor(float("nan"))), known, nz),
        (mask.clone().index_put_((torch.tensor(0), torch.tensor(0), torch.tensor(0)), torch.tensor(float("inf"))), known, nz),
        (mask, None, nz), (mask, known, None), (None, known, nz),     # partial
    ]
    for a, b, c in bad:
        with pytest.raises(ValueError):
            m.set_mask(a, b, c)
    # well-formed arguments get past the checks: what stops them here is that no batch is prepared
    for a in (mask, mask[:, None]):
        with pytest.raises(RuntimeError):
            m.set_mask(a, known, nz)
    m.clear_mask()                                                    # nothing prepared: nothing to clear


def test_sample_argument_checks():
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(10)
    m = FacialRefiner(16)
    x, crf, crl = torch.zeros((2, 4, 16, 16)), torch.zeros((2, 3, 128, 128)), torch.zeros((2, 4, 16, 16))
    mask, known, nz = _good()
    for kw in (dict(mask=mask, known=known), dict(mask=mask, known_noise=nz), dict(known=known, known_noise=nz), dict(known=known),
               dict(mask=mask + 1.0, known=known, known_noise=nz), dict(mask=mask[:1], known=known, known_noise=nz),
               dict(mask=mask * float("nan"), known=known, known_noise=nz)):
        with pytest.raises(ValueError):
            sampling.sample(m, x, crf, crl, s, **kw)


def test_continuous_sampler_submit_checks():
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(10)
    cs = sampling.ContinuousSampler(FacialRefiner(16), s, batch=4)
    crf, crl = torch.zeros((3, 128, 128)), torch.zeros((4, 16, 16))
    for bad in (torch.zeros((8, 16)), torch.full((16, 16), 2.0), torch.full((16, 16), float("nan"))):
        with pytest.raises(ValueError):
            cs.submit(crf, crl, seed=1, mask=bad)
    assert cs.submit(crf, crl, seed=1, mask=torch.ones((16, 16))) == 0
    assert cs.submit(crf, crl, seed=2, mask=torch.ones((1, 16, 16))) == 1
    assert cs.submit(crf, crl, seed=3) == 2
    assert [q[5] is not None for q in cs.queue] == [True, True, False] and tuple(cs.queue[0][5].shape) == (16, 16)
    un = sampling.ContinuousSampler(Denoiser(16), s, batch=4)
    with pytest.raises(ValueError):
        un.submit(None, None, seed=1, mask=torch.ones((16, 16)))
