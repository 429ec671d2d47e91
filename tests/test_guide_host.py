"""Host side of the low-pass fidelity guidance (no GPU): sampling.low_pass against torch's own avg_pool2d + bilinear interpolate in
float64, and the argument checks of set_guidance / sample(guide=...) / ContinuousSampler.submit(fidelity=...) that come before any device
work."""
import pytest
import torch
import torch.nn.functional as F

from hifidiff_amd import _lib, sampling, schedulers
from hifidiff_amd.refiner import Denoiser, FacialRefiner, guidance_args

LP_TOL = 1e-12                                    # float64 against float64: the two differ by a few ulp (2e-16 measured)


def test_the_entry_points_are_exported():
    with open(_lib.HEADER) as fh:
        header = fh.read()
    for name in ("hd_guide_config", "hd_guide_faces"):
        assert name in _lib.EXPORTS
        assert "int %s(" % name in header


# ------------------------------------------------------------------------------------------------ low_pass
@pytest.mark.parametrize("L", [16, 32])
def test_low_pass_is_avg_pool_then_bilinear(L):
    x = torch.randn((3, 4, L, L), generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    for N in sorted({1, 2, 4, 8, 16, L}):
        want = F.interpolate(F.avg_pool2d(x, N), size=L, mode="bilinear", align_corners=False)
        got = sampling.low_pass(x, N)
        err = float((got - want).abs().max())
        print(f"low_pass L = {L}, N = {N}: max abs {err:.2e} from F.interpolate(F.avg_pool2d)")
        assert got.dtype == torch.float64 and tuple(got.shape) == tuple(x.shape)
        assert err <= LP_TOL, (L, N, err)
    assert torch.equal(sampling.low_pass(x, 1), x)                    # N = 1: the identity, bit for bit
    mean = x.mean(dim=(-2, -1), keepdim=True).expand_as(x)
    assert float((sampling.low_pass(x, L) - mean).abs().max()) <= LP_TOL   # N = L: the plane mean everywhere


def test_low_pass_dtypes_and_argument_checks():
    x = torch.randn((2, 16, 16), generator=torch.Generator().manual_seed(1))
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        y = sampling.low_pass(x.to(dt), 4)
        assert y.dtype == dt and tuple(y.shape) == (2, 16, 16)
    assert float((sampling.low_pass(x, 4).double() - sampling.low_pass(x.double(), 4)).abs().max()) <= 1e-6
    for bad in (3, 0, -4, 32, 5):
        with pytest.raises(ValueError):
            sampling.low_pass(x, bad)
    with pytest.raises(ValueError):
        sampling.low_pass(x, 4.0)
    with pytest.raises(ValueError):
        sampling.low_pass(torch.zeros((4, 16, 8)), 4)


# ------------------------------------------------------------------------------------------------ argument checks before any device work
def _bad_guidance(n=2, L=16, batch_known=True):
    """(target, weight, scale, rows) tuples that must be refused for a batch of n faces at latent L.  batch_known=False: without a
    prepared batch the face count is the target's own, so a target of another count is not a shape error yet."""
    g = torch.zeros((n, 4, L, L))
    return ([(torch.zeros((n + 1, 4, L, L)), 0.5, 4, None)] if batch_known else []) + [
        (torch.zeros((n, 3, L, L)), 0.5, 4, None),                    # wrong shapes
        (torch.zeros((n, 4, L, L // 2)), 0.5, 4, None),
        (g, torch.full((n + 1,), 0.5), 4, None),
        (g, 0.5, torch.full((n + 1,), 4), None),
        (g, 0.5, 4, torch.zeros((n + 1, 2), dtype=torch.int64)),
        (g, 0.5, 4, (0, 1, 2)),
        (None, 0.5, 4, None),
        (g, 0.0, 4, None),                                            # weight outside (0, 1] or not finite
        (g, -0.1, 4, None),
        (g, 1.5, 4, None),
        (g, float("nan"), 4, None),
        (g, float("inf"), 4, None),
        (g, torch.tensor([0.5, 0.0][:n]), 4, None),
        (g, 0.5, 3, None),                                            # N not a divisor of L
        (g, 0.5, 0, None),
        (g, 0.5, 2 * L, None),
        (g, 0.5, 4.0, None),
        (g, 0.5, torch.tensor([4, 5][:n]), None),
        (g, 0.5, 4, (3, 3)),                                          # rows: j0 >= j1 or j0 < 0
        (g, 0.5, 4, (5, 2)),
        (g, 0.5, 4, (-1, 4)),
        (g, 0.5, 4, torch.tensor([[0, 4], [4, 4]][:n])),
    ]


def test_guidance_args_returns_the_per_face_arrays():
    g = torch.ones((2, 4, 16, 16), dtype=torch.float64)
    t, w, N, r = guidance_args(g, 0.25, 8, None, 2, 16)
    assert t.dtype == torch.float32 and w.tolist() == [0.25, 0.25] and N.tolist() == [8, 8] and r is None
    assert w.dtype == torch.float32 and N.dtype == torch.int32
    t, w, N, r = guidance_args(g, torch.tensor([1.0, 0.5]), torch.tensor([1, 16]), (2, 5), 2, 16)
    assert w.tolist() == [1.0, 0.5] and N.tolist() == [1, 16] and r.tolist() == [[2, 5], [2, 5]] and r.dtype == torch.int32
    t, w, N, r = guidance_args(g, 1.0, 2, torch.tensor([[0, 1], [3, 9]]), 2, 16)
    assert r.tolist() == [[0, 1], [3, 9]]
    assert guidance_args(torch.ones((1, 4, 32, 32)), 1.0, 32, None, 1, 32)[2].tolist() == [32]


@pytest.mark.parametrize("model", [lambda: FacialRefiner(16), lambda: Denoiser(16)])
def test_set_guidance_argument_checks(model):
    m = model()
    for g, w, N, rows in _bad_guidance(batch_known=False):
        with pytest.raises(ValueError):
            m.set_guidance(g, w, N, rows)
    # well-formed arguments get past the checks: what stops them here is that no batch is prepared
    with pytest.raises(RuntimeError):
        m.set_guidance(torch.zeros((2, 4, 16, 16)), 0.5, 4)
    with pytest.raises(RuntimeError):
        m.set_guidance(torch.zeros((2, 4, 16, 16)), torch.tensor([0.5, 1.0]), torch.tensor([16, 1]), rows=(0, 3))
    m.clear_guidance()                                                # nothing prepared: nothing to clear
    m.disable_guidance()


def test_sample_argument_checks():
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(10)
    m = FacialRefiner(16)
    x, crf, crl = torch.zeros((2, 4, 16, 16)), torch.zeros((2, 3, 128, 128)), torch.zeros((2, 4, 16, 16))
    for g, w, N, rows in _bad_guidance():
        if g is None:
            continue                                                  # guide=None is "no guidance", not an error
        with pytest.raises(ValueError):
            sampling.sample(m, x, crf, crl, s, guide=g, guide_weight=w, guide_scale=N, guide_rows=rows)
    u = Denoiser(16)
    with pytest.raises(ValueError):
        sampling.sample(u, x, None, None, s, guide=crl, guide_weight=2.0)


def test_continuous_sampler_submit_checks():
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(10)
    cs = sampling.ContinuousSampler(FacialRefiner(16), s, batch=4)
    crf, crl = torch.zeros((3, 128, 128)), torch.zeros((4, 16, 16))
    for kw in (dict(fidelity=0.0), dict(fidelity=1.5), dict(fidelity=float("nan")), dict(fidelity=0.5, fidelity_scale=3),
               dict(fidelity=0.5, fidelity_scale=32), dict(fidelity=0.5, fidelity_rows=(4, 4)), dict(fidelity=0.5, fidelity_rows=(-1, 4)),
               dict(fidelity=0.5, fidelity_rows=(1, 2, 3)), dict(fidelity=torch.tensor([0.5, 0.5]))):
        with pytest.raises(ValueError):
            cs.submit(crf, crl, seed=1, **kw)
    with pytest.raises(ValueError):
        cs.submit(crf, torch.zeros((4, 16, 8)), seed=1, fidelity=0.5)
    assert cs.queue == []
    assert cs.submit(crf, crl, seed=1, fidelity=0.5) == 0
    assert cs.submit(crf, crl, seed=2, fidelity=1.0, fidelity_scale=16, fidelity_rows=(0, 6)) == 1
    assert cs.submit(crf, crl, seed=3, mask=torch.ones((16, 16))) == 2
    assert [q[6] for q in cs.queue] == [(0.5, 4, None), (1.0, 16, (0, 6)), None]
    # the fields other host tests read keep their places: the mask is field 5 (tests/test_mask_host.py), the schedule the last (tests/test_spans_host.py)
    assert [q[5] is not None for q in cs.queue] == [False, False, True] and [q[-1] for q in cs.queue] == [None] * 3
    un = sampling.ContinuousSampler(Denoiser(16), s, batch=4)
    with pytest.raises(ValueError):
        un.submit(None, None, seed=1, fidelity=0.5)
