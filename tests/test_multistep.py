"""DPM-Solver++ 2M / SDE-DPM-Solver++ 2M (schedulers.DPMSolverMultistepScheduler) through the multistep coefficient form
(hd_schedule_ms: one history term c7 * previous x0) of the fused step kernels.
CPU: the coefficient table against a float64 restatement of the solver (Lu et al. 2022, arXiv 2211.01095, Alg. 2 and the SDE
variant) and the order of accuracy on a Gaussian problem whose probability-flow ODE has a closed-form solution.
GPU: the graph-replayed loop (hd_sample_multistep) against the eager loop, the oracle's network, a float64 update, and the
single-step path (hd_sample) it must leave untouched."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import golden, psnr, rel_l2, weights16  # noqa: F401  (golden: shared helper; weights16: session fixture)

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
ALGOS = ("dpmsolver++", "sde-dpmsolver++")


# --------------------------------------------------------------------------------------------------- CPU
def _ref_table(alphas_cumprod, n, order, algo):
    """float64 restatement in the lambda / h / r0 form: (timesteps [n], coef [n][8])."""
    ts = np.linspace(0, 999, n + 1).round()[::-1][:-1].astype(np.int64)
    ac = alphas_cumprod.double().numpy()[ts]
    alpha = np.append(np.sqrt(ac), 1.0)
    sigma = np.append(np.sqrt(1.0 - ac), 0.0)
    with np.errstate(divide="ignore"):
        lam = np.log(alpha) - np.log(sigma)                  # +inf after the last step
    coef = np.zeros((n, 8))
    for i in range(n):
        h = lam[i + 1] - lam[i]
        first = order == 1 or i == 0 or i == n - 1
        inv2r0 = 0.0 if first else 1.0 / (2.0 * ((lam[i] - lam[i - 1]) / h))
        if algo == "dpmsolver++":
            # x' = (s'/s) x - a' (e^-h - 1) (x0 + (x0 - h_x0) / (2 r0))
            w = -alpha[i + 1] * np.expm1(-h)
            c4, c6 = sigma[i + 1] / sigma[i], 0.0
        else:
            # x' = (s'/s) e^-h x + a' (1 - e^-2h) (x0 + (x0 - h_x0) / (2 r0)) + s' sqrt(1 - e^-2h) z
            w = -alpha[i + 1] * np.expm1(-2.0 * h)
            c4, c6 = sigma[i + 1] / sigma[i] * np.exp(-h), sigma[i + 1] * np.sqrt(-np.expm1(-2.0 * h))
        coef[i] = [sigma[i], alpha[i], np.inf, w * (1.0 + inv2r0), c4, 0.0, c6, -w * inv2r0]
    return ts, coef


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n", [5, 10, 14, 15, 20, 25])
def test_coefficient_table_against_float64_formulas(n, order, algo):
    from hifidiff_amd import schedulers
    s = schedulers.DPMSolverMultistepScheduler(solver_order=order, algorithm_type=algo)
    s.set_timesteps(n)
    ts, coef = s.coefficient_table()
    rts, rcoef = _ref_table(s.alphas_cumprod, n, order, algo)
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (n, 8)
    assert ts.tolist() == [float(t) for t in rts] and s.timesteps.tolist() == rts.tolist()
    c = coef.double().numpy()
    assert np.isinf(c[:, 2]).all() and (c[:, 5] == 0).all()
    fin = [0, 1, 3, 4, 6, 7]
    np.testing.assert_allclose(c[:, fin], rcoef[:, fin], rtol=2e-6, atol=1e-7)
    assert c[0, 7] == 0.0 and c[n - 1, 7] == 0.0                       # first and last steps: first order
    assert c[n - 1, 3] == 1.0 and c[n - 1, 4] == 0.0 and c[n - 1, 6] == 0.0   # the last step lands on x0
    if order == 1:
        assert (c[:, 7] == 0).all()
    elif n > 2:
        assert (c[1:n - 1, 7] != 0).all()


def test_constructor_subset():
    from hifidiff_amd import schedulers
    S = schedulers.DPMSolverMultistepScheduler
    S(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="epsilon",
      solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, final_sigmas_type="zero",
      timestep_spacing="linspace", use_karras_sigmas=False)
    for kw in (dict(solver_order=3), dict(algorithm_type="dpmsolver"), dict(solver_type="heun"), dict(lower_order_final=False),
               dict(final_sigmas_type="sigma_min"), dict(timestep_spacing="leading"), dict(prediction_type="v_prediction"),
               dict(beta_schedule="linear"), dict(use_karras_sigmas=True), dict(thresholding=True), dict(no_such_option=1)):
        with pytest.raises(NotImplementedError):
            S(**kw)
    s = S()
    assert s.init_noise_sigma == 1.0
    x = torch.randn(2, 4, 3, 3)
    assert s.scale_model_input(x, 10) is x
    t = torch.tensor([10, 900])
    n = torch.randn_like(x)
    a = s.alphas_cumprod[t].view(-1, 1, 1, 1)
    assert torch.allclose(s.add_noise(x, n, t), a.sqrt() * x + (1 - a).sqrt() * n)
    with pytest.raises(ValueError):
        s.step(x, 999, x)                                   # set_timesteps first


MU, SD = 0.3, 0.5                                            # data ~ N(MU, SD^2)


def _gaussian_error(sched, n):
    """Max error of the final sample against the exact ODE solution, the tables applied in float64 numpy."""
    sched.set_timesteps(n)
    ts, coef = sched.coefficient_table()
    ts, coef = ts.numpy().astype(np.int64), coef.double().numpy()
    ac = sched.alphas_cumprod.double().numpy()
    x = np.linspace(-3.0, 3.0, 101)
    a0, s0 = math.sqrt(ac[ts[0]]), math.sqrt(1.0 - ac[ts[0]])
    exact = MU + SD * (x - a0 * MU) / math.sqrt(a0 * a0 * SD * SD + s0 * s0)     # the flow keeps the standardised coordinate
    h = np.full_like(x, np.nan)
    for i, t in enumerate(ts):
        a, s = math.sqrt(ac[t]), math.sqrt(1.0 - ac[t])
        x0_post = MU + a * SD * SD / (a * a * SD * SD + s * s) * (x - a * MU)        # exact E[x0 | x_t]
        eps = (x - a * x0_post) / s
        c = coef[i]
        x0 = np.clip((x - c[0] * eps) / c[1], -c[2], c[2])
        r = c[3] * x0 + c[4] * x + c[5] * eps
        if coef.shape[1] == 8 and c[7] != 0:
            r = r + c[7] * h
        x, h = r, x0
    return float(np.abs(x - exact).max())


def test_order_of_accuracy_on_a_gaussian_problem():
    from hifidiff_amd import schedulers
    ddim = {n: _gaussian_error(schedulers.DDIMScheduler(clip_sample=False), n) for n in (10, 20)}
    dpm = {n: _gaussian_error(schedulers.DPMSolverMultistepScheduler(), n) for n in (10, 20)}
    dpm1 = {n: _gaussian_error(schedulers.DPMSolverMultistepScheduler(solver_order=1), n) for n in (10, 20)}
    assert dpm[20] <= ddim[20] / 8, (dpm, ddim)                       # measured 17x
    assert dpm[10] / dpm[20] >= 4.0, dpm                              # second order (measured 10x)
    assert ddim[10] / ddim[20] < 2.5, ddim                            # first order (measured 1.9x)
    assert dpm1[10] / dpm1[20] < 2.5 and 0.5 * ddim[20] <= dpm1[20] <= 2.0 * ddim[20], (dpm1, ddim)


# --------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


def make_model(weights, latent=16):
    from hifidiff_amd.refiner import FacialRefiner
    m = FacialRefiner(latent)
    m.load_state_dict(weights)
    m.to("cuda:0")
    return m


@pytest.fixture(scope="module")
def model(gpu, weights16):
    return make_model(weights16)


@pytest.fixture(scope="module")
def inputs2():
    from hifidiff_amd import synth
    return synth.sample_inputs(2, 16)


def _philox_normal(seed, step, elems):
    """numpy restatement of hd_kernels.hpp: Philox4x32-10, counter (elem, step, 0, 0), Box-Muller."""
    c = [elems.astype(np.uint64), np.full_like(elems, step, dtype=np.uint64), np.zeros_like(elems, dtype=np.uint64),
         np.zeros_like(elems, dtype=np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    u1 = ((c[0] >> np.uint64(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)
    u2 = (c[1] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.283185307179586) * u2)


def _eager(model, x, crf, crl, sched, n, noise=None):
    """One model(...) + scheduler.step(...) per Python iteration (the reference's loop shape with the scheduler swapped)."""
    sched.set_timesteps(n)
    x = x.cuda()
    cond = () if crf is None else (crf.cuda(), crl.cuda())       # the same objects every step: conditioning computed once
    for i, t in enumerate(sched.timesteps):
        eps = model(x, int(t), *cond).sample
        x = sched.step(eps, t, x, noise=None if noise is None else noise[i]).prev_sample
    return x.cpu()


def _update64(x, eps, c, h, z=None):
    """The hd_schedule_ms update in float64 (c: one coefficient row)."""
    c = [float(v) for v in c]
    x0 = (x - c[0] * eps) / c[1]
    if math.isfinite(c[2]):
        x0 = x0.clamp(-c[2], c[2])
    r = c[3] * x0 + c[4] * x + c[5] * eps
    if c[6] != 0.0:
        r = r + c[6] * z
    if c[7] != 0.0:
        r = r + c[7] * h
    return r, x0


@pytest.mark.gpu
def test_eager_loop_against_graph(model, inputs2):
    from hifidiff_amd import _lib, sampling, schedulers
    x, crl, crf = inputs2
    s = schedulers.DPMSolverMultistepScheduler()
    eager = _eager(model, x, crf, crl, s, 20)
    s.set_timesteps(20)
    graph = sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), s).cpu()
    assert torch.isfinite(graph).all()
    assert psnr(eager, graph) >= 50.0, psnr(eager, graph)
    # the last step lands on x0 (c3 = 1, c4 = 0), and x0 is what the context's history holds after the call
    h = np.zeros(graph.numel(), np.float32)
    assert _lib.lib().hd_debug_read(model.engine.ctx, b"x0_hist", h.ctypes.data, h.size) == h.size
    assert np.array_equal(h.reshape(graph.shape), graph.numpy())


@pytest.mark.gpu
def test_against_the_oracle_network(model, weights16, inputs2):
    from hifidiff_amd import sampling, schedulers
    from oracle import hifidiff_oracle as O
    x, crl, crf = inputs2
    s = schedulers.DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    ts, coef = s.coefficient_table()
    cond = O.Conditioning(weights16, crl, crf, prec=O.BF16)
    xr, h = x.double(), None
    for i, t in enumerate(s.timesteps.tolist()):
        eps = O.fused_denoiser(weights16, xr.float(), torch.full((x.shape[0],), t), prec=O.BF16, cond=cond).double()
        xr, h = _update64(xr, eps, coef[i], h)
    got = sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), s).cpu()
    assert rel_l2(got, xr) <= 2e-2, rel_l2(got, xr)


@pytest.mark.gpu
def test_sde_variant_with_given_and_device_noise(model, inputs2):
    from hifidiff_amd import sampling, schedulers
    x, crl, crf = inputs2
    n, seed = 10, 0x5EED0000000000A7
    s = schedulers.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    s.set_timesteps(n)
    ts, coef = s.coefficient_table()
    given = torch.randn((n,) + tuple(x.shape), generator=torch.Generator().manual_seed(7))
    philox = torch.stack([T(_philox_normal(seed, i, np.arange(x.numel()))).view(x.shape) for i in range(n)])
    crfd, crld = crf.cuda(), crl.cuda()
    for noise, kw in ((given, dict(noise=given.cuda())), (philox, dict(seed=seed))):
        xr, h = x.double(), None
        for i, t in enumerate(s.timesteps.tolist()):
            eps = model(xr.float().cuda(), int(t), crfd, crld).sample.cpu().double()
            xr, h = _update64(xr, eps, coef[i], h, noise[i].double())
        got = sampling.sample(model, x.cuda(), crfd, crld, s, **kw).cpu()
        # measured 7.7e-4 (given z): the eager trajectory's float64 rounding differs from the fp32 one by an ulp, bf16 operands
        # turn that into eps differences of bf16 size, and x0 = (x - sigma eps) / alpha multiplies them by sigma / alpha = 37 at
        # t = 999 (final latents of RMS ~1e2 on the synthetic network).  A wrong z, step index or history term is >= 1e-2.
        assert rel_l2(got, xr) <= 3e-3, rel_l2(got, xr)
    # the eager scheduler with the same z
    eager = _eager(model, x, crf, crl, s, n, noise=given.cuda())
    assert psnr(eager, sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), s, noise=given.cuda()).cpu()) >= 50.0


class _Table:
    """A fixed coefficient table in the scheduler interface sampling.sample reads."""

    def __init__(self, ts, coef):
        self.ts, self.coef = ts, coef

    def coefficient_table(self):
        return self.ts, self.coef


@pytest.mark.gpu
def test_the_single_step_path_is_untouched(model, inputs2):
    from hifidiff_amd import _lib, sampling, schedulers
    x, crl, crf = inputs2
    run = lambda sch: sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), sch).cpu()  # noqa: E731
    ddim = schedulers.DDIMScheduler(clip_sample_range=3.0)
    ddim.set_timesteps(50)
    first = run(ddim)
    ts, c7 = ddim.coefficient_table()
    padded = run(_Table(ts, torch.cat([c7, torch.zeros(c7.shape[0], 1)], 1)))   # hd_sample_multistep with c7 = 0 everywhere
    assert torch.equal(padded, first)
    ops = _lib.lib().hd_num_ops(model.engine.ctx, 0)
    dpm = schedulers.DPMSolverMultistepScheduler()
    dpm.set_timesteps(20)
    assert torch.isfinite(run(dpm)).all()
    assert _lib.lib().hd_num_ops(model.engine.ctx, 0) == ops
    assert torch.equal(run(ddim), first)


@pytest.mark.gpu
def test_two_batch_sizes_of_one_context(model):
    """B = 65 leaves the persistent stages (one launch per GEMM) and parks the batch-2 workspace with its history buffer."""
    from hifidiff_amd import sampling, schedulers, synth
    x, crl, crf = synth.sample_inputs(65, 16)
    s = schedulers.DPMSolverMultistepScheduler()
    eager = _eager(model, x, crf, crl, s, 5)
    s.set_timesteps(5)
    graph = sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), s).cpu()
    assert psnr(eager, graph) >= 50.0 and rel_l2(graph, eager) <= 1e-2, (psnr(eager, graph), rel_l2(graph, eager))
    x2, crl2, crf2 = synth.sample_inputs(2, 16)
    s.set_timesteps(5)
    a = sampling.sample(model, x2.cuda(), crf2.cuda(), crl2.cuda(), s).cpu()                 # the parked batch-2 workspace
    assert psnr(_eager(model, x2, crf2, crl2, s, 5), a) >= 50.0


@pytest.mark.gpu
def test_latent32(gpu):
    from hifidiff_amd import sampling, schedulers, synth
    m = make_model(synth.refiner_state_dict(32), 32)
    x, crl, crf = synth.sample_inputs(2, 32)
    s = schedulers.DPMSolverMultistepScheduler()
    eager = _eager(m, x, crf, crl, s, 5)
    s.set_timesteps(5)
    graph = sampling.sample(m, x.cuda(), crf.cuda(), crl.cuda(), s).cpu()
    assert psnr(eager, graph) >= 50.0 and rel_l2(graph, eager) <= 1e-2, (psnr(eager, graph), rel_l2(graph, eager))


@pytest.mark.gpu
def test_unconditional_denoiser(gpu, weights16):
    from hifidiff_amd import sampling, schedulers, synth
    from hifidiff_amd.refiner import Denoiser
    m = Denoiser(16)
    k = len("denoiser.")
    m.load_state_dict({n[k:]: v for n, v in weights16.items() if n.startswith("denoiser.") and ".hcas." not in n and ".idc_conv" not in n})
    m.to("cuda:0")
    x = T(np.stack([synth.randn(f"x_T/{f}", (4, 16, 16)) for f in range(2)]))
    s = schedulers.DPMSolverMultistepScheduler()
    eager = _eager(m, x, None, None, s, 5)
    s.set_timesteps(5)
    graph = sampling.sample(m, x.cuda(), None, None, s).cpu()
    assert psnr(eager, graph) >= 50.0 and rel_l2(graph, eager) <= 1e-2, (psnr(eager, graph), rel_l2(graph, eager))


@pytest.mark.gpu
def test_argument_checks(model, inputs2):
    from hifidiff_amd import _lib, sampling, schedulers
    L = _lib.lib()
    x, crl, crf = inputs2
    s = schedulers.DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    ts, coef = s.coefficient_table()
    sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), s)              # prepared for batch 2
    xd = x.cuda().contiguous()
    stream = torch.cuda.current_stream().cuda_stream

    def call(ts, coef, n):
        ts, coef = ts.contiguous(), coef.contiguous()
        sch = _lib.ScheduleMS()
        sch.n_steps = n
        sch.timesteps = ctypes.cast(ts.data_ptr(), ctypes.POINTER(ctypes.c_float))
        sch.coef = ctypes.cast(coef.data_ptr(), ctypes.POINTER(ctypes.c_float))
        return L.hd_sample_multistep(model.engine.ctx, xd.data_ptr(), ctypes.byref(sch), None, 0, stream)

    bad = coef.clone()
    bad[0, 7] = 0.5
    assert call(ts, bad, 10) == -1                                           # HD_ERR_INVALID: no history before the first step
    assert call(ts, coef, 0) == -1                                           # empty schedule
    assert call(ts, coef, 10) == 0
    torch.cuda.synchronize()
    # the eager entry point: a history term needs the history; with one, x0 is written back
    n = 4096
    xx, ee, hh = torch.randn(n, device="cuda"), torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    row = [0.6, 0.8, math.inf, 0.5, 0.25, 0.0, 0.0, -0.125]
    c8 = (ctypes.c_float * 8)(*row)
    assert L.hd_scheduler_step_multistep(xx.data_ptr(), ee.data_ptr(), c8, None, None, 0, 1, n, stream) == -1
    want_x0 = (xx - 0.6 * ee) / 0.8
    want = 0.5 * want_x0 + 0.25 * xx + (-0.125) * hh
    assert L.hd_scheduler_step_multistep(xx.data_ptr(), ee.data_ptr(), c8, hh.data_ptr(), None, 0, 1, n, stream) == 0
    torch.cuda.synchronize()
    assert torch.allclose(xx, want, atol=1e-5) and torch.allclose(hh, want_x0, atol=1e-6)
