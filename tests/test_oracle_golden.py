"""Pin the CPU oracle against golden vectors produced by the reference itself
(oracle/make_golden.py).  fp32 mode must reproduce the reference to fp32 noise (it is in fact
bit-identical on the machine that generated the fixtures); the bf16-emulation mode must stay within
the bf16 tolerance SURVEY §8d states (single eps rel-L2 <= 1e-2, 50-step DDIM PSNR >= 40 dB)."""
import numpy as np
import pytest
import torch

from conftest import golden, psnr, rel_l2
from hifidiff_amd import arch, synth
from oracle import hifidiff_oracle as O

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
TOL32 = 2e-6   # fp32 oracle vs reference (different BLAS threading may reorder sums)
TOL32_DEEP = 4e-6   # the same at the coarse restoration's middle_blocks, where the golden itself is 3.2e-6 from exact arithmetic
BLOCKS = ["encoders.0.0", "encoders.1.0", "encoders.2.0", "encoders.3.0", "middle_blks.0"]


def test_time_embedding(weights16):
    g = golden("time_embedding.npz")
    t = T(g["t"])
    assert rel_l2(O.sinusoidal_embedding(t), g["posemb"]) <= TOL32
    assert rel_l2(O.time_embedding(weights16, t), g["temb"]) <= TOL32


@pytest.mark.parametrize("level", range(5))
def test_cond_naf_block(weights16, level):
    g = golden("cond_naf_blocks.npz")
    c, h = arch.naf_levels(16)[level]
    x = T(synth.randn(f"blk_in/{level}", (1, c, h, h)))
    temb = T(synth.randn("blk_temb", (1, 512)))
    p = "denoiser." + BLOCKS[level]
    assert rel_l2(O.cond_naf_block(weights16, p, x, temb), g[f"out{level}"]) <= TOL32
    assert rel_l2(O.cond_naf_block(weights16, p, x, temb, O.BF16), g[f"out{level}"]) <= 2e-3


@pytest.mark.parametrize("i", range(5))
def test_hca(weights16, i):
    g = golden("hca.npz")
    c, h = arch.naf_levels(16)[::-1][i]
    fg = T(synth.randn(f"hca_fg/{i}", (1, c, h, h)))
    fd = T(synth.randn(f"hca_fd/{i}", (1, c, h, h)))
    p = f"denoiser.hcas.{i}"
    w_c, w_s = O.hca_gates(weights16, p, fg)
    assert rel_l2(w_c, g[f"wc{i}"]) <= TOL32 and rel_l2(w_s, g[f"ws{i}"]) <= TOL32
    assert rel_l2(O.hca(weights16, p, fg, fd), g[f"out{i}"]) <= TOL32
    assert rel_l2(O.hca(weights16, p, fg, fd, O.BF16), g[f"out{i}"]) <= 1e-2


def test_fpg_and_idc(weights16):
    _, crl, crf = synth.sample_inputs(1, 16)
    g = golden("fpg_priors.npz")
    for prec, tol in ((O.FP32, TOL32), (O.BF16, 2e-2)):
        for i, p in enumerate(O.fpg(weights16, crl, "fpg", prec)):
            assert rel_l2(p, g[f"prior{i}"]) <= tol, (prec.emulate, i)
    e = golden("idc_embedding.npz")["emb"]
    assert rel_l2(O.resnet50(weights16, crf), e) <= TOL32
    assert rel_l2(O.resnet50(weights16, crf, "idc", O.BF16), e) <= 1e-2


def test_refiner_eps(weights16):
    x, crl, crf = synth.sample_inputs(2, 16)
    g = golden("refiner_eps_L16.npz")
    for t in (980, 500, 0):
        assert rel_l2(O.refiner_forward(weights16, x, torch.full((2,), t), crf, crl), g[f"eps_t{t}"]) <= TOL32
    assert rel_l2(O.refiner_forward(weights16, x, torch.tensor([37, 861]), crf, crl), g["eps_tmixed"]) <= TOL32
    cond = O.Conditioning(weights16, crl, crf)
    assert rel_l2(O.fused_denoiser(weights16, x, 250, cond=cond), g["eps_scalar_t250"]) <= TOL32
    e = O.fused_denoiser(weights16, x, torch.full((2,), 500), cond=O.Conditioning(weights16, crl, crf, prec=O.BF16),
                         prec=O.BF16)
    assert rel_l2(e, g["eps_t500"]) <= 1e-2


@pytest.fixture(scope="module")
def weights64(weights16):
    """Only idc_conv (2048 -> 32768 at latent 64) is generated; every other tensor is the latent-16 one."""
    return synth.refiner_state_dict(64, reuse=(weights16, 16))


def test_refiner_eps_latent64(weights64):
    """FacialRefiner(64) (oracle/make_golden.py --only l64), one face: the fp32 oracle reproduces the reference's eps, the bf16-emulating
    oracle stays within 5e-3 of it -- half of the 1e-2 the HIP path is held to against the same golden (tests/test_latent64.py), so the
    emulation's own error cannot use that bound up.  Measured: 0.0 and 3.14e-3."""
    x, crl, crf = synth.sample_inputs(1, 64)
    g = golden("refiner_eps_L64.npz")["eps_t500"]
    assert g.shape == (1, 4, 64, 64) and g.dtype == np.float32
    r32 = rel_l2(O.refiner_forward(weights64, x, torch.full((1,), 500), crf, crl), g)
    e = O.fused_denoiser(weights64, x, torch.full((1,), 500), cond=O.Conditioning(weights64, crl, crf, prec=O.BF16), prec=O.BF16)
    r16 = rel_l2(e, g)
    print(f"latent 64 eps_t500: fp32 oracle {r32:.3e}, bf16-emulating oracle {r16:.3e}")
    assert r32 <= TOL32
    assert r16 <= 5e-3


def test_ddim50_first5_latent64(weights64):
    """The first 5 steps of the 50-step DDIM (eta 0, clip 3.0) at latent 64: the reference network inside the restated scheduler."""
    x, crl, crf = synth.sample_inputs(1, 64)
    g = golden("ddim50_first5_L64.npz")["final"]
    assert g.shape == (1, 4, 64, 64) and g.dtype == np.float32
    sch = O.DDIMScheduler(clip_sample=True, clip_sample_range=3.0)
    sch.set_timesteps(50)
    lat = O.sample(weights64, x, crf, crl, sch, "ddim", max_steps=5)
    r = rel_l2(lat, g)
    print(f"latent 64 ddim50 first 5: fp32 oracle {r:.3e}")
    assert r <= TOL32


def test_ddim50_and_ddpm20(weights16):
    x, crl, crf = synth.sample_inputs(2, 16)
    sch = O.DDIMScheduler(clip_sample=True, clip_sample_range=3.0)
    sch.set_timesteps(50)
    assert sch.timesteps[0] == 980 and sch.timesteps[-1] == 0
    lat = O.sample(weights16, x, crf, crl, sch, "ddim")
    gd = golden("ddim50_L16.npz")["final"]
    assert float((lat - T(gd)).abs().max()) <= 1e-4
    sch = O.DDPMScheduler(clip_sample=True, clip_sample_range=3.0)
    noise = lambda i: T(np.stack([synth.ddpm_noise(i, b, 16) for b in range(2)]))  # noqa: E731
    lat = O.sample(weights16, x, crf, crl, sch, "ddpm", noise_fn=noise, max_steps=20)
    assert float((lat - T(golden("ddpm20_L16.npz")["final"])).abs().max()) <= 1e-4
    lat = O.sample(weights16, x, crf, crl, sch, "ddpm", noise_fn=noise, max_steps=20, prec=O.BF16)
    assert psnr(lat, golden("ddpm20_L16.npz")["final"]) >= 40.0


def test_scheduler_formulas():
    """Known values of the restated diffusers arithmetic (parity unpinned: no reference fixture)."""
    s = O.DDIMScheduler()
    assert abs(float(s.betas[0]) - 1e-4) < 1e-9 and abs(float(s.betas[-1]) - 0.02) < 1e-7
    ab = np.cumprod(1.0 - np.linspace(1e-4 ** 0.5, 0.02 ** 0.5, 1000, dtype=np.float64) ** 2)
    assert np.allclose(s.alphas_cumprod.numpy(), ab, rtol=2e-5)     # independent float64 evaluation
    s.set_timesteps(250)
    assert s.timesteps[:2] == [996, 992] and s.timesteps[-1] == 0
    # DDIM with eps = 0 and no clipping scales x by sqrt(a_prev/a)
    s = O.DDIMScheduler(clip_sample=False)
    s.set_timesteps(50)
    x = torch.ones(1, 4, 2, 2)
    out = s.step(torch.zeros_like(x), 980, x).prev_sample
    assert torch.allclose(out, x * (s.alphas_cumprod[960] / s.alphas_cumprod[980]) ** 0.5, rtol=1e-6)
    # coefficient form used by the HIP sampler reproduces step()
    d = O.DDPMScheduler(clip_sample=True, clip_sample_range=3.0)
    c = O.step_coefficients(d, "ddpm")
    x, e, z = torch.randn(3, 1, 4, 4, 4).unbind(0)
    for i in (0, 500, 999):
        t = d.timesteps[i]
        ref = d.step(e, t, x, noise=z).prev_sample
        x0 = ((x - c[i, 0] * e) / c[i, 1]).clamp(-c[i, 2], c[i, 2])
        got = c[i, 3] * x0 + c[i, 4] * x + c[i, 5] * e + c[i, 6] * z
        assert torch.allclose(got, ref, atol=2e-5)


def test_unconditional_denoiser(weights16):
    """`Denoiser` (models/denoiser/model.py:32-134) restated, against the reference's own outputs."""
    g = golden("denoiser_uncond_L16.npz")
    x = torch.from_numpy(np.stack([synth.randn(f"x_T/{f}", (4, 16, 16)) for f in range(2)]))
    for i in range(3):
        assert rel_l2(O.denoiser_uncond(weights16, x, torch.from_numpy(g[f"t{i}"])), g[f"eps{i}"]) <= TOL32, i
    assert rel_l2(O.denoiser_uncond(weights16, x, 321), g["eps_scalar_t"]) <= TOL32
    assert rel_l2(O.denoiser_uncond(weights16, x, torch.from_numpy(g["t1"]), prec=O.BF16), g["eps1"]) <= 1e-2


def test_coarse_restoration():
    """CoarseRestoration (models/cr/model.py:33-88, STN models/cr/stn.py) restated, against the
    reference's own output and stage features."""
    g = golden("coarse_restoration.npz")
    P = synth.cr_state_dict()
    x = torch.from_numpy(np.stack([synth.rand(f"ln_face/{f}", (3, 128, 128)) for f in range(2)]))
    taps, taps64 = {}, {}
    assert rel_l2(O.coarse_restoration(P, x, taps=taps), g["out"]) <= TOL32
    assert rel_l2(taps["encoders.3"], g["feat.encoders.3"]) <= TOL32
    # middle_blocks is the deepest tap: the golden's own fp32 rounding sits 3.2e-6 from exact arithmetic there (the oracle in fp64),
    # and fp32 oracles that sum in another order than the fixture's machine land 1.1e-6 .. 2.4e-6 from it -- over TOL32 on some CPUs
    assert rel_l2(taps["middle_blocks"], g["feat.middle_blocks"]) <= TOL32_DEEP
    # the same restatement in fp64 (no summation-order noise of its own) under the same fixed ceiling
    out64 = O.coarse_restoration({k: v.double() if v.is_floating_point() else v for k, v in P.items()}, x.double(), taps=taps64)
    for k, a in (("out", out64), ("feat.encoders.3", taps64["encoders.3"]), ("feat.middle_blocks", taps64["middle_blocks"])):
        assert rel_l2(a, g[k]) <= TOL32_DEEP, k
    assert rel_l2(O.coarse_restoration(P, x, prec=O.BF16), g["out"]) <= 1e-2


def test_coarse_restoration_strong_warps():
    """STN grids that sample 28 % of their points outside the image (zero padding, models/cr/stn.py:43-52): the reference's
    own output and its nine thetas."""
    g = golden("coarse_restoration_wild.npz")
    assert float(g["outside_frac_stn0"]) > 0.2
    P = synth.cr_state_dict(wild=True)
    x = torch.from_numpy(np.stack([synth.rand(f"ln_face/{f}", (3, 128, 128)) for f in range(2)]))
    assert rel_l2(O.coarse_restoration(P, x), g["out"]) <= TOL32
    th = g["thetas"]
    assert th.shape == (9, 2, 6) and np.abs(th[:, :, [0, 4]] - 1).max() > 0.2      # scales far from the identity
    assert rel_l2(O.coarse_restoration(P, x, prec=O.BF16), g["out"]) <= 1e-2


def test_ddpm_tail_and_mid_slices(weights16):
    """The last 20 steps of the 1000-step DDPM (t = 19..0, ends with the no-noise step) and a mid-trajectory slice
    (t = 519..500): the reference network inside the restated scheduler."""
    g = golden("ddpm_slices_L16.npz")
    _, crl, crf = synth.sample_inputs(2, 16)
    for name, first, scale in (("tail", 980, 0.7), ("mid", 480, 1.0)):
        sch = O.DDPMScheduler(clip_sample=True, clip_sample_range=3.0)
        sch.timesteps = sch.timesteps[first:first + 20]
        assert sch.timesteps == [int(v) for v in g[name + "_t"]]
        x = T(np.stack([np.float32(scale) * synth.randn(f"x_{name}/{f}", (4, 16, 16)) for f in range(2)]))
        noise = lambda i: T(np.stack([synth.ddpm_noise(first + i, b, 16) for b in range(2)]))  # noqa: E731
        lat = O.sample(weights16, x, crf, crl, sch, "ddpm", noise_fn=noise)
        assert float((lat - T(g[name])).abs().max()) <= 1e-4, name


def test_vae_restatement_is_self_consistent():
    """SURVEY §8 f2, PARITY UNPINNED (diffusers 0.32.2 and the SD-2.1 VAE checkpoint are absent; the reference holds no fixture):
    shapes, parameter count of the published architecture, determinism, and the properties the boundary relies on."""
    man = arch.vae_manifest()
    assert len(man) == 248 and sum(int(np.prod(s)) for s, _, _ in man.values()) == 83_653_863      # SD VAE: 83.65 M parameters
    assert man["encoder.mid_block.attentions.0.to_q.weight"][0] == (512, 512) and man["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"][0] == (256, 512, 1, 1)
    P = synth.vae_state_dict()
    x = T(synth.rand("vae_in/0", (1, 3, 64, 64)))
    m = O.vae_encode_moments(P, x)
    assert tuple(m.shape) == (1, 8, 8, 8) and torch.equal(m, O.vae_encode_moments(P, x))
    z0 = O.vae_encode_scaled(P, x, 64, torch.zeros(1, 4, 8, 8))
    assert torch.allclose(z0, m[:, :4] * 0.18215)                                                  # zero noise: the scaled mean
    z1 = O.vae_encode_scaled(P, x, 64, torch.ones(1, 4, 8, 8))
    assert torch.allclose(z1 - z0, torch.exp(0.5 * m[:, 4:].clamp(-30, 20)) * 0.18215, atol=1e-6)
    y = O.vae_decode_scaled(P, z0)
    assert tuple(y.shape) == (1, 3, 64, 64) and bool(torch.isfinite(y).all())
    assert rel_l2(O.vae_encode_moments(P, x, O.BF16), m) <= 2e-2
    up = O.vae_encode_scaled(P, x, 128, torch.zeros(1, 4, 16, 16), vae_range=True)                  # bicubic 64 -> 128 + to_vae_range
    assert tuple(up.shape) == (1, 4, 16, 16)


def test_full_trajectory_goldens_are_reproduced_segment_by_segment(weights16):
    """ddpm1000_L16.npz / ddim250_L32.npz hold the reference network's latents every 100 / 50 steps of the FULL loops
    (oracle/make_golden.py --only ddpm1000 | ddim250).  The fp32 oracle, started from one committed checkpoint, reproduces the
    next one: steps 900 -> 1000 of the DDPM (incl. the no-noise step t = 0) and steps 200 -> 250 of the latent-32 DDIM."""
    g = golden("ddpm1000_L16.npz")
    _, crl, crf = synth.sample_inputs(2, 16)
    sch = O.DDPMScheduler(clip_sample=True, clip_sample_range=3.0)
    sch.timesteps = sch.timesteps[900:]
    assert sch.timesteps[0] == 99 and sch.timesteps[-1] == 0
    noise = lambda i: T(np.stack([synth.ddpm_noise(900 + i, b, 16) for b in range(2)]))  # noqa: E731
    lat = O.sample(weights16, T(g["step900"]), crf, crl, sch, "ddpm", noise_fn=noise)
    assert float((lat - T(g["final"])).abs().max()) <= 1e-4
    assert float(np.abs(g["final"]).max()) <= 3.0 + 1e-5 and float(np.abs(g["step500"]).max()) > 3.0     # x_prev leaves the clip range mid-way
    g32 = golden("ddim250_L32.npz")
    P32 = synth.refiner_state_dict(32)
    _, crl, crf = synth.sample_inputs(1, 32)
    sch = O.DDIMScheduler(clip_sample=True, clip_sample_range=3.0)
    sch.set_timesteps(250)
    sch.timesteps = sch.timesteps[200:]
    lat = O.sample(P32, T(g32["step200"]), crf, crl, sch, "ddim")
    assert float((lat - T(g32["final"])).abs().max()) <= 1e-4
