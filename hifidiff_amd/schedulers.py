"""DDIMScheduler / DDPMScheduler with the surface the reference's sampling loop uses
(test_refiner.py:85-91,166-171; train_refiner.py:109-120,337-348):
    sched = DDIMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear",
                          prediction_type="epsilon", clip_sample_range=3.0)
    sched.set_timesteps(50); for t in sched.timesteps: x = sched.step(eps, t, x, eta=0.0).prev_sample
The arithmetic restates diffusers 0.32.2 (not installed here; "parity unpinned"): the
per-step scalars are computed on the host in fp32 exactly in diffusers' order, the elementwise update
runs in the HIP kernel `sched_step_direct_kernel` (or inside the captured graph for `sample()`).
"""
import ctypes
import math

import torch

from . import _lib
from ._context import stream_ptr


class SchedulerOutput:
    def __init__(self, prev_sample):
        self.prev_sample = prev_sample


class _Base:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="scaled_linear",
                 prediction_type="epsilon", clip_sample=True, clip_sample_range=1.0, **unused):
        if beta_schedule != "scaled_linear" or prediction_type != "epsilon":
            raise NotImplementedError("the reference only uses beta_schedule='scaled_linear', prediction_type='epsilon'")
        self.num_train_timesteps = int(num_train_timesteps)
        self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, self.num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.clip_sample = bool(clip_sample)
        self.clip_sample_range = float(clip_sample_range)
        self.init_noise_sigma = 1.0
        self.num_inference_steps = self.num_train_timesteps
        self.timesteps = torch.arange(self.num_train_timesteps - 1, -1, -1, dtype=torch.long)
        self._timesteps_set = False                        # diffusers' num_inference_steps is None until set_timesteps

    def set_timesteps(self, num_inference_steps, device=None):
        if num_inference_steps > self.num_train_timesteps:
            raise ValueError("num_inference_steps cannot exceed num_train_timesteps")
        r = self.num_train_timesteps // num_inference_steps
        self.num_inference_steps = int(num_inference_steps)
        self._timesteps_set = True
        self.timesteps = (torch.arange(0, num_inference_steps, dtype=torch.long) * r).flip(0)   # 'leading', offset 0
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def add_noise(self, original_samples, noise, timesteps):
        """sqrt(abar_t) x0 + sqrt(1-abar_t) n (train_refiner.py:168); plain torch plumbing, not on the sampling path."""
        a = self.alphas_cumprod.to(original_samples.device)[timesteps.long()].to(original_samples.dtype)
        sa = (a ** 0.5).view(-1, *([1] * (original_samples.dim() - 1)))
        sb = ((1 - a) ** 0.5).view(-1, *([1] * (original_samples.dim() - 1)))
        return sa * original_samples + sb * noise

    def _alpha(self, t):
        return self.alphas_cumprod[t] if t >= 0 else self.final_alpha_cumprod

    def _coef(self, t):
        raise NotImplementedError

    def coefficient_table(self):
        """(timesteps [n] fp32, coef [n,7] fp32) for hd_sample: see hd_schedule in include/hifidiff_hip.h.
        The table depends on the schedule only (1000 x a dozen fp32 scalar operations in diffusers' order: 12 ms of host time),
        so it is kept until anything `_coef` reads changes (timesteps, step counts, clipping, the alpha tables) -- like the FiLM
        table of the schedule inside hd_sample.  The two tensors are shared with the cache: read-only for the caller."""
        ts = [int(t) for t in (self.timesteps.tolist() if hasattr(self.timesteps, "tolist") else self.timesteps)]
        ac, fa = self.alphas_cumprod, self.final_alpha_cumprod
        # everything _coef reads: the schedule, the clipping, and the alpha tables (identity + in-place version of the tensors)
        key = (tuple(ts), self.num_inference_steps, self.num_train_timesteps, self.clip_sample, self.clip_sample_range,
               id(ac), getattr(ac, "_version", 0), float(fa))
        hit = getattr(self, "_coef_cache", None)
        if hit is None or hit[0] != key:
            hit = (key, torch.tensor(ts, dtype=torch.float32),
                   torch.tensor([self._coef(t) for t in ts], dtype=torch.float32).reshape(len(ts), 7))
            self._coef_cache = hit
        return hit[1], hit[2]

    def _launch(self, eps, t, x, noise, seed, step):
        if not (x.is_cuda and eps.is_cuda):
            raise RuntimeError("hifidiff_amd schedulers run on the GPU only (no CPU fallback)")
        if eps.device != x.device or (noise is not None and noise.is_cuda and noise.device != x.device):
            raise RuntimeError("scheduler.step: sample, model_output and noise must live on one device (%s vs %s)" % (x.device, eps.device))
        x = x.contiguous().clone()
        eps = eps.contiguous().to(torch.float32)
        c = (ctypes.c_float * 7)(*self._coef(int(t)))
        nptr = None
        if noise is not None:
            noise = noise.contiguous().to(device=x.device, dtype=torch.float32)
            nptr = noise.data_ptr()
        with torch.cuda.device(x.device):                  # the C function takes no context: launch on x's device and stream
            rc = _lib.lib().hd_scheduler_step(x.data_ptr(), eps.data_ptr(), c, nptr, int(seed), int(step), x.numel(),
                                              stream_ptr(x.device))
        _lib.check(rc)
        return SchedulerOutput(x)


class DDIMScheduler(_Base):
    def _coef(self, t):
        r = self.num_train_timesteps // self.num_inference_steps
        a, a_p = self._alpha(t), self._alpha(t - r)
        clip = self.clip_sample_range if self.clip_sample else float("inf")
        return [float((1 - a) ** 0.5), float(a ** 0.5), clip, float(a_p ** 0.5), 0.0, float((1 - a_p) ** 0.5), 0.0]

    def step(self, model_output, timestep, sample, eta=0.0, **kw):
        if eta != 0.0:
            raise NotImplementedError("only eta=0 (the reference's setting, test_refiner.py:91) is implemented")
        if not self._timesteps_set:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        eps = getattr(model_output, "sample", model_output)
        return self._launch(eps, timestep, sample, None, 0, 0)


class DDPMScheduler(_Base):
    """variance_type 'fixed_small'.  `step(..., noise=z)` takes the noise explicitly; without it z is
    drawn from Philox(seed, step_index) on the device."""

    def _coef(self, t):
        r = self.num_train_timesteps // self.num_inference_steps
        a, a_p = self._alpha(t), self._alpha(t - r)
        alpha_t = a / a_p
        beta_t = 1 - alpha_t
        clip = self.clip_sample_range if self.clip_sample else float("inf")
        sig = float(torch.clamp((1 - a_p) / (1 - a) * beta_t, min=1e-20) ** 0.5) if t > 0 else 0.0
        return [float((1 - a) ** 0.5), float(a ** 0.5), clip, float(a_p ** 0.5 * beta_t / (1 - a)),
                float(alpha_t ** 0.5 * (1 - a_p) / (1 - a)), 0.0, sig]

    def step(self, model_output, timestep, sample, noise=None, seed=0, **kw):
        eps = getattr(model_output, "sample", model_output)
        ts = [int(v) for v in self.timesteps]
        if int(timestep) not in ts:                        # the Philox stream is keyed by the step's index in the schedule
            raise ValueError("timestep %d is not in the current schedule (set_timesteps changed, or a stale t)" % int(timestep))
        return self._launch(eps, timestep, sample, noise, seed, ts.index(int(timestep)))


class DPMSolverMultistepScheduler(_Base):
    """DPM-Solver++ 2M (`algorithm_type="dpmsolver++"`) and SDE-DPM-Solver++ 2M (`"sde-dpmsolver++"`) for the
    epsilon-prediction network, with the constructor subset of diffusers' DPMSolverMultistepScheduler that a pipeline
    swaps in for DDIMScheduler (linspace timesteps, midpoint solver type, final sigma 0, first-order last step).
    Written from Lu et al. 2022 (arXiv 2211.01095, Alg. 2 and its SDE variant):
        alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda = log(alpha / sigma), h = lambda' - lambda, r0 = h_prev / h
        2M:     x' = (sigma'/sigma) x - alpha' (e^-h - 1) (x0 + (x0 - x0_prev) / (2 r0))
        SDE 2M: x' = (sigma'/sigma) e^-h x + alpha' (1 - e^-2h) (x0 + (x0 - x0_prev) / (2 r0)) + sigma' sqrt(1 - e^-2h) z
    folded into the 8-column coefficient form of hd_schedule_ms (include/hifidiff_hip.h): c0 = sigma, c1 = alpha, c2 = inf,
    c5 = 0 and c3 / c4 / c6 / c7 from the lines above.  The first step (no x0_prev) and the last step (sigma' = 0: lands on x0)
    are first order.  The previous step's x0 lives in a device tensor of the scheduler (`step`) or of the context (`sample()`)."""

    _DEFAULTS = dict(trained_betas=None, thresholding=False, use_karras_sigmas=False, use_lu_lambdas=False, euler_at_final=False,
                     variance_type=None, lambda_min_clipped=-float("inf"), steps_offset=0, use_exponential_sigmas=False,
                     use_beta_sigmas=False)

    def __init__(self, num_train_timesteps=1000, beta_start=1e-4, beta_end=0.02, beta_schedule="scaled_linear",
                 prediction_type="epsilon", solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint",
                 lower_order_final=True, final_sigmas_type="zero", timestep_spacing="linspace", **kw):
        for k, v in kw.items():
            if k not in self._DEFAULTS or v != self._DEFAULTS[k]:
                raise NotImplementedError("DPMSolverMultistepScheduler: %s=%r is not implemented" % (k, v))
        if solver_order not in (1, 2):
            raise NotImplementedError("solver_order must be 1 or 2")
        if algorithm_type not in ("dpmsolver++", "sde-dpmsolver++"):
            raise NotImplementedError("algorithm_type must be 'dpmsolver++' or 'sde-dpmsolver++'")
        if solver_type != "midpoint" or not lower_order_final or final_sigmas_type != "zero" or timestep_spacing != "linspace":
            raise NotImplementedError("only solver_type='midpoint', lower_order_final=True, final_sigmas_type='zero', "
                                      "timestep_spacing='linspace' are implemented")
        super().__init__(num_train_timesteps, beta_start, beta_end, beta_schedule, prediction_type, clip_sample=False)
        self.solver_order = int(solver_order)
        self.algorithm_type = algorithm_type
        self._x0_hist = None

    def set_timesteps(self, num_inference_steps, device=None):
        n = int(num_inference_steps)
        if not 1 <= n <= self.num_train_timesteps:
            raise ValueError("num_inference_steps must be in [1, num_train_timesteps]")
        ts = torch.linspace(0, self.num_train_timesteps - 1, n + 1, dtype=torch.float64).round().flip(0)[:-1].to(torch.long)
        self.num_inference_steps = n
        self._timesteps_set = True
        self.timesteps = ts if device is None else ts.to(device)
        self._x0_hist = None                               # the history belongs to one pass over the schedule

    def _rows(self, ts):
        """float64 coefficient rows [n][8] of the schedule ts."""
        ac = self.alphas_cumprod.to(torch.float64)
        al = [float(ac[t]) ** 0.5 for t in ts] + [1.0]     # after the last step: sigma 0, alpha 1
        sg = [(1.0 - float(ac[t])) ** 0.5 for t in ts] + [0.0]
        lam = [math.log(a / s) if s > 0 else math.inf for a, s in zip(al, sg)]
        sde = self.algorithm_type == "sde-dpmsolver++"
        n, rows = len(ts), []
        for i in range(n):
            a, s, a1, s1 = al[i], sg[i], al[i + 1], sg[i + 1]
            h = lam[i + 1] - lam[i]
            eh = math.exp(-h)                              # 0 at the last step (h = inf)
            second = self.solver_order == 2 and 0 < i < n - 1
            k = 0.5 * h / (lam[i] - lam[i - 1]) if second else 0.0     # 1 / (2 r0), r0 = h_prev / h
            if sde:
                c4, g, c6 = s1 / s * eh, a1 * (1.0 - eh * eh), s1 * math.sqrt(1.0 - eh * eh)
            else:
                c4, g, c6 = s1 / s, -a1 * (eh - 1.0), 0.0
            rows.append([s, a, math.inf, g * (1.0 + k), c4, 0.0, c6, -g * k if second else 0.0])
        return rows

    def coefficient_table(self):
        """(timesteps [n] fp32, coef [n,8] fp32) for hd_sample_multistep (hd_schedule_ms); cached like the DDIM table."""
        ts = [int(t) for t in self.timesteps.tolist()]
        ac = self.alphas_cumprod
        key = (tuple(ts), self.solver_order, self.algorithm_type, id(ac), getattr(ac, "_version", 0))
        hit = getattr(self, "_coef_cache", None)
        if hit is None or hit[0] != key:
            hit = (key, torch.tensor(ts, dtype=torch.float32), torch.tensor(self._rows(ts), dtype=torch.float32).reshape(len(ts), 8))
            self._coef_cache = hit
        return hit[1], hit[2]

    def step(self, model_output, timestep, sample, noise=None, seed=0, **kw):
        """One update; the previous step's x0 is kept in the scheduler (reset by set_timesteps).  noise: z of this step
        (SDE variant), or None -> device Philox(seed, index of the step in the schedule), as in sample()."""
        if not self._timesteps_set:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        eps = getattr(model_output, "sample", model_output)
        ts = [int(v) for v in self.timesteps]
        if int(timestep) not in ts:
            raise ValueError("timestep %d is not in the current schedule (set_timesteps changed, or a stale t)" % int(timestep))
        i = ts.index(int(timestep))
        x = sample
        if not (x.is_cuda and eps.is_cuda):
            raise RuntimeError("hifidiff_amd schedulers run on the GPU only (no CPU fallback)")
        if eps.device != x.device or (noise is not None and noise.is_cuda and noise.device != x.device):
            raise RuntimeError("scheduler.step: sample, model_output and noise must live on one device (%s vs %s)" % (x.device, eps.device))
        x = x.contiguous().to(torch.float32).clone()
        eps = eps.contiguous().to(torch.float32)
        row = self.coefficient_table()[1][i].tolist()
        h = self._x0_hist
        if h is None or h.shape != x.shape or h.device != x.device:
            if row[7] != 0.0:
                raise RuntimeError("DPMSolverMultistepScheduler.step: step %d needs the previous step's x0 of this sample "
                                   "(steps must run in schedule order from the first one)" % i)
            h = self._x0_hist = torch.empty_like(x)       # c7 == 0: the unwritten history is not read
        c = (ctypes.c_float * 8)(*row)
        nptr = None
        if noise is not None:
            noise = noise.contiguous().to(device=x.device, dtype=torch.float32)
            nptr = noise.data_ptr()
        with torch.cuda.device(x.device):
            rc = _lib.lib().hd_scheduler_step_multistep(x.data_ptr(), eps.data_ptr(), c, h.data_ptr(), nptr, int(seed), i, x.numel(),
                                                        stream_ptr(x.device))
        _lib.check(rc)
        return SchedulerOutput(x)
