"""The reverse-diffusion loop of the refiner in latent space.

`ddim_sample_eager` is the body of the reference's `ddim_sample` (test_refiner.py:85-91,
train_refiner.py:109-120) verbatim against the mirrored modules: one `model(...)` + one
`scheduler.step(...)` per Python iteration.

`sample` is the MI355X-first form of the same loop: conditioning once, FiLM table for all steps once,
then one captured hipGraph replayed n_steps times inside libhifidiff_hip.so (`hd_sample`).
"""
import ctypes

import torch

from . import _lib


@torch.no_grad()
def ddim_sample_eager(model, latents, cr_face, cr_latent, scheduler, num_inference_steps=50):
    bs = latents.shape[0]
    scheduler.set_timesteps(num_inference_steps, device=latents.device)
    for t in scheduler.timesteps:
        t_batch = torch.full((bs,), int(t), device=latents.device, dtype=torch.long)
        noise_pred = model(latents, t_batch, cr_face, cr_latent).sample
        latents = scheduler.step(noise_pred, t, latents, eta=0.0).prev_sample
    return latents


@torch.no_grad()
def ddim_sample_eager_unconditional(model, latents, scheduler, num_inference_steps=50):
    """The unconditional loop of pretrain_denoiser.py:99-110 against the mirrored `Denoiser`."""
    bs = latents.shape[0]
    scheduler.set_timesteps(num_inference_steps, device=latents.device)
    for t in scheduler.timesteps:
        t_batch = torch.full((bs,), int(t), device=latents.device, dtype=torch.long)
        noise_pred = model(latents, t_batch).sample
        latents = scheduler.step(noise_pred, t, latents, eta=0.0).prev_sample
    return latents


def img2img_start(scheduler, cr_latent, strength, noise=None, generator=None):
    """diffusers' img2img start (`get_timesteps` + `scheduler.add_noise`) with one strength per face: returns (latents, start_steps).

    For a schedule of n rows (`scheduler.set_timesteps(n)` first) and face f of strength s_f: init = min(int(n * s_f), n),
    start_f = n - init, latents_f = add_noise(cr_latent_f, noise_f, timesteps[start_f]); a face with start_f == n (strength 0) is
    returned unchanged.  strength: a float or a [B] tensor in [0, 1]; noise: [B,4,L,L] or None (torch.randn with `generator`).
    start_steps is an int64 [B] CPU tensor for `sample(..., start_steps=...)`."""
    ts = scheduler.timesteps
    n = int(ts.numel())
    B = cr_latent.shape[0]
    s = torch.as_tensor(strength, dtype=torch.float64).flatten().cpu()
    if s.numel() == 1:
        s = s.expand(B)
    if s.numel() != B:
        raise ValueError(f"strength must be a float or a [{B}] tensor")
    if bool(((s < 0) | (s > 1)).any()):
        raise ValueError("strength must lie in [0, 1]")
    init = [min(int(n * float(v)), n) for v in s]       # diffusers: init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
    start = torch.tensor([n - i for i in init], dtype=torch.int64)
    if noise is None:
        noise = torch.randn(cr_latent.shape, generator=generator, dtype=cr_latent.dtype,
                            device=generator.device if generator is not None else cr_latent.device).to(cr_latent.device)
    noise = noise.to(device=cr_latent.device, dtype=cr_latent.dtype)
    latents = cr_latent.clone()
    run = start < n
    if bool(run.any()):
        idx = run.nonzero().flatten()
        t = ts.cpu()[start[idx]]
        latents[idx.to(cr_latent.device)] = scheduler.add_noise(cr_latent[idx.to(cr_latent.device)], noise[idx.to(cr_latent.device)],
                                                                t.to(cr_latent.device))
    return latents, start


@torch.no_grad()
def sample(model, latents, cr_face, cr_latent, scheduler, noise=None, seed=0, prepare=True, check=True,
           start_steps=None, n_iters=None, resume=False):
    """Whole loop on the GPU: returns the final latents (a new tensor).

    The scheduler's coefficient table picks the entry point: 7 columns (DDIM / DDPM) -> hd_sample, 8 columns
    (DPMSolverMultistepScheduler) -> hd_sample_multistep.
    start_steps: None (every face runs the whole schedule), or an int / [B] tensor of start rows r_f in [0, n_steps]
    (img2img_start, or a loop split over calls) -> hd_sample_rows / hd_sample_rows_multistep: n_iters iterations (default
    n_steps - min r_f) where face f is at row r_f + i and is held once past the last row.  resume=True (multistep only)
    continues the x0 history of the previous multistep call on this batch; the conditioning must not be prepared again in
    between: pass the same cr_face / cr_latent tensors (the conditioning cache then hits), or prepare=False -- needed under
    torch.inference_mode, where tensors carry no version and the cache never hits.  With resume=False a multistep face's first
    row is taken first-order (diffusers' img2img start).
    noise: optional [n_steps, B, 4, L, L] tensor of z (DDPM, SDE-DPM-Solver++); None -> device Philox(seed).
    For the unconditional `Denoiser` pass cr_face = cr_latent = None.
    check=True (the default): ONE stream synchronisation after the whole loop (not per step), then RuntimeError if a persistent
    stage launch gave up during it -- where the reference's loop would have raised (test_refiner.py:89-91), so that the last batch
    of a val_loop cannot end with rc 0 and NaN images.  check=False only enqueues the work (the returned latents are NaN in the
    failing case either way; `model.check()` reports it later).  bench.py times the loop with its own synchronisation."""
    e = model.engine
    e.ensure(latents.device)
    if latents.shape[0] == 0:                              # empty batch: nothing to sample
        return latents.to(device=e.device, dtype=torch.float32).clone()
    if not e.conditional:
        if cr_face is not None or cr_latent is not None:
            raise RuntimeError("the unconditional Denoiser takes no cr_face / cr_latent")
        e.require_loaded()
        e.prepare_unconditional(latents.shape[0])
    elif prepare:
        model.prepare(cr_face, cr_latent)
    e.require_loaded()
    x = latents.to(device=e.device, dtype=torch.float32).contiguous().clone()
    ts, coef = scheduler.coefficient_table()
    ts, coef = ts.contiguous(), coef.contiguous()
    multistep = coef.shape[1] == 8                         # DPMSolverMultistepScheduler: one history term (hd_schedule_ms)
    sch = _lib.ScheduleMS() if multistep else _lib.Schedule()
    sch.n_steps = ts.numel()
    sch.timesteps = ctypes.cast(ts.data_ptr(), ctypes.POINTER(ctypes.c_float))
    sch.coef = ctypes.cast(coef.data_ptr(), ctypes.POINTER(ctypes.c_float))
    nptr = None
    if noise is not None:
        noise = noise.to(device=e.device, dtype=torch.float32).contiguous()
        if noise.numel() != ts.numel() * x.numel():
            raise RuntimeError("noise must be [n_steps, B, 4, L, L]")
        nptr = noise.data_ptr()
    stream = torch.cuda.current_stream(e.device).cuda_stream
    if start_steps is None:
        if n_iters is not None or resume:
            raise ValueError("n_iters / resume need start_steps")
        with torch.cuda.device(e.device):
            run = _lib.lib().hd_sample_multistep if multistep else _lib.lib().hd_sample
            _lib.check(run(e.ctx, x.data_ptr(), ctypes.byref(sch), nptr, int(seed), stream), e.ctx)
    else:
        B = x.shape[0]
        rows = torch.as_tensor(start_steps).to(device="cpu", dtype=torch.int32).flatten()
        if rows.numel() == 1:
            rows = rows.expand(B)
        rows = rows.contiguous()
        if rows.numel() != B:
            raise ValueError(f"start_steps must be an int or a [{B}] tensor")
        if n_iters is None:
            n_iters = ts.numel() - int(rows.min())
            if n_iters == 0:                               # every face starts past the last row (strength 0): nothing to run
                return x
        if resume and not multistep:
            raise ValueError("resume applies to multistep schedules only")
        rptr = ctypes.cast(rows.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        with torch.cuda.device(e.device):
            if multistep:
                rc = _lib.lib().hd_sample_rows_multistep(e.ctx, x.data_ptr(), ctypes.byref(sch), rptr, int(n_iters), int(bool(resume)),
                                                         nptr, int(seed), stream)
            else:
                rc = _lib.lib().hd_sample_rows(e.ctx, x.data_ptr(), ctypes.byref(sch), rptr, int(n_iters), nptr, int(seed), stream)
            _lib.check(rc, e.ctx)
    if check:
        e.check()
    return x
