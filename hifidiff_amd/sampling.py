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
from ._context import stream_ptr


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


def inpaint_start(scheduler, known, strength=1.0, noise=None, generator=None):
    """diffusers' inpaint start: returns (latents, start_steps, noise).  A face of strength 1 (`is_strength_max`) starts from the pure
    noise at row 0; otherwise this is img2img_start(scheduler, known, strength, noise): face f starts at row n - min(int(n * s_f), n) from
    add_noise(known_f, noise_f, timesteps[start_f]).  The returned noise is the `known_noise` of sample(mask=...) / set_mask: the one fixed
    noise tensor the kept region is re-noised with after every step."""
    B = known.shape[0]
    s = torch.as_tensor(strength, dtype=torch.float64).flatten().cpu()
    if s.numel() not in (1, B):
        raise ValueError(f"strength must be a float or a [{B}] tensor")
    if bool(((s < 0) | (s > 1)).any()):
        raise ValueError("strength must lie in [0, 1]")
    if noise is None:
        noise = torch.randn(known.shape, generator=generator, dtype=known.dtype,
                            device=generator.device if generator is not None else known.device)
    noise = noise.to(device=known.device, dtype=known.dtype)
    latents, start = img2img_start(scheduler, known, strength, noise=noise)
    full = (s.expand(B) if s.numel() == 1 else s) == 1
    if bool(full.any()):                                   # strength 1: the noise itself, not add_noise(known, noise, timesteps[0])
        idx = full.nonzero().flatten().to(known.device)
        latents[idx] = noise[idx]
    return latents, start, noise


def region_mask(boxes, latent_res, image_res=128, feather=0):
    """Latent mask [latent_res, latent_res] (fp32, CPU) of pixel boxes (x0, y0, x1, y1), half-open, in an image_res x image_res image: every
    latent pixel gets the fraction of its (image_res / latent_res)^2 pixel cell that the union of the boxes covers (1: resample).
    feather > 0: a box blur of (2 * feather + 1)^2 latent pixels with zero padding, so the values stay in [0, 1].  Host-only torch."""
    L, R = int(latent_res), int(image_res)
    if L < 1 or R % L != 0:
        raise ValueError("image_res must be a multiple of latent_res")
    cell = R // L
    px = torch.zeros((R, R), dtype=torch.float64)
    for b in boxes:
        if len(b) != 4:
            raise ValueError("a box is (x0, y0, x1, y1)")
        x0, y0, x1, y1 = (int(v) for v in b)
        if not (0 <= x0 <= x1 <= R and 0 <= y0 <= y1 <= R):
            raise ValueError(f"box {tuple(b)} must satisfy 0 <= x0 <= x1 <= {R} and 0 <= y0 <= y1 <= {R}")
        px[y0:y1, x0:x1] = 1.0
    m = px.reshape(L, cell, L, cell).mean(dim=(1, 3))
    f = int(feather)
    if f < 0:
        raise ValueError("feather must be >= 0")
    if f > 0:
        k = 2 * f + 1
        m = torch.nn.functional.avg_pool2d(m[None, None], k, stride=1, padding=f, count_include_pad=True)[0, 0]
    return m.clamp(0.0, 1.0).to(torch.float32)


def low_pass(x, N):
    """LP_N of the guidance (model.set_guidance): every L x L plane of x [..., L, L] is replaced by the mean over its N x N blocks, upsampled
    bilinearly back to L x L with align_corners=False -- F.interpolate(F.avg_pool2d(x, N), size=L, mode="bilinear"), in closed form: for
    output index i in either axis s = max((i + 0.5)/N - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, P - 1), frac = s - i0 with P = L/N.  N = 1
    returns x itself (as a copy), N = L the plane mean everywhere.  Any device, any floating dtype; ValueError unless N divides L."""
    x = torch.as_tensor(x)
    if x.dim() < 2 or x.shape[-1] != x.shape[-2]:
        raise ValueError(f"low_pass needs square planes [..., L, L], got {tuple(x.shape)}")
    if isinstance(N, bool) or not isinstance(N, int):
        raise ValueError(f"N must be an int, got {N!r}")
    L = int(x.shape[-1])
    if N < 1 or L % N != 0:
        raise ValueError(f"N = {N} does not divide the plane size {L}")
    if N == 1:
        return x.clone()
    P = L // N
    bm = x.reshape(x.shape[:-2] + (P, N, P, N)).mean(dim=(-3, -1))
    i = torch.arange(L, device=x.device, dtype=torch.float64)
    s = ((i + 0.5) / N - 0.5).clamp(min=0.0)
    i0 = s.floor().long()
    i1 = (i0 + 1).clamp(max=P - 1)
    f = (s - i0.to(s.dtype)).to(x.dtype)
    rows = (1 - f)[:, None] * bm[..., i0, :] + f[:, None] * bm[..., i1, :]           # [..., L, P]
    return (1 - f) * rows[..., i0] + f * rows[..., i1]


class ScheduleSet:
    """Several schedules as one table, for batches whose faces run different step counts or solvers (hd_sample_spans).

    schedulers: a dict name -> scheduler, or a list (the keys are then 0, 1, ..); every member has had set_timesteps called.  The members'
    coefficient tables are concatenated in order into one (timesteps [N], coef [N,8]) table -- a 7-column member (DDIM / DDPM) is padded
    with c7 = 0 -- and span(key) is the member's rows [begin, end) of it.  The table is cached like a scheduler's coefficient_table() and
    rebuilt when a member's table changes (a new set_timesteps).  The library keeps one FiLM row per table row (0.5 MB at latent 16), so
    the memory price of a set is that of the sum of its members' lengths."""

    def __init__(self, schedulers):
        items = list(schedulers.items()) if isinstance(schedulers, dict) else list(enumerate(schedulers))
        if not items:
            raise ValueError("a ScheduleSet needs at least one scheduler")
        for k, m in items:
            ts = getattr(m, "timesteps", None)
            if ts is None or len(ts) == 0 or not hasattr(m, "coefficient_table"):
                raise ValueError(f"schedule {k!r} has no timesteps: call set_timesteps first")
        self.keys = [k for k, _ in items]
        self.members = dict(items)
        self._cache = None

    def __len__(self):
        return len(self.keys)

    def __contains__(self, key):
        return key in self.members

    def member(self, key):
        if key not in self.members:
            raise KeyError(f"no schedule {key!r} in the set (members: {self.keys})")
        return self.members[key]

    def _built(self):
        tabs = [self.members[k].coefficient_table() for k in self.keys]
        # the members hand out their cached tensors: a member's table has changed exactly when it returns another tensor
        ident = tuple((id(t), id(c)) for t, c in tabs)
        if self._cache is None or self._cache[0] != ident:
            coefs, spans, at = [], {}, 0
            for k, (t, c) in zip(self.keys, tabs):
                if c.shape[1] == 7:
                    c = torch.cat([c, torch.zeros((c.shape[0], 1), dtype=c.dtype)], dim=1)
                coefs.append(c)
                spans[k] = (at, at + int(t.numel()))
                at += int(t.numel())
            self._cache = (ident, tabs, torch.cat([t for t, _ in tabs]).contiguous(), torch.cat(coefs).contiguous(), spans)
        return self._cache

    def coefficient_table(self):
        """(timesteps [N] fp32, coef [N,8] fp32): the members' tables one after the other (hd_schedule_ms form); read-only for the caller."""
        b = self._built()
        return b[2], b[3]

    def span(self, key):
        """(begin, end): the member's rows of the concatenated table."""
        self.member(key)
        return self._built()[4][key]

    def spans(self, schedules, B):
        """schedules (one key, or one key per face) -> (begin [B], end [B]) int32 CPU tensors."""
        if isinstance(schedules, (list, tuple)):
            keys = list(schedules)
        else:
            keys = [schedules] * B
        if len(keys) != B:
            raise ValueError(f"schedules must be one key or {B} keys (one per face), got {len(keys)}")
        se = [self.span(k) for k in keys]
        return (torch.tensor([b for b, _ in se], dtype=torch.int32), torch.tensor([e for _, e in se], dtype=torch.int32))


@torch.no_grad()
def sample(model, latents, cr_face, cr_latent, scheduler, noise=None, seed=0, prepare=True, check=True,
           start_steps=None, n_iters=None, resume=False, face_seeds=None, mask=None, known=None, known_noise=None, schedules=None,
           previews=None, guide=None, guide_weight=1.0, guide_scale=4, guide_rows=None):
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
    face_seeds: None, or one Philox key per face (int list / int64 tensor [B]): face f's z at row k, element e of the face is
    Philox(face_seeds[f]; k, e), independent of its slot and its neighbours (diffusers' `generator=[...]`).  resume may also be a
    [B] bool tensor (multistep): True continues that face's history, False takes its first row first-order (a slot refilled by
    FacialRefiner.prepare_slots).  Either one dispatches to hd_sample_faces / hd_sample_faces_multistep (start_steps default 0).
    For the unconditional `Denoiser` pass cr_face = cr_latent = None.
    mask / known / known_noise (inpainting; all three or none): [B,L,L] or [B,1,L,L] in [0, 1] (1: resample, 0: keep), [B,4,L,L] and
    [B,4,L,L] (inpaint_start): set on the engine after preparing (model.set_mask), so after every step the kept region is `known`
    re-noised to the next row, and exactly `known` after the last.  mask=None with prepare=True removes any mask the engine still holds
    (the conditioning cache can hit without a new prepare); with prepare=False the engine's masks are left alone (continuous batching,
    a loop split over calls).
    scheduler may be a ScheduleSet (per-request schedules, hd_sample_spans): `schedules` is then one member key or one per face, face f
    runs its member's rows only and is held after them, start_steps is relative to the face's own schedule (0 .. n_f, default 0), n_iters
    defaults to the longest remaining run, and resume (a bool or a [B] tensor) continues a face's history as above -- it needs
    start_steps[f] > 0.  A face's z counts rows from the start of its own schedule; an explicit noise tensor is indexed by the row of the
    concatenated table ([N, B, 4, L, L]).  With a plain scheduler `schedules` must stay None.
    guide (low-pass fidelity guidance; None: off): a [B,4,L,L] target -- usually cr_latent -- that every face's denoised estimate is pulled
    towards in the low frequencies, x0 <- x0 + w (LP_N(guide) - LP_N(x0)) (low_pass is LP_N): guide_weight w in (0, 1] (a float or [B]),
    guide_scale N, a divisor of L (an int or [B]; 1: every element, L: only each channel's mean), guide_rows (j0, j1) or [B,2]: the rows
    of each face's own schedule on which it is guided (None: all).  Set on the engine after preparing (model.set_guidance).  guide=None
    with prepare=True removes any guidance the engine still holds (the conditioning cache can hit without a new prepare); with
    prepare=False the engine's guidance is left alone (continuous batching, a loop split over calls).
    previews: None, or an int k >= 1: the call also returns every k-th denoised estimate of each face -- (latents, x0_snaps [S,B,4,L,L],
    rows [S,B] int32) with S = ceil(longest schedule / k) (at most 64): x0_snaps[s, f] is face f's x0 of row (s + 1) * k - 1 of its own
    schedule (a masked face: blended with its known latent) and rows[s, f] that row of the table, or zeros and -1 where the face did
    not run that row in this call.  The latents are bit for bit those of previews=None; previews are switched on for the call
    (model.enable_previews(k, S), which forgets earlier previews) and the model's own setting is restored afterwards.
    check=True (the default): ONE stream synchronisation after the whole loop (not per step), then RuntimeError if a persistent
    stage launch gave up during it -- where the reference's loop would have raised (test_refiner.py:89-91), so that the last batch
    of a val_loop cannot end with rc 0 and NaN images.  check=False only enqueues the work (the returned latents are NaN in the
    failing case either way; `model.check()` reports it later).  bench.py times the loop with its own synchronisation."""
    B = latents.shape[0]
    rows, spans = start_steps, None
    if previews is not None:                               # argument errors before any device work
        if isinstance(previews, bool) or not isinstance(previews, int) or previews < 1:
            raise ValueError(f"previews must be None or an int >= 1, got {previews!r}")
        longest = (max(e - b for b, e in (scheduler.span(k) for k in scheduler.keys)) if isinstance(scheduler, ScheduleSet)
                   else int(scheduler.coefficient_table()[0].numel()))
        n_snaps = -(-longest // previews)
        if n_snaps > 64:
            raise ValueError(f"previews={previews} would take {n_snaps} snapshots of a {longest}-row schedule; at most 64 are kept")
    if isinstance(scheduler, ScheduleSet):
        begin, end, rows = _span_args(scheduler, schedules, start_steps, B)
        spans = (begin, end)
    elif schedules is not None:
        raise ValueError("schedules needs a ScheduleSet as the scheduler")
    if face_seeds is not None:
        face_seeds = face_seeds_arg(face_seeds, B)
    if isinstance(resume, torch.Tensor) or spans is not None:
        resume = resume_arg(resume, B)
    if mask is None and (known is not None or known_noise is not None):
        raise ValueError("known / known_noise need a mask")
    if mask is not None:
        from .refiner import mask_args
        mask, known, known_noise = mask_args(mask, known, known_noise, B, model.engine.latent_res)
    if guide is not None:
        from .refiner import guidance_args
        guide = guidance_args(guide, guide_weight, guide_scale, guide_rows, B, model.engine.latent_res)
    e = model.engine
    e.ensure(latents.device)
    if B == 0:                                             # empty batch: nothing to sample
        x = latents.to(device=e.device, dtype=torch.float32).clone()
        if previews is None:
            return x
        return x, x.new_zeros((n_snaps,) + tuple(x.shape)), torch.zeros((n_snaps, 0), dtype=torch.int32, device=e.device)
    _ready(model, B, cr_face, cr_latent, prepare)
    if mask is not None:
        e.set_mask(mask, known, known_noise)
    elif prepare:
        e.clear_mask()
    if guide is not None:
        e.set_guidance(*guide)
    elif prepare and getattr(e, "guide_on", False):        # (an engine that never switched guidance on holds none)
        e.clear_guidance()
    x = latents.to(device=e.device, dtype=torch.float32).contiguous().clone()
    if previews is None:
        return _run(e, x, scheduler.coefficient_table(), rows, spans, n_iters, resume, face_seeds, noise, seed, check)
    before = e.preview_cfg
    e.enable_previews(previews, n_snaps)                   # after the prepare: every face starts without a preview
    try:
        x = _run(e, x, scheduler.coefficient_table(), rows, spans, n_iters, resume, face_seeds, noise, seed, check)
        snaps = [e.previews(None, s) for s in range(n_snaps)]
    finally:
        if before is None:
            e.disable_previews()
        else:
            e.enable_previews(*before)
    return x, torch.stack([p for p, _ in snaps]), torch.stack([r for _, r in snaps])


def _ready(model, B, cr_face=None, cr_latent=None, prepare=False):
    """The engine (device chosen) before a loop on a batch of B: weights loaded, the batch prepared (always for the unconditional
    Denoiser, else with prepare=True)."""
    e = model.engine
    if not e.conditional:
        if cr_face is not None or cr_latent is not None:
            raise RuntimeError("the unconditional Denoiser takes no cr_face / cr_latent")
        e.require_loaded()
        e.prepare_unconditional(B)
    elif prepare:
        model.prepare(cr_face, cr_latent)
    e.require_loaded()


def _run(e, x, table, start_steps=None, spans=None, n_iters=None, resume=False, face_seeds=None, noise=None, seed=0, check=True):
    """The one path to the library's sampling loop: runs it in place on x ([B,4,L,L] fp32 on the engine's device) and returns x.

    table: (timesteps [n], coef [n,7] or [n,8]).  The entry point follows sample()'s rule: spans ((begin, end) int32 [B] CPU tensors, with
    start_steps the absolute rows) -> hd_sample_spans; face_seeds (a face_seeds_arg array) or a tensor resume -> hd_sample_faces*;
    start_steps -> hd_sample_rows*; else hd_sample*; 8 columns pick the multistep form.  n_iters defaults to the longest remaining run,
    and when that is 0 nothing is called."""
    ts, coef = (t.contiguous() for t in table)
    n, B, multistep = ts.numel(), x.shape[0], coef.shape[1] == 8   # 8: DPMSolverMultistepScheduler, one history term (hd_schedule_ms)
    ptr = lambda t, ty=ctypes.c_int32: ctypes.cast(t.data_ptr(), ctypes.POINTER(ty))   # noqa: E731
    sch = _lib.ScheduleMS() if multistep else _lib.Schedule()
    sch.n_steps, sch.timesteps, sch.coef = n, ptr(ts, ctypes.c_float), ptr(coef, ctypes.c_float)
    nptr = None
    if noise is not None:
        noise = noise.to(device=e.device, dtype=torch.float32).contiguous()
        if noise.numel() != n * x.numel():
            raise RuntimeError("noise must be [n_steps, B, 4, L, L]")
        nptr = noise.data_ptr()
    L = _lib.lib()
    faces = spans is not None or face_seeds is not None or isinstance(resume, torch.Tensor)
    if start_steps is None and not faces:
        if n_iters is not None or resume:
            raise ValueError("n_iters / resume need start_steps")
        fn, args = (L.hd_sample_multistep if multistep else L.hd_sample), ()
    else:
        rows = _rows_arg(start_steps, B)
        bad_resume = (isinstance(resume, torch.Tensor) or resume) and not multistep
        if faces and bad_resume:
            raise ValueError("resume applies to multistep schedules only")
        if n_iters is None:
            n_iters = int(((n if spans is None else spans[1]) - rows).max())
            if n_iters == 0:                               # every face starts past its last row (strength 0): nothing to run
                return x
        if bad_resume:
            raise ValueError("resume applies to multistep schedules only")
        sptr = face_seeds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if face_seeds is not None else None
        res = resume_arg(resume, B) if faces and multistep else None
        if spans is not None:
            fn, args = L.hd_sample_spans, (ptr(spans[0]), ptr(spans[1]), ptr(rows), int(n_iters), ptr(res), sptr)
        elif faces and multistep:
            fn, args = L.hd_sample_faces_multistep, (ptr(rows), int(n_iters), ptr(res), sptr)
        elif faces:
            fn, args = L.hd_sample_faces, (ptr(rows), int(n_iters), sptr)
        elif multistep:
            fn, args = L.hd_sample_rows_multistep, (ptr(rows), int(n_iters), int(bool(resume)))
        else:
            fn, args = L.hd_sample_rows, (ptr(rows), int(n_iters))
    with torch.cuda.device(e.device):
        _lib.check(fn(e.ctx, x.data_ptr(), ctypes.byref(sch), *args, nptr, int(seed), stream_ptr(e.device)), e.ctx)
    if check:
        e.check()
    return x


def _rows_arg(start_steps, B):
    """start rows as an int32 [B] CPU tensor (None: 0 for every face)."""
    rows = torch.as_tensor(0 if start_steps is None else start_steps).to(device="cpu", dtype=torch.int32).flatten()
    if rows.numel() == 1:
        rows = rows.expand(B)
    rows = rows.contiguous()
    if rows.numel() != B:
        raise ValueError(f"start_steps must be an int or a [{B}] tensor")
    return rows


def face_seeds_arg(face_seeds, B):
    """face_seeds (int list / tuple / int tensor of B values in [-2**63, 2**64); negative int64 keys keep their bit pattern) -> uint64 [B]
    numpy array for hd_sample_faces*."""
    import numpy as np
    if isinstance(face_seeds, torch.Tensor):
        if face_seeds.dtype.is_floating_point or face_seeds.dtype == torch.bool:
            raise ValueError("face_seeds must hold integers")
        vals = [int(v) for v in face_seeds.flatten().cpu().tolist()]
    else:
        vals = [int(v) for v in face_seeds]
    if len(vals) != B:
        raise ValueError(f"face_seeds must hold {B} seeds (one per face), got {len(vals)}")
    if any(v < -(1 << 63) or v >= (1 << 64) for v in vals):
        raise ValueError("face_seeds must lie in [-2**63, 2**64)")
    return np.array([v & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64)   # int64 seeds keep their bit pattern


def resume_arg(resume, B):
    """resume (bool / [B] bool or 0/1 tensor) -> int32 [B] CPU tensor of 0/1 for hd_sample_faces_multistep."""
    r = torch.as_tensor(resume).flatten().cpu()
    if r.dtype.is_floating_point:
        raise ValueError("resume must be a bool or a [B] bool tensor")
    if r.numel() == 1:
        r = r.expand(B)
    if r.numel() != B:
        raise ValueError(f"resume must be a bool or a [{B}] tensor")
    if bool(((r != 0) & (r != 1)).any()):
        raise ValueError("resume holds 0 / 1 (False / True) per face")
    return r.to(torch.int32).contiguous()


def _span_args(sset, schedules, start_steps, B):
    """(begin, end, start) int32 [B] CPU tensors of a ScheduleSet call: start_steps is relative to each face's own schedule."""
    if schedules is None:
        raise ValueError("a ScheduleSet needs schedules=: one member key, or one per face")
    begin, end = sset.spans(schedules, B)
    rel = _rows_arg(start_steps, B)
    if bool(((rel < 0) | (rel > end - begin)).any()):
        f = int(((rel < 0) | (rel > end - begin)).nonzero()[0])
        raise ValueError(f"start_steps[{f}] = {int(rel[f])} outside face {f}'s schedule [0, {int(end[f] - begin[f])}]")
    return begin.contiguous(), end.contiguous(), (begin + rel).contiguous()


class SlotTable:
    """Slot bookkeeping of continuous batching (host only, no device): which request holds which slot of a batch of B, the schedule
    row each slot is at, and whether its multistep history is its own.

    A request placed in a slot starts at its own row (img2img_start's convention) and is "fresh": its first row is taken first-order
    (resume 0).  After a call of n_iters iterations every occupied slot advances by n_iters rows; a slot that ran at least one row has a
    history of its own from then on (resume 1), and a slot whose row reached n_steps is complete and free again.  An empty slot is held
    (start row n_steps) and is never resumed.

    Per-request schedules (ScheduleSet): assign(req, start_row, begin, end) gives the slot the span [begin, end) of a table of n_steps rows
    as its own schedule; start_row is a row of the table inside the span, and the slot is complete when it reaches `end`.  Without a span
    a slot's schedule is the whole table."""

    def __init__(self, batch, n_steps):
        if batch < 1 or n_steps < 1:
            raise ValueError("batch and n_steps must be >= 1")
        self.batch, self.n_steps = int(batch), int(n_steps)
        self.req = [None] * self.batch          # request id per slot (None: empty)
        self.row = [self.n_steps] * self.batch  # schedule row of the slot's next iteration
        self.fresh = [False] * self.batch       # True until the slot's request has run a row (first-order first row)
        self.begin = [0] * self.batch           # the slot's own schedule: rows [begin, end) of the table
        self.end = [self.n_steps] * self.batch

    def free_slots(self):
        return [i for i, r in enumerate(self.req) if r is None]

    def occupied(self):
        return [i for i, r in enumerate(self.req) if r is not None]

    def assign(self, req_id, start_row, begin=None, end=None):
        """Place a request in the lowest free slot at row start_row of its schedule [begin, end) (default: the whole table,
        0 <= begin <= start_row <= end <= n_steps); returns the slot."""
        begin, end = 0 if begin is None else int(begin), self.n_steps if end is None else int(end)
        if not 0 <= begin <= end <= self.n_steps:
            raise ValueError(f"span [{begin}, {end}) outside the table [0, {self.n_steps}]")
        if not begin <= int(start_row) <= end:
            raise ValueError(f"start row {start_row} outside [{begin}, {end}]")
        free = self.free_slots()
        if not free:
            raise RuntimeError("no free slot")
        i = free[0]
        self.req[i], self.row[i], self.fresh[i] = req_id, int(start_row), True
        self.begin[i], self.end[i] = begin, end
        return i

    def start_rows(self):
        """Start rows of the next call: the slot's row, n_steps (held) for an empty slot."""
        return [self.row[i] if self.req[i] is not None else self.n_steps for i in range(self.batch)]

    def begin_rows(self):
        """Begin rows of the next call (hd_sample_spans): the slot's span, n_steps for an empty slot (held: begin == start == end)."""
        return [self.begin[i] if self.req[i] is not None else self.n_steps for i in range(self.batch)]

    def end_rows(self):
        """End rows of the next call: the slot's span, n_steps for an empty slot."""
        return [self.end[i] if self.req[i] is not None else self.n_steps for i in range(self.batch)]

    def resume_flags(self):
        """Multistep resumption of the next call: 1 for a slot whose request has already run a row, else 0."""
        return [int(self.req[i] is not None and not self.fresh[i]) for i in range(self.batch)]

    def iters(self, limit):
        """Iterations of the next call: `limit`, or fewer when no occupied slot has that many rows left (0: nothing runs).  A slot that
        reaches its last row inside the call is held for the rest of it: refills come every `limit` iterations, not at every finish."""
        left = [self.end[i] - self.row[i] for i in self.occupied() if self.row[i] < self.end[i]]
        return min(int(limit), max(left)) if left else 0

    def progress(self, slot, row):
        """(rows done, rows of the schedule) of the request in `slot` whose latest preview was taken at table row `row` (hd_preview_read):
        row - begin + 1 of end - begin, relative to the slot's own schedule.  None for an empty slot, a request that has not run a row yet
        (its slot may still hold its predecessor's preview) or a row outside the slot's span."""
        if self.req[slot] is None or self.fresh[slot] or not self.begin[slot] <= int(row) < self.end[slot]:
            return None
        return int(row) - self.begin[slot] + 1, self.end[slot] - self.begin[slot]

    def advance(self, n_iters):
        """Account for a call of n_iters iterations; returns [(slot, request id)] of the requests it completed (their slots are free)."""
        done = []
        for i in self.occupied():
            if self.row[i] < self.end[i] and n_iters > 0:
                self.fresh[i] = False
            self.row[i] = min(self.row[i] + int(n_iters), self.end[i])
            if self.row[i] >= self.end[i]:
                done.append((i, self.req[i]))
                self.req[i], self.fresh[i] = None, False
        return done


class PoolTable:
    """Entry bookkeeping of the conditioning pool (host only, no device): which request holds which of `capacity` entries.

    take(req_ids) gives each request the lowest free entry and queues it as prepared; pop(n) hands the n oldest prepared requests back
    in submission order (FIFO) as (request id, entry) -- they are about to be committed to slots -- and release(entry) frees the entry
    of a committed request for the next take."""

    def __init__(self, capacity):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError("capacity must be an int >= 1")
        self.capacity = capacity
        self.req = [None] * capacity            # request id per entry (None: free)
        self.fifo = []                          # entries of the prepared, uncommitted requests, oldest first

    def free_entries(self):
        return [e for e, r in enumerate(self.req) if r is None]

    def pending(self):
        """[(request id, entry)] of the prepared requests no slot has taken yet, oldest first."""
        return [(self.req[e], e) for e in self.fifo]

    def take(self, req_ids):
        """Give each of req_ids (in submission order) a free entry, lowest first; returns the entries.  RuntimeError when fewer are free."""
        req_ids = list(req_ids)
        free = self.free_entries()
        if len(req_ids) > len(free):
            raise RuntimeError(f"no free entry: {len(req_ids)} requests for {len(free)} free entries of {self.capacity}")
        entries = free[:len(req_ids)]
        for e, r in zip(entries, req_ids):
            self.req[e] = r
        self.fifo += entries
        return entries

    def pop(self, n):
        """The n oldest prepared requests as [(request id, entry)]; their entries stay taken until release."""
        if not 0 <= n <= len(self.fifo):
            raise ValueError(f"{n} requests asked for, {len(self.fifo)} are prepared")
        out, self.fifo = [(self.req[e], e) for e in self.fifo[:n]], self.fifo[n:]
        return out

    def release(self, entry):
        """Free the entry of a committed request."""
        if self.req[entry] is None or entry in self.fifo:
            raise ValueError(f"entry {entry} is free or its request is not committed yet")
        self.req[entry] = None


class ContinuousSampler:
    """Continuous batching: a serving loop that keeps the B slots of one prepared batch busy.  A request that reaches the last row
    leaves its slot, and the next queued request takes it (FacialRefiner.prepare_slots replaces that slot's conditioning alone, nothing
    is recaptured); the other faces go on.  Every request's result depends on its own inputs and seed only, not on its slot or
    neighbours: its initial latents come from a CPU torch.Generator seeded with `seed`, its z (DDPM, SDE-DPM-Solver++) from device
    Philox keyed by the same seed per face (hd_sample_faces*).

        cs = ContinuousSampler(model, scheduler, batch=64, refill_every=5)    # scheduler.set_timesteps(n) first
        rid = cs.submit(cr_face, cr_latent, seed=7, strength=0.6)             # [3,128,128], [4,L,L]
        results = cs.drain()                                                  # {rid: [4,L,L] latents}

    step() runs one call of refill_every iterations (fewer when no slot has that many rows left) after refilling free slots from the
    queue; a face that reaches its last row inside the call is held (not evaluated further) until the next refill;
    poll() returns what has finished since the last poll.  The model is the sampler's own while it runs: any other prepare / forward
    on it replaces the batch.  For the unconditional Denoiser pass cr_face = cr_latent = None (pure-noise start, strength 1).

    Per-request schedules: pass a ScheduleSet instead of a scheduler and pick a member per request, submit(..., schedule=key) (default: the
    set's first member).  Requests of different step counts and solvers then share the batch (hd_sample_spans): each runs its own member's
    rows, its strength maps onto that member's row count, and its result is what it would be on that member alone.

    previews=True: previews() returns, between two step() calls, the progress and the current denoised estimate of every request that
    is in a slot and has run a row; like its result, a request's preview does not depend on its slot or neighbours.

    prefetch=P >= 1: the conditioning of queued requests is prepared ahead, up to P of them (and at most `batch`) in one
    FacialRefiner.pool_prepare call, and a refill copies it into the freed slots with one pool_commit -- the prologue costs about the
    same for 64 faces as for one, so refilling one or two slots at a time (refill_every=1) no longer pays it per refill.  The first fill
    stays one prepare of the whole batch.  A refill commits at most the requests the pool holds, so P below `batch` caps the slots filled
    per refill at P: the other free slots stay empty until the next step().  A request's conditioning is then computed at the batch size of its pool_prepare call instead
    of its refill; everything else about it is unchanged.  pool_calls / pool_prepared count the calls and the requests they prepared."""

    def __init__(self, model, scheduler, batch=64, refill_every=5, previews=False, prefetch=0):
        if batch < 1 or refill_every < 1:
            raise ValueError("batch and refill_every must be >= 1")
        if isinstance(prefetch, bool) or not isinstance(prefetch, int) or prefetch < 0:
            raise ValueError(f"prefetch must be an int >= 0, got {prefetch!r}")
        if prefetch and not model.engine.conditional:
            raise ValueError("prefetch needs the refiner: the unconditional Denoiser has no conditioning to prepare ahead")
        self.model, self.scheduler = model, scheduler
        self.prefetch = prefetch
        self.pool = None
        if prefetch:                    # the model keeps the pool (model.disable_pool())
            model.enable_pool(prefetch)
            self.pool = PoolTable(prefetch)
        self.want_previews = bool(previews)
        if self.want_previews:          # the latest estimate of every slot; the model keeps the setting (model.disable_previews())
            model.enable_previews(1, 0)
        self.batch, self.refill_every = int(batch), int(refill_every)
        self.conditional = model.engine.conditional
        self.L = model.engine.latent_res
        self.sset = scheduler if isinstance(scheduler, ScheduleSet) else None
        self.n_steps = int(scheduler.coefficient_table()[0].numel()) if self.sset else int(scheduler.timesteps.numel())
        self.table = SlotTable(self.batch, self.n_steps)
        self.queue = []                 # (rid, cr_face, cr_latent, seed, strength, mask, fidelity, schedule) in submission order
        self.finished = {}
        self.seeds = [0] * self.batch
        self.x = None                   # [B,4,L,L] device latents of every slot
        self.prepared = False
        self.next_id = 0
        self.calls = 0
        self.refilled = 0
        self.pool_calls = 0             # pool_prepare calls, and the requests they prepared
        self.pool_prepared = 0

    def submit(self, cr_face, cr_latent, seed, strength=1.0, mask=None, schedule=None, fidelity=None, fidelity_scale=4, fidelity_rows=None):
        """schedule: the member of the ScheduleSet this request runs (None: the first member; without a set it must stay None).
        mask: None, or [L,L] / [1,L,L] in [0, 1] (1: resample): the request is inpainted -- its known latent is cr_latent, the noise of
        the kept region the z its start is drawn from (inpaint_start; strength 1 starts from pure noise).  Masked and unmasked requests
        share a batch.
        fidelity: None, or a weight in (0, 1]: the request is guided towards its own cr_latent (model.set_guidance) with block size
        fidelity_scale (a divisor of L) on the rows fidelity_rows = (j0, j1) of its own schedule (None: all).  Guided and unguided requests
        share a batch."""
        L = self.L
        if self.sset is None:
            if schedule is not None:
                raise ValueError("schedule= needs a ContinuousSampler over a ScheduleSet")
        else:
            schedule = self.sset.keys[0] if schedule is None else schedule
            self.sset.member(schedule)
        if mask is not None:
            if not self.conditional:
                raise ValueError("a mask needs the refiner: the request's known latent is its cr_latent")
            from .refiner import mask_args
            mask = torch.as_tensor(mask)
            if cr_latent is None:
                raise ValueError("the refiner needs cr_face and cr_latent")
            mask = mask_args(mask[None] if mask.dim() == 2 else mask, cr_latent[None], cr_latent[None], 1, L)[0][0].cpu()
        if fidelity is not None:
            if not self.conditional:
                raise ValueError("fidelity needs the refiner: the request's target is its cr_latent")
            if cr_latent is None:
                raise ValueError("the refiner needs cr_face and cr_latent")
            from .refiner import guidance_args
            _, w, N, r = guidance_args(torch.as_tensor(cr_latent)[None], fidelity, fidelity_scale, fidelity_rows, 1, L)
            fidelity = (float(w[0]), int(N[0]), None if r is None else (int(r[0, 0]), int(r[0, 1])))
        if self.conditional:
            if cr_face is None or cr_latent is None:
                raise ValueError("the refiner needs cr_face and cr_latent")
            if tuple(cr_latent.shape) != (4, L, L) or tuple(cr_face.shape) != (3, 128, 128):
                raise ValueError(f"expected cr_face (3,128,128) and cr_latent (4,{L},{L}), got {tuple(cr_face.shape)} and {tuple(cr_latent.shape)}")
        elif cr_face is not None or cr_latent is not None or float(strength) != 1.0:
            raise ValueError("the unconditional Denoiser takes no cr_face / cr_latent and starts from noise (strength 1)")
        if not 0.0 <= float(strength) <= 1.0:
            raise ValueError("strength must lie in [0, 1]")
        seed = int(seed)
        if not 0 <= seed < (1 << 63):
            raise ValueError("seed must lie in [0, 2**63)")
        rid = self.next_id
        self.next_id += 1
        self.queue.append((rid, cr_face, cr_latent, seed, float(strength), mask, fidelity, schedule))
        return rid

    def _z(self, seed):
        """The request's one CPU-generator noise tensor [1,4,L,L]: its start is drawn from it, and a masked request's kept region is
        re-noised with it."""
        return torch.randn((1, 4, self.L, self.L), generator=torch.Generator().manual_seed(seed))

    def _start(self, cr_latent, seed, strength, masked=False, schedule=None):
        """(initial latents [4,L,L] on the CPU, start row) of one request: img2img_start (inpaint_start for a masked request) with a CPU
        generator seeded by the request.  Over a ScheduleSet the start row is relative to the request's member `schedule`, whose
        timesteps and row count the strength maps onto."""
        sch = self.scheduler if self.sset is None else self.sset.member(self.sset.keys[0] if schedule is None else schedule)
        z = self._z(seed)
        if cr_latent is None:
            return z[0], 0
        if masked:
            lat, start, _ = inpaint_start(sch, cr_latent.detach().float().cpu()[None], strength, noise=z)
        else:
            lat, start = img2img_start(sch, cr_latent.detach().float().cpu()[None], strength, noise=z)
        return lat[0], int(start[0])

    @staticmethod
    def _upload(tensors, dev):
        """n tensors of one kind as [n, ...] fp32 on the device: one host-to-device transfer when they all live on the host."""
        ts = [t.detach().to(torch.float32) for t in tensors]
        if all(t.device.type == "cpu" for t in ts):
            return torch.stack(ts).to(dev)
        return torch.stack([t.to(dev) for t in ts])

    def _top_up(self, dev, n_free):
        """Prepare queued requests ahead when fewer are prepared than slots are free: min(unprepared, free entries, batch) of them, in
        submission order, in one pool_prepare call.  The prepared requests are the head of the queue, in order."""
        ahead = len(self.pool.pending())
        unprepared = len(self.queue) - ahead
        if ahead >= n_free or unprepared < 1:
            return
        k = min(unprepared, len(self.pool.free_entries()), self.batch)
        if k < 1:
            return
        reqs = self.queue[ahead:ahead + k]
        entries = self.pool.take([r[0] for r in reqs])
        self.model.pool_prepare(entries, self._upload([r[1] for r in reqs], dev), self._upload([r[2] for r in reqs], dev))
        self.pool_calls += 1
        self.pool_prepared += k

    def _refill(self, dev):
        free = self.table.free_slots()
        pooled = self.pool is not None and self.prepared      # the first fill is one prepare of the whole batch
        if pooled and free and self.queue:
            self._top_up(dev, len(free))
        n_new = min(len(self.queue), len(free), len(self.pool.pending()) if pooled else len(free))
        new, lats, masked, guided = [], [], [], []
        for _ in range(n_new):
            rid, crf, crl, seed, strength, mask, fidelity, schedule = self.queue.pop(0)
            lat, start = self._start(crl, seed, strength, mask is not None, schedule)
            if self.sset is None:
                slot = self.table.assign(rid, start)
            else:
                begin, end = self.sset.span(schedule)
                slot = self.table.assign(rid, begin + start, begin, end)
            self.seeds[slot] = seed
            lats.append(lat)
            new.append((slot, crf, crl))
            if mask is not None:
                masked.append((slot, mask, crl, self._z(seed)[0]))
            if fidelity is not None:
                guided.append((slot, crl, fidelity))
        if not new:
            return
        slots = [s for s, _, _ in new]
        self.x[slots] = self._upload(lats, dev)
        if not self.conditional:
            return
        if pooled:                      # the conditioning is in the pool already: the oldest prepared requests are these
            took = self.pool.pop(len(slots))
            self.model.pool_commit(slots, [e for _, e in took])
            for _, e in took:
                self.pool.release(e)
            self.refilled += len(slots)
        else:
            crf, crl = self._upload([f for _, f, _ in new], dev), self._upload([l for _, _, l in new], dev)
            if not self.prepared:       # the first batch: the whole batch is prepared once (empty slots get zeros; they are held)
                B, L = self.batch, self.L
                full_f = torch.zeros((B, 3, 128, 128), device=dev)
                full_l = torch.zeros((B, 4, L, L), device=dev)
                full_f[slots], full_l[slots] = crf, crl
                self.model.prepare(full_f, full_l)
                self.model.engine.cond_key = None      # the batch belongs to the sampler: no cache hit on these tensors later
                self.prepared = True
            else:
                self.model.prepare_slots(slots, crf, crl)
                self.refilled += len(slots)
        if masked:                      # after the prepare: it has cleared the masks of the slots it filled
            self.model.set_mask(torch.stack([m for _, m, _, _ in masked]), torch.stack([l.detach().float().cpu() for _, _, l, _ in masked]),
                                torch.stack([z for _, _, _, z in masked]), slots=[s for s, _, _, _ in masked])
        if guided:                      # likewise: the prepare has cleared the guidance of the slots it filled
            big = 0x7fffffff            # "all rows" next to requests that gave a window
            self.model.set_guidance(torch.stack([l.detach().float().cpu() for _, l, _ in guided]), torch.tensor([f[0] for _, _, f in guided]),
                                    torch.tensor([f[1] for _, _, f in guided]),
                                    rows=torch.tensor([f[2] if f[2] is not None else (0, big) for _, _, f in guided]), slots=[s for s, _, _ in guided])

    def step(self):
        """Refill free slots from the queue, then run one call of up to refill_every iterations.  Returns the number of iterations."""
        e = self.model.engine
        dev = torch.device("cuda", torch.cuda.current_device()) if e.device is None else e.device
        if self.x is None:
            self.x = torch.zeros((self.batch, 4, self.L, self.L), device=dev)
        self._refill(dev)
        n = self.table.iters(self.refill_every)
        if n > 0:                       # the slots' rows (and spans) go to the library as they stand in the table
            t, i32 = self.table, lambda v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
            table = self.scheduler.coefficient_table()
            e.ensure(self.x.device)
            _ready(self.model, self.batch)
            x = self.x.to(device=e.device, dtype=torch.float32).contiguous().clone()
            self.x = _run(e, x, table, i32(t.start_rows()), None if self.sset is None else (i32(t.begin_rows()), i32(t.end_rows())), n,
                          i32(t.resume_flags()) if table[1].shape[1] == 8 else False, face_seeds_arg(self.seeds, self.batch))
            self.calls += 1
        for slot, rid in self.table.advance(n):
            self.finished[rid] = self.x[slot].clone()
        return n

    def previews(self):
        """{request id: (rows_done, rows_total, x0 [4,L,L] on the device)} of every request in a slot that has run a row: rows_done of the
        rows_total rows of its own schedule (from its start row on: a request of strength < 1 begins with rows_done > 1), and the x0 of
        the last of them.  A request that finished in the last step() has left its slot: poll() has its result."""
        if not self.want_previews:
            raise RuntimeError("this ContinuousSampler was created without previews=True")
        slots = [i for i in self.table.occupied() if not self.table.fresh[i]]
        if not slots:
            return {}
        x0, rows = self.model.previews(slots)
        out = {}
        for j, (slot, row) in enumerate(zip(slots, rows.cpu().tolist())):
            p = self.table.progress(slot, row)
            if p is not None:
                out[self.table.req[slot]] = (p[0], p[1], x0[j])
        return out

    def busy(self):
        return bool(self.queue) or bool(self.table.occupied())

    def poll(self):
        """Finished requests since the last poll: {request id: final latents [4,L,L] (device)}."""
        out, self.finished = self.finished, {}
        return out

    def drain(self):
        """Run until every submitted request has finished; returns poll()."""
        while self.busy():
            self.step()
        return self.poll()
