"""Masked sampling (inpainting) in the graph-replayed loop: hd_mask_faces and sampling.sample(mask=...).

After the update of row k has produced r, a masked face ends the row on m*r + (1 - m)*(c1[k+1]*known + c0[k+1]*nz), and on `known` where
m == 0 after the last row.  In that order m == 1 returns r and m == 0 the re-noised known latent exactly, so a binary mask composes bit
for bit with the unmasked one-row step, and the unmasked path is compared bit for bit with itself before and after mask calls.  As in
tests/test_start_rows.py the bit-for-bit comparisons between hd_sample and the per-face form run with "xcd2" off.  Where fma contraction
is the compiler's choice (0 < m < 1, or the re-noised latent itself) the bound is 1e-5: two fp32 roundings on values of magnitude <= 5."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from conftest import rel_l2, weights16  # noqa: F401  (weights16: session fixture)

ERR_INVALID, ERR_NOT_READY = -1, -4
BLEND_TOL = 1e-5                                  # two fp32 roundings on values of magnitude <= 5 (module docstring)
TRAJ_TOL = 1e-2                                   # tests/test_slots.py: a request in a batch against the same request alone


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


def _L():
    from hifidiff_amd import _lib
    return _lib.lib()


def make_model(weights, latent=16):
    from hifidiff_amd.refiner import FacialRefiner
    m = FacialRefiner(latent)
    m.load_state_dict(weights)
    m.to("cuda:0")
    return m


def make_denoiser(weights):
    from hifidiff_amd.refiner import Denoiser
    u = Denoiser(16)
    n = len("denoiser.")
    u.load_state_dict({k[n:]: v for k, v in weights.items() if k.startswith("denoiser.") and ".hcas." not in k and ".idc_conv" not in k})
    u.to("cuda:0")
    return u


def free(m):
    del m
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class Runner:
    """Direct C-ABI calls on a prepared context (tests/test_start_rows.py's Runner, with the mask call)."""

    def __init__(self, m, crf=None, crl=None, B=None):
        self.m, self.e = m, m.engine
        if crl is not None:
            m.prepare(crf.cuda(), crl.cuda())
        else:
            self.e.ensure(torch.device("cuda", 0))
            self.e.prepare_unconditional(B)

    @property
    def ctx(self):
        return self.e.ctx

    def opt(self, key):
        return _L().hd_get_option(self.ctx, key.encode())

    def counters(self):
        return (self.opt("graph_captures"), _L().hd_num_ops(self.ctx, 0), self.opt("sample_stage_launches"), self.opt("rows_stage_launches"))

    def _sch(self, ts, coef):
        from hifidiff_amd import _lib
        self._keep = (ts.float().contiguous(), coef.float().contiguous())
        ts, coef = self._keep
        sch = _lib.ScheduleMS() if coef.shape[1] == 8 else _lib.Schedule()
        sch.n_steps = ts.numel()
        sch.timesteps = ctypes.cast(ts.data_ptr(), ctypes.POINTER(ctypes.c_float))
        sch.coef = ctypes.cast(coef.data_ptr(), ctypes.POINTER(ctypes.c_float))
        return sch

    def _run(self, rc):
        from hifidiff_amd import _lib
        _lib.check(rc, self.ctx)
        torch.cuda.synchronize()
        _lib.check(_L().hd_check(self.ctx), self.ctx)

    def mask_rc(self, mask, known, nz, slots=None, n=None):
        """hd_mask_faces; mask None clears.  The device copies are kept until the stream has passed the call."""
        dev = [None if t is None else t.cuda().float().contiguous() for t in (mask, known, nz)]
        sl = None if slots is None else torch.as_tensor(slots, dtype=torch.int32).contiguous()
        if n is None:
            n = sl.numel() if sl is not None else self.e.batch
        sp = None if sl is None else ctypes.cast(sl.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        rc = _L().hd_mask_faces(self.ctx, n, sp, *[None if t is None else t.data_ptr() for t in dev], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def mask(self, mask, known, nz, slots=None):
        assert self.mask_rc(mask, known, nz, slots) == 0, _L().hd_last_error(self.ctx)

    def clear(self, slots=None):
        assert self.mask_rc(None, None, None, slots) == 0, _L().hd_last_error(self.ctx)

    def full(self, x, ts, coef, noise=None, seed=0):
        xd = x.cuda().float().contiguous().clone()
        nd = None if noise is None else noise.cuda().float().contiguous()
        sch = self._sch(ts, coef)
        fn = _L().hd_sample_multistep if coef.shape[1] == 8 else _L().hd_sample
        self._run(fn(self.ctx, xd.data_ptr(), ctypes.byref(sch), None if nd is None else nd.data_ptr(), seed,
                     torch.cuda.current_stream().cuda_stream))
        return xd.cpu()

    def rows(self, x, ts, coef, rows, n_iters, resume=0, seed=0):
        xd = x.cuda().float().contiguous().clone()
        sch = self._sch(ts, coef)
        r = torch.as_tensor(rows, dtype=torch.int32).contiguous()
        rp = ctypes.cast(r.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        s = torch.cuda.current_stream().cuda_stream
        if coef.shape[1] == 8:
            rc = _L().hd_sample_rows_multistep(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, resume, None, seed, s)
        else:
            rc = _L().hd_sample_rows(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, None, seed, s)
        self._run(rc)
        return xd.cpu()

    def faces(self, x, ts, coef, rows, n_iters, seeds):
        xd = x.cuda().float().contiguous().clone()
        sch = self._sch(ts, coef)
        r = torch.as_tensor(rows, dtype=torch.int32).contiguous()
        rp = ctypes.cast(r.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        self._run(_L().hd_sample_faces(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                       None, 0, torch.cuda.current_stream().cuda_stream))
        return xd.cpu()

    def read(self, name, shape):
        n = _L().hd_debug_read(self.ctx, name.encode(), None, 0)
        assert n == int(np.prod(shape)), (name, n, shape)
        buf = np.empty(n, dtype=np.float32)
        assert _L().hd_debug_read(self.ctx, name.encode(), buf.ctypes.data, n) == n
        return torch.from_numpy(buf.reshape(shape))


def _tables(kind, n):
    from hifidiff_amd import schedulers
    s = {"ddim": lambda: schedulers.DDIMScheduler(clip_sample_range=3.0), "ddpm": lambda: schedulers.DDPMScheduler(clip_sample_range=3.0),
         "dpm": lambda: schedulers.DPMSolverMultistepScheduler()}[kind]()
    s.set_timesteps(n)
    ts, coef = s.coefficient_table()
    return s, ts.float().contiguous(), coef.float().contiguous()


def box(B, L, y0, y1, x0, x1):
    """A fixed binary box mask [B,L,L] (1 inside: resample) that covers between 20 % and 80 % of the latent pixels."""
    m = torch.zeros((B, L, L))
    m[:, y0:y1, x0:x1] = 1.0
    cover = float(m.mean())
    assert 0.2 <= cover <= 0.8, cover
    return m


def _kn64(coef, k, known, nz):
    """The known latent re-noised to row k in float64 (the table's fp32 coefficients): c1[k]*known + c0[k]*nz; `known` past the last row."""
    if k >= coef.shape[0]:
        return known.double()
    return float(coef[k, 1]) * known.double() + float(coef[k, 0]) * nz.double()


@pytest.fixture(scope="module")
def data(gpu):
    from hifidiff_amd import synth
    x, crl, crf = synth.sample_inputs(64, 16)
    return x, crl, crf


@pytest.fixture(scope="module")
def run64(gpu, weights16, data):
    """Batch 64, known = the coarse latent, noise = the initial latents; the K-split form at level 2 in both forms of the graphs."""
    x, crl, crf = data
    m = make_model(weights16)
    run = Runner(m, crf, crl)
    _L().hd_set_option(m.engine.ctx, b"xcd2", 0)
    yield run
    free(m)


# ------------------------------------------------------------------------------------------------ 1. the unmasked path is untouched
@pytest.mark.gpu
def test_unmasked_path_is_untouched(run64, data):
    x, crl, _ = data
    _, ts, coef = _tables("ddim", 50)
    rows = [(0, 7, 25, 49, 50)[f % 5] for f in range(64)]
    base, base_rows = run64.full(x, ts, coef), run64.rows(x, ts, coef, rows, 50)
    before = run64.counters()
    assert run64.opt("masked_faces") == 0
    run64.mask(box(64, 16, 4, 12, 2, 14), crl, x)
    assert run64.opt("masked_faces") == 64
    run64.clear()
    assert run64.opt("masked_faces") == 0
    assert torch.equal(run64.full(x, ts, coef), base)
    assert torch.equal(run64.rows(x, ts, coef, rows, 50), base_rows)
    run64.mask(torch.ones((64, 16, 16)), crl, x)                      # m == 1 everywhere: r comes back exactly
    assert torch.equal(run64.full(x, ts, coef), base)
    assert torch.equal(run64.rows(x, ts, coef, rows, 50), base_rows)
    run64.clear()
    assert run64.counters() == before, (run64.counters(), before)


# ------------------------------------------------------------------------------------------------ 2. the kept region is exact
def _check_kept(run, x, known, nz, kind, n, k_part, **kw):
    B, L = x.shape[0], x.shape[-1]
    _, ts, coef = _tables(kind, n)
    run.mask(torch.zeros((B, L, L)), known, nz)
    try:
        assert torch.equal(run.full(x, ts, coef, **kw), known.float()), kind
        assert torch.equal(run.rows(x, ts, coef, [0] * B, n, **kw), known.float()), kind
        got = run.rows(x, ts, coef, [0] * B, k_part, **kw)
        err = float((got.double() - _kn64(coef, k_part, known, nz)).abs().max())
        print(f"kept region after {k_part} of {n} {kind} rows: max abs {err:.3e} from the float64 re-noised latent")
        assert err <= BLEND_TOL, (kind, err)
    finally:
        run.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("ddim", 50), ("dpm", 20), ("ddpm", 20)])
def test_kept_region_is_exact(run64, data, kind, n):
    x, crl, _ = data
    _check_kept(run64, x, crl, x, kind, n, 7, **({"seed": 11} if kind == "ddpm" else {}))


# ------------------------------------------------------------------------------------------------ 3. a binary mask composes bit for bit
def _check_compose(run, x, known, nz, mask, kind, n, iters=8):
    """x_{i+1} = where(m == 1, one unmasked row from x_i, kn_i) -- kn_i read from the device's own m == 0 run -- equals the masked loop's x
    after i + 1 iterations; the multistep form steps with resume = 1, so the history has to be the unblended x0 of the masked loop too."""
    B, L = x.shape[0], x.shape[-1]
    _, ts, coef = _tables(kind, n)
    try:
        run.mask(torch.zeros((B, L, L)), known, nz)
        kn = [run.rows(x, ts, coef, [0] * B, i + 1) for i in range(iters)]
        run.mask(mask, known, nz)
        masked = [run.rows(x, ts, coef, [0] * B, i + 1) for i in range(iters)]
    finally:
        run.clear()
    sel = (mask == 1)[:, None].expand_as(x)
    assert bool(((mask == 0) | (mask == 1)).all())
    xi = x.float()
    for i in range(iters):
        u = run.rows(xi, ts, coef, [i] * B, 1, resume=int(i > 0))
        xi = torch.where(sel, u, kn[i])
        assert torch.equal(xi, masked[i]), (kind, i, float((xi - masked[i]).abs().max()))
    assert not torch.equal(masked[-1][sel], kn[-1][sel])              # the masked region is resampled, not kept


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("ddim", 50), ("dpm", 20)])
def test_binary_mask_composes_with_the_unmasked_step(run64, data, kind, n):
    x, crl, _ = data
    assert run64.opt("end_fold") == 1                                 # the fused ending launch (hca_ending_conv_kernel)
    _check_compose(run64, x, crl, x, box(64, 16, 3, 13, 5, 16), kind, n)


@pytest.mark.gpu
def test_binary_mask_composes_on_the_unconditional_denoiser(gpu, weights16, data):
    x, crl = data[0][:4], data[1][:4]
    u = make_denoiser(weights16)
    run = Runner(u, B=4)
    _L().hd_set_option(u.engine.ctx, b"xcd2", 0)
    assert run.opt("end_fold") == 0                                   # ending_conv_kernel
    _check_compose(run, x, crl, x, box(4, 16, 0, 9, 2, 12), "ddim", 20)
    _check_compose(run, x, crl, x, box(4, 16, 0, 9, 2, 12), "dpm", 20)
    _check_kept(run, x, crl, x, "ddim", 20, 5)
    free(u)


# ------------------------------------------------------------------------------------------------ 4. soft mask
@pytest.mark.gpu
def test_soft_mask_against_the_float64_formula(run64, data):
    from hifidiff_amd import sampling
    x, crl, _ = data
    m1 = sampling.region_mask([(24, 16, 104, 96)], 16, feather=2)
    assert 0.2 <= float(m1.mean()) <= 0.8 and bool(((m1 > 0) & (m1 < 1)).any())
    m = m1[None].expand(64, 16, 16).contiguous()
    for kind in ("ddim", "dpm"):
        _, ts, coef = _tables(kind, 20)
        u = run64.rows(x, ts, coef, [0] * 64, 1)
        run64.mask(m, crl, x)
        try:
            got = run64.rows(x, ts, coef, [0] * 64, 1)
        finally:
            run64.clear()
        md = m[:, None].double()
        want = md * u.double() + (1.0 - md) * _kn64(coef, 1, crl, x)
        err = float((got.double() - want).abs().max())
        print(f"soft mask, one {kind} row: max abs {err:.3e} from the float64 formula")
        assert err <= BLEND_TOL, (kind, err)


# ------------------------------------------------------------------------------------------------ 5. against the oracle network
@pytest.mark.gpu
def test_against_the_oracle_network(gpu, weights16):
    """tests/test_multistep.py::test_against_the_oracle_network's loop with the blend added in float64 after each update."""
    from hifidiff_amd import sampling, schedulers, synth
    from oracle import hifidiff_oracle as O
    from test_multistep import _update64
    x, crl, crf = synth.sample_inputs(2, 16)
    s = schedulers.DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    ts, coef = s.coefficient_table()
    mask = box(2, 16, 4, 12, 3, 13)
    md = mask[:, None].double()
    cond = O.Conditioning(weights16, crl, crf, prec=O.BF16)
    xr, h = x.double(), None
    for i, t in enumerate(s.timesteps.tolist()):
        eps = O.fused_denoiser(weights16, xr.float(), torch.full((x.shape[0],), t), prec=O.BF16, cond=cond).double()
        r, h = _update64(xr, eps, coef[i], h)
        xr = md * r + (1.0 - md) * _kn64(coef, i + 1, crl, x)
    model = make_model(weights16)
    got = sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), s, mask=mask, known=crl, known_noise=x).cpu()
    r = rel_l2(got, xr)
    print(f"masked DPM-Solver++ 2M, 10 steps, against the oracle network: rel-L2 {r:.3e}")
    assert r <= 2e-2, r
    keep = (mask == 0)[:, None].expand_as(got)
    assert torch.equal(got[keep], crl.float()[keep])
    free(model)


# ------------------------------------------------------------------------------------------------ 6. per face
@pytest.mark.gpu
def test_masks_are_per_face(run64, data):
    x, crl, _ = data
    _, ts, coef = _tables("ddpm", 20)
    seeds = [900 + 3 * f for f in range(64)]
    ma, mb = box(64, 16, 2, 10, 2, 14), box(64, 16, 6, 16, 0, 9)
    plain = run64.faces(x, ts, coef, [0] * 64, 20, seeds)
    try:
        run64.mask(ma[:16], crl[:16], x[:16], slots=list(range(16)))
        run64.mask(mb[:16], crl[16:32], x[16:32], slots=list(range(16, 32)))
        assert run64.opt("masked_faces") == 32
        mixed = run64.faces(x, ts, coef, [0] * 64, 20, seeds)
        got_mask = run64.read("mask", (64, 16, 16))
        assert torch.equal(got_mask[:16], ma[:16]) and torch.equal(got_mask[16:32], mb[:16])
        assert torch.equal(run64.read("mask_known", (64, 4, 16, 16))[:32], crl[:32].float())
        assert torch.equal(run64.read("mask_noise", (64, 4, 16, 16))[:32], x[:32].float())
        run64.mask(ma, crl, x)
        all_a = run64.faces(x, ts, coef, [0] * 64, 20, seeds)
        run64.mask(mb, crl, x)
        all_b = run64.faces(x, ts, coef, [0] * 64, 20, seeds)
    finally:
        run64.clear()
    assert torch.equal(mixed[32:], plain[32:])
    assert torch.equal(mixed[:16], all_a[:16]) and torch.equal(mixed[16:32], all_b[16:32])
    assert not torch.equal(mixed[:32], plain[:32])
    keep = (ma == 0)[:16, None].expand(16, 4, 16, 16)
    assert torch.equal(mixed[:16][keep], crl[:16].float()[keep])


# ------------------------------------------------------------------------------------------------ 8. continuous batching
@pytest.mark.gpu
def test_continuous_sampler_with_masks(run64, data):
    """24 requests through 8 slots, every other one masked, strengths mixed: each result against the same request sampled alone in slot 0,
    within TRAJ_TOL as tests/test_slots.py compares a request of a batch with the request alone (the conditioning of a refill is computed
    at another batch size); the kept region of a masked request is its coarse latent exactly."""
    from hifidiff_amd import sampling
    _, crl, crf = data
    s, _, _ = _tables("ddpm", 10)
    N = 24
    strength = [(1.0, 0.35, 0.6, 0.85)[i % 4] for i in range(N)]
    masks = [None if i % 2 else (box(1, 16, 4, 12, 2, 14), box(1, 16, 0, 8, 4, 16))[(i // 2) % 2][0] for i in range(N)]
    m = run64.m
    cs = sampling.ContinuousSampler(m, s, batch=8, refill_every=3)
    ids = [cs.submit(crf[i], crl[i], seed=700 + i, strength=strength[i], mask=masks[i]) for i in range(N)]
    out = cs.drain()
    assert sorted(out) == ids and cs.refilled >= N - 8
    worst, exact = 0.0, 0
    for i in ids:
        lat, start = cs._start(crl[i], 700 + i, strength[i], masks[i] is not None)
        z = cs._z(700 + i)[0]
        kw = {} if masks[i] is None else dict(mask=masks[i][None], known=crl[i][None], known_noise=z[None])
        got = sampling.sample(m, lat[None].cuda(), crf[i][None].cuda(), crl[i][None].cuda(), s, start_steps=start, face_seeds=[700 + i], **kw)[0].cpu()
        r = rel_l2(out[i].cpu(), got)
        worst, exact = max(worst, r), exact + int(torch.equal(out[i].cpu(), got))
        if masks[i] is not None:
            keep = (masks[i] == 0)[None].expand(4, 16, 16)
            assert torch.equal(out[i].cpu()[keep], crl[i].float()[keep]), i
    print(f"ContinuousSampler with masks vs each request alone: {exact}/{N} bit-identical, worst rel-L2 {worst:.2e}")
    assert worst <= TRAJ_TOL, worst
    m.prepare(data[2].cuda(), data[1].cuda())                         # the batch of the module's other tests


# ------------------------------------------------------------------------------------------------ 7. lifetime
@pytest.mark.gpu
def test_mask_lifetime(run64, data):
    from hifidiff_amd import sampling
    x, crl, crf = data
    run64.mask(box(64, 16, 4, 12, 2, 14), crl, x)
    assert run64.opt("masked_faces") == 64
    run64.e.prepare_slots([3, 17, 40], crl[:3].cuda(), cr_face=crf[:3].cuda())     # clears the refilled slots only
    assert run64.opt("masked_faces") == 61
    run64.e.prepare(crl.cuda(), cr_face=crf.cuda())                   # hd_prepare clears every mask
    assert run64.opt("masked_faces") == 0
    # the Python calls on the same conditioning tensors: the cache hits, hd_prepare does not run, and the mask must still be gone
    s, _, _ = _tables("ddim", 10)
    xd, crfd, crld = x.cuda(), crf.cuda(), crl.cuda()
    never = sampling.sample(run64.m, xd, crfd, crld, s).cpu()
    masked = sampling.sample(run64.m, xd, crfd, crld, s, mask=box(64, 16, 4, 12, 2, 14), known=crl, known_noise=x).cpu()
    assert run64.opt("masked_faces") == 64 and not torch.equal(masked, never)
    assert run64.e.cond_key is not None                               # the next call hits the cache
    again = sampling.sample(run64.m, xd, crfd, crld, s).cpu()
    assert run64.opt("masked_faces") == 0
    assert torch.equal(again, never)
    # a loop split over calls with prepare=False keeps the mask
    one = sampling.sample(run64.m, xd, crfd, crld, s, mask=box(64, 16, 4, 12, 2, 14), known=crl, known_noise=x, start_steps=0).cpu()
    y = sampling.sample(run64.m, xd, crfd, crld, s, mask=box(64, 16, 4, 12, 2, 14), known=crl, known_noise=x, start_steps=0, n_iters=4)
    y = sampling.sample(run64.m, y, None, None, s, prepare=False, start_steps=4, n_iters=6).cpu()
    assert run64.opt("masked_faces") == 64 and torch.equal(y, one)
    run64.m.clear_mask()
    assert run64.opt("masked_faces") == 0


# ------------------------------------------------------------------------------------------------ 9. argument checks through the C-ABI
@pytest.mark.gpu
def test_argument_checks(gpu, weights16):
    from hifidiff_amd import synth
    m = make_model(weights16)
    e = m.engine
    x, crl, crf = synth.sample_inputs(2, 16)
    xd, crld = x.cuda().contiguous(), crl.cuda().contiguous()
    md = box(2, 16, 4, 12, 2, 14).cuda().contiguous()
    s = torch.cuda.current_stream().cuda_stream
    err = lambda: _L().hd_last_error(e.ctx)  # noqa: E731
    call = lambda n, slots, a, b, c: _L().hd_mask_faces(  # noqa: E731
        e.ctx, n, None if slots is None else ctypes.cast(slots.data_ptr(), ctypes.POINTER(ctypes.c_int32)), a, b, c, s)
    assert call(2, None, md.data_ptr(), crld.data_ptr(), xd.data_ptr()) == ERR_NOT_READY and err()
    run = Runner(m, crf, crl)
    sl = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    bad = [(2, sl(0, 0), True, True, True), (2, sl(0, 2), True, True, True), (1, sl(-1), True, True, True), (1, None, True, True, True),
           (3, sl(0, 1, 1), True, True, True), (0, sl(0), True, True, True),
           (2, None, True, False, True), (2, None, True, True, False), (2, None, False, True, True), (2, None, False, False, True)]
    _, ts, coef = _tables("ddim", 10)
    for n, slots, a, b, c in bad:
        rc = call(n, slots, md.data_ptr() if a else None, crld.data_ptr() if b else None, xd.data_ptr() if c else None)
        assert rc == ERR_INVALID and err(), (n, slots, a, b, c, rc)
        assert run.opt("masked_faces") == 0
        assert bool(torch.isfinite(run.full(x, ts, coef)).all())      # the context is still usable
    assert call(1, sl(1), md.data_ptr(), crld.data_ptr(), xd.data_ptr()) == 0
    torch.cuda.synchronize()
    assert run.opt("masked_faces") == 1
    out = run.full(x, ts, coef)
    keep = (md[0].cpu() == 0)[None].expand(4, 16, 16)
    assert torch.equal(out[1][keep], crl[0].float()[keep])            # slot 1 carries face 0 of the call's tensors
    assert call(1, sl(1), None, None, None) == 0 and run.opt("masked_faces") == 0
    free(m)


# ------------------------------------------------------------------------------------------------ 10. latent 32
@pytest.mark.gpu
def test_latent32(gpu):
    from hifidiff_amd import synth
    m = make_model(synth.refiner_state_dict(32), 32)
    x, crl, crf = synth.sample_inputs(2, 32)
    run = Runner(m, crf, crl)
    _L().hd_set_option(m.engine.ctx, b"xcd2", 0)
    _check_kept(run, x, crl, x, "ddim", 10, 4)
    _check_compose(run, x, crl, x, box(2, 32, 5, 27, 8, 30), "ddim", 10)
    free(m)
