"""Per-face schedule positions in the graph-replayed loop (hd_sample_rows / hd_sample_rows_multistep, sampling.sample(start_steps=...)).

Face f starts at its own row r_f of one shared table and is held once past the last row.  Faces never interact and the per-face form
reads the same FiLM values and coefficient rows as hd_sample does on the tail schedule[r_f:], so its latents are compared bit for bit:
with hd_sample (all r_f = 0), with hd_sample on schedule[r:] (staggered starts, no noise), and with one call of the same loop (a loop
split over calls).  The per-face form runs every persistent stage: the face-cluster stages of levels 0 / 1 and the K-split XCD-local
stages of levels 2 / 3 with per-face FiLM rows.  The autonomous-wave form of level 2 (hd_xcd2.hpp, hd_sample's default there) has no
per-face instantiation; it and the K-split form add in a different order, so the bit-for-bit comparisons run with "xcd2" off (hd_sample
then runs the K-split form at level 2 as well), and the default program is compared with hd_sample within TRAJ_TOL
(tests/test_program_variants.py's bound for forms that differ in summation order)."""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

from conftest import psnr, rel_l2, weights16  # noqa: F401  (weights16: session fixture)

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


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


def free(m):
    del m
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class Runner:
    """Direct C-ABI calls on a prepared context (the Python wrapper would prepare again)."""

    def __init__(self, m, crf=None, crl=None, B=None):
        self.m, self.e = m, m.engine
        if crl is not None:
            m.prepare(crf.cuda(), crl.cuda())
        else:
            self.e.ensure(torch.device("cuda", 0))
            self.e.prepare_unconditional(B)

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
        _lib.check(rc, self.e.ctx)
        torch.cuda.synchronize()
        _lib.check(_L().hd_check(self.e.ctx), self.e.ctx)

    def full(self, x, ts, coef, noise=None, seed=0):
        xd = x.cuda().float().contiguous().clone()
        nd = None if noise is None else noise.cuda().float().contiguous()
        sch = self._sch(ts, coef)
        fn = _L().hd_sample_multistep if coef.shape[1] == 8 else _L().hd_sample
        self._run(fn(self.e.ctx, xd.data_ptr(), ctypes.byref(sch), None if nd is None else nd.data_ptr(), seed,
                     torch.cuda.current_stream().cuda_stream))
        return xd.cpu()

    def rows_rc(self, x, ts, coef, rows, n_iters, resume=0, noise=None, seed=0):
        xd = x.cuda().float().contiguous().clone()
        nd = None if noise is None else noise.cuda().float().contiguous()
        sch = self._sch(ts, coef)
        r = torch.as_tensor(rows, dtype=torch.int32).contiguous()
        rp = ctypes.cast(r.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        s = torch.cuda.current_stream().cuda_stream
        if coef.shape[1] == 8:
            rc = _L().hd_sample_rows_multistep(self.e.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, resume,
                                               None if nd is None else nd.data_ptr(), seed, s)
        else:
            rc = _L().hd_sample_rows(self.e.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, None if nd is None else nd.data_ptr(), seed, s)
        return rc, xd

    def rows(self, *a, **k):
        rc, xd = self.rows_rc(*a, **k)
        self._run(rc)
        return xd.cpu()


def _tables(kind, n):
    from hifidiff_amd import schedulers
    s = {"ddim": lambda: schedulers.DDIMScheduler(clip_sample_range=3.0), "ddpm": lambda: schedulers.DDPMScheduler(clip_sample_range=3.0),
         "dpm": lambda: schedulers.DPMSolverMultistepScheduler()}[kind]()
    s.set_timesteps(n)
    ts, coef = s.coefficient_table()
    return s, ts, coef


@pytest.fixture(scope="module")
def data(gpu):
    from hifidiff_amd import synth
    x, crl, crf = synth.sample_inputs(64, 16)
    return x, crl, crf


TRAJ_TOL = 1e-2                                   # tests/test_program_variants.py: forms of the program that differ in summation order


@pytest.fixture(scope="module")
def run64(gpu, weights16, data):
    """Batch 64 with the K-split form of the XCD-local stages at level 2 in both forms (module docstring)."""
    x, crl, crf = data
    m = make_model(weights16)
    run = Runner(m, crf, crl)
    _L().hd_set_option(m.engine.ctx, b"xcd2", 0)
    yield run
    free(m)


GROUPS = (0, 7, 25, 49, 50)


def _staggered(B, groups=GROUPS):
    return [groups[f % len(groups)] for f in range(B)]


def _check_staggered(run, x, ts, coef, rows):
    """Every group of faces against hd_sample on schedule[r:] of the same batch (faces at r = n come back unchanged)."""
    n = ts.numel()
    got = run.rows(x, ts, coef, rows, n - min(rows))
    rows_t = torch.tensor(rows)
    for r in sorted(set(rows)):
        sel = rows_t == r
        want = x.float() if r == n else run.full(x, ts[r:], coef[r:])
        assert torch.equal(got[sel], want[sel]), (r, float((got[sel] - want[sel]).abs().max()))
    return got


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.gpu
def test_all_rows_zero_is_hd_sample(run64, data):
    x = data[0]
    _, ts, coef = _tables("ddim", 50)
    assert torch.equal(run64.rows(x, ts, coef, [0] * 64, 50), run64.full(x, ts, coef))
    _, ts, coef = _tables("ddpm", 20)
    noise = torch.randn((20, 64, 4, 16, 16), generator=torch.Generator().manual_seed(5))
    assert torch.equal(run64.rows(x, ts, coef, [0] * 64, 20, seed=123), run64.full(x, ts, coef, seed=123))
    assert torch.equal(run64.rows(x, ts, coef, [0] * 64, 20, noise=noise), run64.full(x, ts, coef, noise=noise))
    _, ts, coef = _tables("dpm", 20)
    assert torch.equal(run64.rows(x, ts, coef, [0] * 64, 20), run64.full(x, ts, coef))


@pytest.mark.gpu
def test_default_program_within_the_stage_tolerance(run64, data):
    """The default program: hd_sample runs level 2 in the autonomous-wave form, the per-face form in the K-split form; every stage runs."""
    x = data[0]
    _L().hd_set_option(run64.e.ctx, b"xcd2", 1)
    try:
        _, ts, coef = _tables("ddim", 50)
        got, want = run64.rows(x, ts, coef, [0] * 64, 50), run64.full(x, ts, coef)
        r = rel_l2(got, want)
        print(f"default program, DDIM-50, all rows 0: rel-L2 {r:.3e} from hd_sample, bit-identical {torch.equal(got, want)}")
        assert bool(torch.isfinite(got).all()) and r <= TRAJ_TOL, r
        opt = lambda k: _L().hd_get_option(run64.e.ctx, k.encode())  # noqa: E731
        assert opt("sample_stage_launches") == 8 and opt("sample_face_stage_launches") == 4
        assert opt("rows_stage_launches") == opt("sample_stage_launches")
    finally:
        _L().hd_set_option(run64.e.ctx, b"xcd2", 0)


# ------------------------------------------------------------------------------------------------ 2. staggered starts
@pytest.mark.gpu
def test_staggered_starts_against_the_tail_schedules(run64, data):
    _, ts, coef = _tables("ddim", 50)
    _check_staggered(run64, data[0], ts, coef, _staggered(64))


# ------------------------------------------------------------------------------------------------ 3. resume
@pytest.mark.gpu
def test_split_loops_reproduce_one_call(run64, data):
    x = data[0]
    _, ts, coef = _tables("ddpm", 50)
    one = run64.rows(x, ts, coef, [0] * 64, 50, seed=77)
    y = x
    for c in range(5):
        y = run64.rows(y, ts, coef, [10 * c] * 64, 10, seed=77)
    assert torch.equal(y, one)
    _, ts, coef = _tables("dpm", 20)
    one = run64.rows(x, ts, coef, [0] * 64, 20)
    assert torch.equal(one, run64.full(x, ts, coef))
    y, r0 = x, 0
    for c, k in enumerate((7, 7, 6)):
        y = run64.rows(y, ts, coef, [r0] * 64, k, resume=int(c > 0))
        r0 += k
    assert torch.equal(y, one)
    # without the history, a resumed call would start from the wrong x0: refused
    _, ts7, coef7 = _tables("ddim", 10)
    run64.full(x, ts7, coef7)                                        # a single-step call in between
    rc, _ = run64.rows_rc(x, ts, coef, [7] * 64, 7, resume=1)
    assert rc == -1


@pytest.mark.gpu
def test_resume_needs_history_of_this_batch(gpu, weights16):
    from hifidiff_amd import synth
    m = make_model(weights16)
    x, crl, crf = synth.sample_inputs(2, 16)
    run = Runner(m, crf, crl)
    _, ts, coef = _tables("dpm", 10)
    rc, _ = run.rows_rc(x, ts, coef, [0, 0], 3, resume=1)            # no earlier call
    assert rc == -1
    run.rows(x, ts, coef, [0, 0], 3)
    assert run.rows_rc(x, ts, coef, [3, 3], 3, resume=1)[0] == 0
    torch.cuda.synchronize()
    x3, crl3, crf3 = synth.sample_inputs(3, 16)
    Runner(m, crf3, crl3)                                            # hd_prepare of another batch
    rc, _ = run.rows_rc(x3, ts, coef, [3, 3, 3], 3, resume=1)
    assert rc == -1
    free(m)


def _first_order_tail(coef, r):
    """schedule[r:] whose row 0 is first-order (diffusers' img2img start of a multistep solver): x0 coefficient c3 + c7, no history."""
    t = coef[r:].clone()
    t[0, 3] = t[0, 3] + t[0, 7]
    t[0, 7] = 0.0
    return t


@pytest.mark.gpu
def test_staggered_multistep_starts_are_first_order(run64, data):
    x = data[0]
    _, ts, coef = _tables("dpm", 20)
    groups = (0, 5, 12, 19, 20)
    rows = _staggered(64, groups)
    assert (coef[1:19, 7] != 0).all()                                  # second-order rows: the first-row rule matters
    got = run64.rows(x, ts, coef, rows, 20)
    rows_t = torch.tensor(rows)
    for r in groups:
        sel = rows_t == r
        want = x.float() if r == 20 else run64.full(x, ts[r:], _first_order_tail(coef, r))
        assert torch.equal(got[sel], want[sel]), (r, float((got[sel] - want[sel]).abs().max()))


@pytest.mark.gpu
def test_held_faces_keep_their_history(run64, data):
    """Faces at rows 0 and 10 for 10 iterations, then a resumed call at rows 10 and 20: the first group finishes the one-call loop bit for
    bit; the second group is held in the resumed call -- its latents and its x0 history stay as the first call left them."""
    x = data[0]
    _, ts, coef = _tables("dpm", 20)
    one = run64.rows(x, ts, coef, [0] * 64, 20)
    rows = torch.tensor(_staggered(64, (0, 10)))
    y = run64.rows(x, ts, coef, rows, 10)
    held = rows == 10
    hist0 = np.zeros(x.numel(), np.float32)
    assert _L().hd_debug_read(run64.e.ctx, b"x0_hist", hist0.ctypes.data, hist0.size) == hist0.size
    z = run64.rows(y, ts, coef, rows + 10, 10, resume=1)
    hist1 = np.zeros(x.numel(), np.float32)
    assert _L().hd_debug_read(run64.e.ctx, b"x0_hist", hist1.ctypes.data, hist1.size) == hist1.size
    assert torch.equal(z[~held], one[~held])
    assert torch.equal(z[held], y[held])
    h0, h1 = hist0.reshape(x.shape), hist1.reshape(x.shape)
    assert np.array_equal(h1[held.numpy()], h0[held.numpy()]) and not np.array_equal(h1[~held.numpy()], h0[~held.numpy()])


@pytest.mark.gpu
def test_python_split_loop_with_resume(gpu, weights16):
    """sampling.sample split over calls: the conditioning of the same tensors is not prepared again, so the multistep history carries over."""
    from hifidiff_amd import sampling, synth
    m = make_model(weights16)
    x, crl, crf = [t.cuda() for t in synth.sample_inputs(2, 16)]
    s, _, _ = _tables("dpm", 20)
    one = sampling.sample(m, x, crf, crl, s, start_steps=0)        # (the default program: see test_default_program_within_the_stage_tolerance)
    y = sampling.sample(m, x, crf, crl, s, start_steps=0, n_iters=7)
    y = sampling.sample(m, y, crf, crl, s, start_steps=7, n_iters=7, resume=True)
    y = sampling.sample(m, y, crf, crl, s, start_steps=14, n_iters=6, resume=True)
    assert torch.equal(y, one)
    free(m)


# ------------------------------------------------------------------------------------------------ 4. the stages ran
@pytest.mark.gpu
def test_the_face_stages_run_in_the_per_face_program(run64, data):
    x = data[0]
    _, ts, coef = _tables("ddim", 10)
    _opt = lambda k: _L().hd_get_option(run64.e.ctx, k.encode())  # noqa: E731
    run64.full(x, ts, coef)
    run64.rows(x, ts, coef, _staggered(64, (0, 3, 9)), 10)
    # (a capture happens only when the graphs are stale: force one of each form on this context)
    _L().hd_set_option(run64.e.ctx, b"face", 1)
    run64.full(x, ts, coef)
    run64.rows(x, ts, coef, _staggered(64, (0, 3, 9)), 10)
    shared, shared_face, rows = _opt("sample_stage_launches"), _opt("sample_face_stage_launches"), _opt("rows_stage_launches")
    # levels 0 / 1: encoder and decoder stages of the face clusters; levels 2 / 3: the XCD-local stages -- all with per-face FiLM rows
    assert shared == 8 and shared_face == 4, (shared, shared_face)
    assert rows == shared, (rows, shared)


# ------------------------------------------------------------------------------------------------ 5. against the eager loop
def _eager_rows(model, x, crf, crl, sched, rows, n_iters):
    """model(latents, t_per_face, ...) + scheduler.step per face, face f at row r_f + i."""
    ts = sched.timesteps
    n = ts.numel()
    x = x.cuda().clone()
    for i in range(n_iters):
        k = [r + i for r in rows]
        t = torch.tensor([int(ts[min(kk, n - 1)]) for kk in k], device="cuda")
        eps = model(x, t, crf.cuda(), crl.cuda()).sample
        for f, kk in enumerate(k):
            if kk < n:
                x[f:f + 1] = sched.step(eps[f:f + 1], ts[kk], x[f:f + 1], eta=0.0).prev_sample
    return x.cpu()


@pytest.mark.gpu
def test_img2img_against_the_oracle_and_the_eager_loop(gpu, weights16):
    """B = 3 at rows {0, 20, 40}: the bf16-emulating oracle network driven face by face at the same rows with the oracle's DDIM step
    (test_multistep.py's oracle bound), and the eager loop of this library's model(...) + scheduler.step."""
    from hifidiff_amd import sampling, synth
    from oracle import hifidiff_oracle as O
    m = make_model(weights16)
    x, crl, crf = synth.sample_inputs(3, 16)
    sched, ts, coef = _tables("ddim", 50)
    lat, start = sampling.img2img_start(sched, crl, torch.tensor([1.0, 0.6, 0.2]), noise=x)
    assert start.tolist() == [0, 20, 40]
    got = sampling.sample(m, lat.cuda(), crf.cuda(), crl.cuda(), sched, start_steps=start, n_iters=3).cpu()
    osch = O.DDIMScheduler(clip_sample=True, clip_sample_range=3.0)
    osch.set_timesteps(50)
    cond = O.Conditioning(weights16, crl, crf, prec=O.BF16)
    xr = lat.clone().float()
    for i in range(3):
        t = torch.tensor([int(sched.timesteps[r + i]) for r in start.tolist()])
        eps = O.fused_denoiser(weights16, xr, t, prec=O.BF16, cond=cond)
        xr = torch.cat([osch.step(eps[f:f + 1], int(t[f]), xr[f:f + 1]).prev_sample for f in range(3)])
    assert rel_l2(got, xr) <= 2e-2, rel_l2(got, xr)
    want = _eager_rows(m, lat, crf, crl, sched, start.tolist(), 3)
    assert psnr(got, want) >= 50.0 and rel_l2(got, want) <= 1e-2, (psnr(got, want), rel_l2(got, want))
    full = sampling.sample(m, lat.cuda(), crf.cuda(), crl.cuda(), sched, start_steps=start).cpu()
    assert torch.isfinite(full).all()
    free(m)


# ------------------------------------------------------------------------------------------------ 6. other program forms
@pytest.mark.gpu
def test_face_stages_off(gpu, weights16, data):
    x, crl, crf = data
    m = make_model(weights16)
    run = Runner(m, crf, crl)
    _L().hd_set_option(m.engine.ctx, b"face", 0)
    _L().hd_set_option(m.engine.ctx, b"xcd", 0)                       # the per-GEMM form of every level
    _, ts, coef = _tables("ddim", 50)
    _check_staggered(run, x, ts, coef, _staggered(64))
    assert _L().hd_get_option(m.engine.ctx, b"rows_stage_launches") == 0
    free(m)


@pytest.mark.gpu
def test_two_chains(gpu, weights16, data):
    x, crl, crf = data
    saved = {k: os.environ.get(k) for k in ("HD_EXPERIMENTS", "HD_CHAINS")}
    os.environ.update({"HD_EXPERIMENTS": "1", "HD_CHAINS": "2"})
    try:
        m = make_model(weights16)
        run = Runner(m, crf, crl)
        assert _L().hd_num_chains(m.engine.ctx) == 2
        _, ts, coef = _tables("ddim", 50)
        _check_staggered(run, x, ts, coef, _staggered(64))
        _, ts, coef = _tables("dpm", 20)
        one = run.rows(x, ts, coef, [0] * 64, 20)
        assert torch.equal(one, run.full(x, ts, coef))
        y = run.rows(x, ts, coef, [0] * 64, 9)
        assert torch.equal(run.rows(y, ts, coef, [9] * 64, 11, resume=1), one)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    free(m)


@pytest.mark.gpu
def test_batch_65(gpu, weights16):
    from hifidiff_amd import synth
    x, crl, crf = synth.sample_inputs(65, 16)
    m = make_model(weights16)
    run = Runner(m, crf, crl)
    _, ts, coef = _tables("ddim", 20)
    _check_staggered(run, x, ts, coef, _staggered(65, (0, 3, 19, 20)))
    free(m)


@pytest.mark.gpu
def test_latent32(gpu):
    from hifidiff_amd import synth
    m = make_model(synth.refiner_state_dict(32), 32)
    x, crl, crf = synth.sample_inputs(2, 32)
    run = Runner(m, crf, crl)
    _, ts, coef = _tables("ddim", 10)
    _check_staggered(run, x, ts, coef, [0, 4])
    free(m)


@pytest.mark.gpu
def test_unconditional_denoiser(gpu, weights16):
    from hifidiff_amd import synth
    from hifidiff_amd.refiner import Denoiser
    m = Denoiser(16)
    k = len("denoiser.")
    m.load_state_dict({n[k:]: v for n, v in weights16.items() if n.startswith("denoiser.") and ".hcas." not in n and ".idc_conv" not in n})
    m.to("cuda:0")
    x = T(np.stack([synth.randn(f"x_T/{f}", (4, 16, 16)) for f in range(4)]))
    run = Runner(m, B=4)
    _L().hd_set_option(m.engine.ctx, b"xcd2", 0)
    _, ts, coef = _tables("ddim", 10)
    _check_staggered(run, x, ts, coef, [0, 2, 9, 10])
    free(m)


# ------------------------------------------------------------------------------------------------ 7. argument checks
@pytest.mark.gpu
def test_argument_checks(gpu, weights16):
    from hifidiff_amd import synth
    m = make_model(weights16)
    x, crl, crf = synth.sample_inputs(2, 16)
    run = Runner(m, crf, crl)
    _, ts, coef = _tables("ddim", 10)
    _, tsm, coefm = _tables("dpm", 10)
    for rows, k in (([-1, 0], 1), ([0, 11], 1), ([0, 0], 0), ([0, 0], 11), ([5, 10], 6), ([10, 10], 1)):
        assert run.rows_rc(x, ts, coef, rows, k)[0] == -1, (rows, k)
        assert run.rows_rc(x, tsm, coefm, rows, k)[0] == -1, (rows, k)
    assert run.rows_rc(x, ts, coef, [5, 10], 5)[0] == 0
    torch.cuda.synchronize()
    xd = x.cuda().contiguous()
    sch = run._sch(ts, coef)
    r = torch.zeros(2, dtype=torch.int32)
    rp = ctypes.cast(r.data_ptr(), ctypes.POINTER(ctypes.c_int32))
    s = torch.cuda.current_stream().cuda_stream
    assert _L().hd_sample_rows(m.engine.ctx, None, ctypes.byref(sch), rp, 1, None, 0, s) == -1
    assert _L().hd_sample_rows(m.engine.ctx, xd.data_ptr(), None, rp, 1, None, 0, s) == -1
    assert _L().hd_sample_rows(m.engine.ctx, xd.data_ptr(), ctypes.byref(sch), None, 1, None, 0, s) == -1
    schm = run._sch(tsm, coefm)
    assert _L().hd_sample_rows_multistep(m.engine.ctx, xd.data_ptr(), ctypes.byref(schm), rp, 1, 2, None, 0, s) == -1
    assert _L().hd_sample_rows_multistep(m.engine.ctx, xd.data_ptr(), ctypes.byref(schm), None, 1, 0, None, 0, s) == -1
    # the C-ABI cannot tell a 7-column table from an 8-column one; sampling.sample picks the entry point by the table's width and refuses
    # resume for a single-step schedule
    from hifidiff_amd import sampling
    with pytest.raises(ValueError):
        sampling.sample(m, x.cuda(), crf.cuda(), crl.cuda(), _tables("ddim", 10)[0], start_steps=0, resume=True)
    with pytest.raises(ValueError):
        sampling.sample(m, x.cuda(), crf.cuda(), crl.cuda(), _tables("ddim", 10)[0], start_steps=[0, 0, 0])
    free(m)
