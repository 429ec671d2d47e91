"""Per-request schedules on the GPU: hd_sample_spans (every face runs its own span [begin_f, end_f) of one concatenated coefficient table),
sampling.sample(scheduler=ScheduleSet, schedules=...) and sampling.ContinuousSampler over a ScheduleSet.

Faces never interact in the step program and the per-face graphs are one program whatever the entry point (tests/test_slots.py), so a
face of a mixed batch must come out bit for bit as the same face of a batch in which every face runs that member alone through the
existing entry points -- hd_sample_faces for a 7-column member, hd_sample_faces_multistep for an 8-column one -- with the same start row
and Philox key.  That covers the hold at the face's own end row, the FiLM staging past a short span, the noise counter that starts at the
span's begin row, and the c7 = 0 embedding of DDIM / DDPM rows in the 8-column table.  One check against the bf16-emulating oracle shows
that the mixed path computes the right thing and is not merely self-consistent."""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2, weights16  # noqa: F401  (weights16: session fixture)

TRAJ_TOL = 1e-2                                   # tests/test_slots.py: a request in a refilled batch against the same request alone
ORACLE_TOL = 2e-2                                 # tests/test_multistep.py / tests/test_start_rows.py: trajectories of <= 10 rows against the oracle
ERR_INVALID = -1
MIXED = (("ddim10", "ddim", 10), ("ddim25", "ddim", 25), ("sde8", "sde", 8), ("ddpm12", "ddpm", 12))


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


class _env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _sched(kind, n):
    from hifidiff_amd import schedulers
    s = {"ddim": lambda: schedulers.DDIMScheduler(clip_sample_range=3.0), "ddpm": lambda: schedulers.DDPMScheduler(clip_sample_range=3.0),
         "dpm": lambda: schedulers.DPMSolverMultistepScheduler(),
         "sde": lambda: schedulers.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")}[kind]()
    s.set_timesteps(n)
    return s


def _set(spec):
    from hifidiff_amd.sampling import ScheduleSet
    return ScheduleSet({k: _sched(kind, n) for k, kind, n in spec})


def _i32(v):
    t = torch.as_tensor(v, dtype=torch.int32).contiguous()
    return t, ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int32))


class Ctx:
    """Direct C-ABI calls on one model's context."""

    def __init__(self, m):
        self.m, self.e = m, m.engine
        self.e.ensure(torch.device("cuda", 0))

    @property
    def ctx(self):
        return self.e.ctx

    def prep(self, crf, crl):
        self.e.prepare(crl.cuda(), cr_face=crf.cuda())

    def opt(self, key):
        return _L().hd_get_option(self.ctx, key)

    def sch(self, ts, coef):
        from hifidiff_amd import _lib
        self._keep = (ts.float().contiguous(), coef.float().contiguous())
        ts, coef = self._keep
        s = _lib.ScheduleMS() if coef.shape[1] == 8 else _lib.Schedule()
        s.n_steps = ts.numel()
        s.timesteps = ctypes.cast(ts.data_ptr(), ctypes.POINTER(ctypes.c_float))
        s.coef = ctypes.cast(coef.data_ptr(), ctypes.POINTER(ctypes.c_float))
        return s

    @staticmethod
    def _seeds(seeds):
        sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        return sd, None if sd is None else sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))

    def faces_rc(self, x, tab, rows, n_iters, seeds=None, resume=None, seed=0):
        """hd_sample_faces (7 columns) / hd_sample_faces_multistep (8 columns)."""
        ts, coef = tab
        xd = x.cuda().float().contiguous().clone()
        _r, rp = _i32(rows)
        _sd, sp = self._seeds(seeds)
        s = torch.cuda.current_stream().cuda_stream
        sch = self.sch(ts, coef)
        if coef.shape[1] == 8:
            _rs, rsp = _i32([0] * len(rows) if resume is None else resume)
            rc = _L().hd_sample_faces_multistep(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, rsp, sp, None, seed, s)
        else:
            rc = _L().hd_sample_faces(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, sp, None, seed, s)
        return rc, xd

    def spans_rc(self, x, tab, begin, end, rows, n_iters, seeds=None, resume=None, seed=0, noise=None):
        """hd_sample_spans on an 8-column table."""
        ts, coef = tab
        assert coef.shape[1] == 8
        xd = x.cuda().float().contiguous().clone()
        _b, bp = _i32(begin)
        _e, ep = _i32(end)
        _r, rp = _i32(rows)
        _rs, rsp = _i32([0] * len(rows) if resume is None else resume)
        _sd, sp = self._seeds(seeds)
        nd = None if noise is None else noise.cuda().float().contiguous()
        sch = self.sch(ts, coef)
        rc = _L().hd_sample_spans(self.ctx, xd.data_ptr(), ctypes.byref(sch), bp, ep, rp, n_iters, rsp, sp,
                                  None if nd is None else nd.data_ptr(), seed, torch.cuda.current_stream().cuda_stream)
        return rc, xd

    def done(self, rc_xd):
        from hifidiff_amd import _lib
        rc, xd = rc_xd
        _lib.check(rc, self.ctx)
        torch.cuda.synchronize()
        _lib.check(_L().hd_check(self.ctx), self.ctx)
        return xd.cpu()

    def faces(self, *a, **k):
        return self.done(self.faces_rc(*a, **k))

    def spans(self, *a, **k):
        return self.done(self.spans_rc(*a, **k))


@pytest.fixture(scope="module")
def data(gpu):
    from hifidiff_amd import synth
    return synth.sample_inputs(64, 16)


@pytest.fixture(scope="module")
def c64(gpu, weights16, data):
    m = make_model(weights16)
    c = Ctx(m)
    c.prep(data[2], data[1])
    yield c
    free(m)


def _assignment(sset, B):
    """Round-robin members, and a start row inside the member's schedule for every face: 0 for most, later rows for some (a face of
    every member starts at its last row, one past it -- held for the whole call)."""
    keys = [sset.keys[f % len(sset.keys)] for f in range(B)]
    rel = []
    for f, k in enumerate(keys):
        b, e = sset.span(k)
        n = e - b
        rel.append((0, 0, 3, 0, n // 2, 0, n - 1, n)[(f // len(sset.keys)) % 8])
    return keys, rel


def _mixed_against_each_member_alone(c, x, sset, seeds):
    """The mixed hd_sample_spans call against one hd_sample_faces* call per member on the same prepared batch; returns the mixed result."""
    B = x.shape[0]
    keys, rel = _assignment(sset, B)
    tab = sset.coefficient_table()
    begin = [sset.span(k)[0] for k in keys]
    end = [sset.span(k)[1] for k in keys]
    start = [b + r for b, r in zip(begin, rel)]
    mixed = c.spans(x, tab, begin, end, start, max(e - s for e, s in zip(end, start)), seeds=seeds)
    assert bool(torch.isfinite(mixed).all())
    for k in sset.keys:
        mine = [f for f in range(B) if keys[f] == k]
        ts, coef = sset.member(k).coefficient_table()
        n = ts.numel()
        rows = [min(r, n) if keys[f] != k else r for f, r in enumerate(rel)]      # the other faces: any valid row of this member
        alone = c.faces(x, (ts, coef), rows, n - min(rows), seeds=seeds)
        for f in mine:
            assert torch.equal(mixed[f], alone[f]), (k, f, rel[f])
        moved = [f for f in mine if rel[f] < n]
        held = [f for f in mine if rel[f] == n]
        assert all(not torch.equal(mixed[f], x[f]) for f in moved) and all(torch.equal(mixed[f], x[f]) for f in held)
    return mixed, (keys, rel, begin, end, start)


# ------------------------------------------------------------------------------------------------ 1. whole-table spans
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dpm", "sde"])
@pytest.mark.parametrize("keyed", [True, False])
def test_whole_table_spans_are_hd_sample_faces_multistep(c64, data, kind, keyed):
    x = data[0]
    tab = _sched(kind, 10).coefficient_table()
    rows = (torch.arange(64) * 5 % 9).tolist()                        # staggered starts, first-order first rows
    seeds = (np.arange(64, dtype=np.uint64) * 7919 + 11) if keyed else None
    want = c64.faces(x, tab, rows, 10 - min(rows), seeds=seeds, seed=77)
    got = c64.spans(x, tab, [0] * 64, [10] * 64, rows, 10 - min(rows), seeds=seeds, seed=77)
    assert torch.equal(got, want)
    assert not torch.equal(got, x)


# ------------------------------------------------------------------------------------------------ 2. a mixed batch
@pytest.mark.gpu
def test_mixed_batch_equals_every_member_alone(c64, data):
    sset = _set(MIXED)
    assert [sset.span(k) for k in sset.keys] == [(0, 10), (10, 35), (35, 43), (43, 55)]
    seeds = np.arange(64, dtype=np.uint64) * 104729 + 3
    _mixed_against_each_member_alone(c64, data[0], sset, seeds)


@pytest.mark.gpu
def test_batch_keyed_noise_counts_rows_from_the_span(c64, data):
    """Without face_seeds the z of the batch keying is Philox(seed; k - begin_f, element of the batch): the DDPM member at rows [10, 22)
    of a table equals hd_sample_faces(seed) on the member's own table."""
    x = data[0]
    sset = _set((("ddim10", "ddim", 10), ("ddpm12", "ddpm", 12)))
    tab = sset.coefficient_table()
    got = c64.spans(x, tab, [10] * 64, [22] * 64, [10] * 64, 12, seed=99)
    want = c64.faces(x, sset.member("ddpm12").coefficient_table(), [0] * 64, 12, seed=99)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ 3. a mixed loop split over calls
@pytest.mark.gpu
def test_mixed_loop_split_over_calls_reproduces_one_call(c64, data):
    x = data[0]
    sset = _set(MIXED)
    tab = sset.coefficient_table()
    seeds = np.arange(64, dtype=np.uint64) * 104729 + 3
    keys, rel = _assignment(sset, 64)
    begin = [sset.span(k)[0] for k in keys]
    end = [sset.span(k)[1] for k in keys]
    start = [b + r for b, r in zip(begin, rel)]
    one = c64.spans(x, tab, begin, end, start, max(e - s for e, s in zip(end, start)), seeds=seeds)
    c64.prep(data[2], data[1])                                         # no history left over from the one-call loop
    y, row, ran, calls = x, list(start), [0] * 64, 0
    while any(r < e for r, e in zip(row, end)):
        n = min(3, max(e - r for r, e in zip(row, end)))
        y = c64.spans(y, tab, begin, end, row, n, seeds=seeds, resume=ran)
        ran = [int(a or r < e) for a, r, e in zip(ran, row, end)]     # a face that ran a row has a history of its own
        row = [min(r + n, e) for r, e in zip(row, end)]
        calls += 1
    assert calls == 9                                                  # 25 rows in calls of 3
    assert torch.equal(y, one)


# ------------------------------------------------------------------------------------------------ 4. masks
@pytest.mark.gpu
def test_masked_face_on_a_short_schedule_ends_on_known(c64, data):
    from hifidiff_amd import sampling
    x, crl, crf = data
    sset = _set((("short", "ddim", 10), ("long", "ddim", 25)))        # the short span ends inside the table: row 10 exists
    keys = ["short" if f % 2 == 0 else "long" for f in range(64)]
    mask = torch.zeros((64, 16, 16))
    mask[:, 4:12, 3:13] = 1.0
    xd, crfd, crld = x.cuda(), crf.cuda(), crl.cuda()
    got = sampling.sample(c64.m, xd, crfd, crld, sset, schedules=keys, mask=mask, known=crl, known_noise=x).cpu()
    keep = (mask == 0)[:, None].expand(-1, 4, -1, -1)
    assert torch.equal(got[keep], crl[keep])                          # every face ends exactly on `known`, at its own last row
    assert not torch.equal(got[~keep], crl[~keep])
    for key in ("short", "long"):
        alone = sampling.sample(c64.m, xd, crfd, crld, sset.member(key), start_steps=0, mask=mask, known=crl, known_noise=x).cpu()
        mine = [f for f in range(64) if keys[f] == key]
        assert torch.equal(got[mine], alone[mine]), key
    plain = sampling.sample(c64.m, xd, crfd, crld, sset, schedules=keys).cpu()      # prepare=True without a mask clears it
    assert not torch.equal(plain[keep], crl[keep])
    c64.prep(crf, crl)


# ------------------------------------------------------------------------------------------------ 5. graphs
@pytest.mark.gpu
def test_alternating_faces_and_spans_calls_capture_nothing(c64, data):
    x = data[0]
    sset = _set(MIXED)
    tab = sset.coefficient_table()
    keys, rel = _assignment(sset, 64)
    begin = [sset.span(k)[0] for k in keys]
    end = [sset.span(k)[1] for k in keys]
    start = [b + r for b, r in zip(begin, rel)]
    c64.faces(x, tab, [0] * 64, 2)                                     # the per-face graphs exist, and the table's FiLM rows
    before = (c64.opt(b"graph_captures"), c64.opt(b"rows_stage_launches"))
    assert before[0] > 0
    for _ in range(2):
        c64.spans(x, tab, begin, end, start, 2)
        c64.faces(x, tab, [0] * 64, 2)
    assert (c64.opt(b"graph_captures"), c64.opt(b"rows_stage_launches")) == before


# ------------------------------------------------------------------------------------------------ 6. other program forms
SHORT = (("ddim6", "ddim", 6), ("sde4", "sde", 4), ("ddpm5", "ddpm", 5))


@pytest.mark.gpu
def test_variant_two_chains(weights16, data):
    with _env({"HD_EXPERIMENTS": "1", "HD_CHAINS": "2"}):
        m = make_model(weights16)
        c = Ctx(m)
        c.prep(data[2], data[1])
        assert _L().hd_num_chains(c.ctx) == 2
        _mixed_against_each_member_alone(c, data[0], _set(SHORT), np.arange(64, dtype=np.uint64) + 17)
        free(m)


@pytest.mark.gpu
def test_variant_latent32(weights16, gpu):
    from hifidiff_amd import synth
    m = make_model(synth.refiner_state_dict(32, reuse=(weights16, 16)), 32)
    x, crl, crf = synth.sample_inputs(8, 32)
    c = Ctx(m)
    c.prep(crf, crl)
    _mixed_against_each_member_alone(c, x, _set(SHORT), np.arange(8, dtype=np.uint64) + 17)
    free(m)


@pytest.mark.gpu
def test_variant_unconditional_denoiser(weights16, gpu):
    from hifidiff_amd import sampling
    u = make_denoiser(weights16)
    c = Ctx(u)
    c.e.prepare_unconditional(8)
    x = torch.randn((8, 4, 16, 16), generator=torch.Generator().manual_seed(5))
    sset = _set(SHORT)
    seeds = np.arange(8, dtype=np.uint64) + 17
    mixed, (keys, rel, _, _, _) = _mixed_against_each_member_alone(c, x, sset, seeds)
    got = sampling.sample(u, x.cuda(), None, None, sset, schedules=keys, start_steps=torch.tensor(rel), face_seeds=seeds.tolist()).cpu()
    assert torch.equal(got, mixed)                                    # the Python entry: start rows relative to the face's schedule
    free(u)


# ------------------------------------------------------------------------------------------------ 7. the serving loop
@pytest.mark.gpu
def test_continuous_sampler_over_a_set_matches_each_request_alone(c64, data):
    from hifidiff_amd import sampling, synth
    sset = _set(((10, "ddim", 10), (20, "dpm", 20), (40, "ddim", 40)))
    N = 80
    _, crl, crf = synth.sample_inputs(N, 16, seed=903)
    strength = (0.2 + 0.8 * torch.rand(N, generator=torch.Generator().manual_seed(903))).tolist()
    steps = [(10, 20, 40)[i % 3] for i in range(N)]
    box = torch.zeros((16, 16))
    box[3:11, 5:14] = 1.0
    masks = [box if i % 5 == 2 else None for i in range(N)]           # 16 masked requests, on all three members
    cs = sampling.ContinuousSampler(c64.m, sset, batch=64, refill_every=3)
    ids = [cs.submit(crf[i], crl[i], seed=500 + i, strength=strength[i], mask=masks[i], schedule=steps[i]) for i in range(N)]
    out = cs.drain()
    assert sorted(out) == ids and cs.refilled >= N - 64
    worst, exact = 0.0, 0
    rep = lambda t: t[None].expand(64, *t.shape).contiguous()          # noqa: E731  (the request in every slot; slot 0 is compared)
    for i in ids:
        masked = masks[i] is not None
        lat, start = cs._start(crl[i], 500 + i, strength[i], masked, steps[i])
        kw = dict(mask=rep(masks[i]), known=rep(crl[i]), known_noise=rep(cs._z(500 + i)[0])) if masked else {}
        got = sampling.sample(c64.m, rep(lat).cuda(), rep(crf[i]).cuda(), rep(crl[i]).cuda(), sset.member(steps[i]), start_steps=start,
                              face_seeds=[500 + i] * 64, **kw)[0].cpu()
        r = rel_l2(out[i].cpu(), got)
        worst, exact = max(worst, r), exact + int(torch.equal(out[i].cpu(), got))
        if masked:
            keep = (masks[i] == 0)[None].expand(4, -1, -1)
            assert torch.equal(out[i].cpu()[keep], crl[i][keep]), i   # the kept region ends exactly on the request's known latent
    print(f"ContinuousSampler over a set vs each request alone: {exact}/{N} bit-identical, worst rel-L2 {worst:.2e}")
    assert worst <= TRAJ_TOL, worst
    c64.prep(data[2], data[1])


# ------------------------------------------------------------------------------------------------ 8. bad arguments
@pytest.mark.gpu
def test_argument_checks(c64, data):
    x, crl, crf = data
    c64.prep(crf, crl)                                                 # no face has a history
    sset = _set((("ddim10", "ddim", 10), ("dpm8", "dpm", 8)))
    tab = sset.coefficient_table()
    B = 64
    b, e, r = [0] * B, [10] * B, [0] * B
    err = lambda: _L().hd_last_error(c64.ctx).decode()                 # noqa: E731

    def one(lst, f, v):
        lst = list(lst)
        lst[f] = v
        return lst

    assert c64.spans_rc(x, tab, one(b, 5, 1), e, r, 2)[0] == ERR_INVALID and "face 5" in err()          # begin > start
    assert c64.spans_rc(x, tab, b, one(e, 7, 19), r, 2)[0] == ERR_INVALID and "face 7" in err()         # end > n
    assert c64.spans_rc(x, tab, b, e, one(r, 9, 11), 2)[0] == ERR_INVALID and "face 9" in err()         # start > end
    assert c64.spans_rc(x, tab, one(b, 3, -1), e, r, 2)[0] == ERR_INVALID and "face 3" in err()
    assert c64.spans_rc(x, tab, one(b, 4, 11), one(e, 4, 18), one(r, 4, 11), 2)[0] == ERR_INVALID and "face 4" in err()   # c7 != 0 at a begin row
    assert float(tab[1][11, 7]) != 0.0 and float(tab[1][10, 7]) == 0.0
    assert c64.spans_rc(x, tab, b, e, r, 2, resume=one([0] * B, 6, 1))[0] == ERR_INVALID and "6" in err()   # resume at start == begin
    assert c64.spans_rc(x, tab, b, e, one(r, 6, 2), 2, resume=one([0] * B, 6, 1))[0] == ERR_INVALID and "6" in err()   # resume without a history
    assert c64.spans_rc(x, tab, b, e, r, 2, resume=one([0] * B, 6, 2))[0] == ERR_INVALID
    assert c64.spans_rc(x, tab, b, e, r, 0)[0] == ERR_INVALID and c64.spans_rc(x, tab, b, e, r, 11)[0] == ERR_INVALID   # n_iters
    assert c64.spans_rc(x, tab, b, e, [10] * B, 1)[0] == ERR_INVALID                                    # every face held: nothing to run
    sch = c64.sch(*tab)
    z, zp = _i32([0] * B)
    s = torch.cuda.current_stream().cuda_stream
    xd = x.cuda()
    assert _L().hd_sample_spans(c64.ctx, xd.data_ptr(), ctypes.byref(sch), None, zp, zp, 1, zp, None, None, 0, s) == ERR_INVALID
    assert _L().hd_sample_spans(c64.ctx, xd.data_ptr(), ctypes.byref(sch), zp, None, zp, 1, zp, None, None, 0, s) == ERR_INVALID
    assert _L().hd_sample_spans(c64.ctx, xd.data_ptr(), ctypes.byref(sch), zp, zp, zp, 1, None, None, None, 0, s) == ERR_INVALID
    assert _L().hd_check(c64.ctx) == 0
    # the context is usable: the valid call, and a resumed one after it (face 6 has run rows now)
    y = c64.spans(x, tab, b, e, r, 2)
    full = c64.spans(y, tab, b, e, [2] * B, 8, resume=[1] * B)
    assert torch.equal(full, c64.faces(x, sset.member("ddim10").coefficient_table(), [0] * B, 10))


# ------------------------------------------------------------------------------------------------ 9. against the oracle
def _update64(x, eps, c, h):
    """The hd_schedule_ms update in float64 (c: one coefficient row; no noise term: DDIM and DPM-Solver++ 2M rows have c6 == 0)."""
    c = [float(v) for v in c]
    assert c[6] == 0.0
    x0 = (x - c[0] * eps) / c[1]
    if np.isfinite(c[2]):
        x0 = x0.clamp(-c[2], c[2])
    r = c[3] * x0 + c[4] * x + c[5] * eps
    if c[7] != 0.0:
        r = r + c[7] * h
    return r, x0


@pytest.mark.gpu
def test_mixed_batch_against_the_oracle(gpu, weights16):
    """4 faces, DDIM-10 and DPM-Solver++ 2M-8 alternating: the bf16-emulating oracle network evaluated at every face's own timestep, and
    every face's own coefficient rows applied in float64 (the bound and the trajectory lengths of tests/test_multistep.py)."""
    from hifidiff_amd import sampling, synth
    from oracle import hifidiff_oracle as O
    m = make_model(weights16)
    x, crl, crf = synth.sample_inputs(4, 16)
    sset = _set((("ddim10", "ddim", 10), ("dpm8", "dpm", 8)))
    keys = ["ddim10", "dpm8", "ddim10", "dpm8"]
    ts, coef = sset.coefficient_table()
    span = [sset.span(k) for k in keys]
    got = sampling.sample(m, x.cuda(), crf.cuda(), crl.cuda(), sset, schedules=keys).cpu()
    cond = O.Conditioning(weights16, crl, crf, prec=O.BF16)
    xr, h = x.double(), [None] * 4
    for i in range(10):
        k = [min(b + i, e - 1) for b, e in span]                      # a held face is evaluated and its eps discarded
        eps = O.fused_denoiser(weights16, xr.float(), torch.tensor([int(ts[j]) for j in k]), prec=O.BF16, cond=cond).double()
        for f, (b, e) in enumerate(span):
            if b + i < e:
                xr[f], h[f] = _update64(xr[f], eps[f], coef[b + i], h[f])
    per_face = [rel_l2(got[f], xr[f]) for f in range(4)]
    print("mixed batch vs oracle, rel-L2 per face:", [f"{v:.2e}" for v in per_face], f"batch {rel_l2(got, xr):.2e}")
    assert rel_l2(got, xr) <= ORACLE_TOL and max(per_face) <= ORACLE_TOL, per_face
    free(m)
