"""Continuous batching on the GPU: hd_prepare_slots (refill the conditioning of some slots of a prepared batch) and hd_sample_faces* (per-face
Philox keys and per-face multistep resumption), and sampling.ContinuousSampler on top of them.

Faces never interact in the step program, so a refill must leave every other slot's latents bit for bit as they were, and a face's result
must not depend on its slot when it carries its own Philox key.  The per-face program runs the K-split form of the level-2 XCD-local stage
whatever "xcd2" says (tests/test_start_rows.py), so the per-face comparisons below are bit for bit in the default program as well.  The
refilled conditioning is computed at batch n on the workspace's staging chain: bit for bit what hd_prepare(n) computes; against
hd_prepare of the composed batch at 64 the priors and gates are bit for bit too, and the ResNet-50 embedding and idc term are within
3e-3 rel-L2 (COND_TOL: the ResNet's GEMMs pick their launch form by row count)."""
import ctypes
import gc
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2, weights16  # noqa: F401  (weights16: session fixture)

TRAJ_TOL = 1e-2                                   # tests/test_program_variants.py: forms of the program that differ in summation order
EPS_TOL = 6e-3                                    # tests/test_program_variants.py: eps against the bf16-emulating oracle
# refilled conditioning (computed at batch n) against hd_prepare of the composed batch (batch 64): the FPG priors and the HCA gates come
# out bit for bit; the ResNet-50 embedding and the idc term differ, because its GEMMs pick their launch form by row count (measured on an
# MI355X, n = 3: id_emb 7.2e-4, idc 1.86e-3 rel-L2)
COND_TOL = {"id_emb": 3e-3, "idc": 3e-3}
COND_TOL_OTHER = 1e-3
ERR_INVALID, ERR_NOT_READY = -1, -4
REFILL = [3, 17, 40]
BUFS = [f"prior{i}" for i in range(5)] + [f"wc{i}" for i in range(5)] + [f"ws{i}" for i in range(5)] + ["idc", "id_emb"]


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


def _tables(kind, n):
    from hifidiff_amd import schedulers
    s = {"ddim": lambda: schedulers.DDIMScheduler(clip_sample_range=3.0), "ddpm": lambda: schedulers.DDPMScheduler(clip_sample_range=3.0),
         "dpm": lambda: schedulers.DPMSolverMultistepScheduler(),
         "sde": lambda: schedulers.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")}[kind]()
    s.set_timesteps(n)
    ts, coef = s.coefficient_table()
    return s, ts.float().contiguous(), coef.float().contiguous()


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

    def refill(self, slots, crf, crl):
        self.e.prepare_slots(slots, crl.cuda(), cr_face=crf.cuda())

    def opt(self, key):
        return _L().hd_get_option(self.ctx, key)

    def read(self, name, B):
        n = _L().hd_debug_read(self.ctx, name.encode(), None, 0)
        buf = np.empty(n, dtype=np.float32)
        _L().hd_debug_read(self.ctx, name.encode(), buf.ctypes.data, n)
        return buf.reshape(B, -1)

    def sch(self, ts, coef):
        from hifidiff_amd import _lib
        self._keep = (ts, coef)
        s = _lib.ScheduleMS() if coef.shape[1] == 8 else _lib.Schedule()
        s.n_steps = ts.numel()
        s.timesteps = ctypes.cast(ts.data_ptr(), ctypes.POINTER(ctypes.c_float))
        s.coef = ctypes.cast(coef.data_ptr(), ctypes.POINTER(ctypes.c_float))
        return s

    def faces_rc(self, x, tab, rows, n_iters, seeds=None, resume=None, seed=0, noise=None):
        """hd_sample_faces* (seeds: per-face keys or None; resume: per-face 0/1, multistep only)."""
        _, ts, coef = tab
        xd = x.cuda().float().contiguous().clone()
        r = torch.as_tensor(rows, dtype=torch.int32).contiguous()
        rp = ctypes.cast(r.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        sp = None if sd is None else sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        nd = None if noise is None else noise.cuda().float().contiguous()
        s = torch.cuda.current_stream().cuda_stream
        sch = self.sch(ts, coef)
        if coef.shape[1] == 8:
            rs = torch.as_tensor(resume, dtype=torch.int32).contiguous()
            rc = _L().hd_sample_faces_multistep(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters,
                                                ctypes.cast(rs.data_ptr(), ctypes.POINTER(ctypes.c_int32)), sp,
                                                None if nd is None else nd.data_ptr(), seed, s)
        else:
            rc = _L().hd_sample_faces(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, sp, None if nd is None else nd.data_ptr(), seed, s)
        return rc, xd

    def rows_rc(self, x, tab, rows, n_iters, resume=0, seed=0):
        """hd_sample_rows* (batch keying)."""
        _, ts, coef = tab
        xd = x.cuda().float().contiguous().clone()
        r = torch.as_tensor(rows, dtype=torch.int32).contiguous()
        rp = ctypes.cast(r.data_ptr(), ctypes.POINTER(ctypes.c_int32))
        s = torch.cuda.current_stream().cuda_stream
        sch = self.sch(ts, coef)
        if coef.shape[1] == 8:
            rc = _L().hd_sample_rows_multistep(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, resume, None, seed, s)
        else:
            rc = _L().hd_sample_rows(self.ctx, xd.data_ptr(), ctypes.byref(sch), rp, n_iters, None, seed, s)
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

    def rows(self, *a, **k):
        return self.done(self.rows_rc(*a, **k))


@pytest.fixture(scope="module")
def data(gpu):
    from hifidiff_amd import synth
    A = synth.sample_inputs(64, 16)
    C = synth.sample_inputs(3, 16, seed=901)
    Y = synth.sample_inputs(64, 16, seed=902)
    return {"A": A, "C": C, "Y": Y}


@pytest.fixture(scope="module")
def c64(gpu, weights16):
    m = make_model(weights16)
    yield Ctx(m)
    free(m)


def _isolation(c, A, C, slots, tab, n1=10, n2=8):
    """Run n1 rows of batch A, refill `slots` with faces C, run n2 more rows; the same without the refill.  Returns the two results and
    the capture counters around the refill."""
    x, crl, crf = A
    xc, crlc, crfc = C
    B = x.shape[0]
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 5
    c.prep(crf, crl)
    x1 = c.faces(x, tab, [0] * B, n1, seeds=seeds)
    plain = c.faces(x1, tab, [n1] * B, n2, seeds=seeds)
    c.prep(crf, crl)
    x1b = c.faces(x, tab, [0] * B, n1, seeds=seeds)
    assert torch.equal(x1b, x1)                                       # the loop is deterministic
    before = (c.opt(b"graph_captures"), c.opt(b"rows_stage_launches"))
    c.refill(slots, crfc, crlc)
    x1b[slots] = xc
    rows = [n1] * B
    for s in slots:
        rows[s] = 0
    refilled = c.faces(x1b, tab, rows, n2, seeds=seeds)
    after = (c.opt(b"graph_captures"), c.opt(b"rows_stage_launches"))
    return plain, refilled, before, after


@pytest.mark.gpu
@pytest.mark.parametrize("xcd2", [1, 0])
def test_refill_leaves_other_slots_bit_identical_and_recaptures_nothing(c64, data, xcd2):
    _L().hd_set_option(c64.ctx, b"xcd2", xcd2)
    try:
        plain, refilled, before, after = _isolation(c64, data["A"], data["C"], REFILL, _tables("ddpm", 20))
    finally:
        _L().hd_set_option(c64.ctx, b"xcd2", 1)
    keep = [f for f in range(64) if f not in REFILL]
    assert torch.equal(refilled[keep], plain[keep])
    assert bool(torch.isfinite(refilled).all()) and not torch.equal(refilled[REFILL], plain[REFILL])
    assert after == before, (before, after)                           # no graph instantiated, the same stage launches
    assert before[1] > 0                                              # the persistent stages still run in the per-face program


@pytest.mark.gpu
def test_refilled_conditioning_equals_prepare_of_the_n_faces(c64, data):
    x, crl, crf = data["A"]
    _, crlc, crfc = data["C"]
    c64.prep(crfc, crlc)                                             # hd_prepare of the 3 faces as a batch of 3
    b3 = {k: c64.read(k, 3) for k in BUFS}
    c64.prep(crf, crl)
    old = {k: c64.read(k, 64) for k in BUFS}
    c64.refill(REFILL, crfc, crlc)
    torch.cuda.synchronize()
    new = {k: c64.read(k, 64) for k in BUFS}
    keep = [f for f in range(64) if f not in REFILL]
    for k in BUFS:
        assert np.array_equal(new[k][REFILL], b3[k]), k
        assert np.array_equal(new[k][keep], old[k][keep]), k
    comp_f, comp_l = crf.clone(), crl.clone()
    comp_f[REFILL], comp_l[REFILL] = crfc, crlc
    c64.prep(comp_f, comp_l)                                         # the composed batch at 64
    worst = {k: rel_l2(new[k][REFILL], c64.read(k, 64)[REFILL]) for k in BUFS}
    print("refilled conditioning vs hd_prepare of the composed batch, rel-L2 per buffer:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v <= COND_TOL.get(k, COND_TOL_OTHER) for k, v in worst.items()), worst


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ddpm", "sde"])
def test_face_seed_makes_a_face_independent_of_its_slot(c64, data, kind):
    x, crl, crf = data["A"]
    xy, crly, crfy = data["Y"]
    xc, crlc, crfc = data["C"]
    tab = _tables(kind, 12 if kind == "ddpm" else 10)
    n = tab[1].numel()
    ms = kind == "sde"
    runs = []
    for base, slot in (((x, crl, crf), 5), ((xy, crly, crfy), 40)):
        bx, bl, bf = [t.clone() for t in base]
        bx[slot], bl[slot], bf[slot] = xc[0], crlc[0], crfc[0]
        seeds = np.arange(64, dtype=np.uint64) + (1000 if slot == 5 else 2000)
        seeds[slot] = 0xDEADBEEF12345
        c64.prep(bf, bl)
        out = c64.faces(bx, tab, [0] * 64, n, seeds=seeds, resume=[0] * 64 if ms else None, seed=slot)
        runs.append(out[slot])
    assert torch.equal(runs[0], runs[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ddpm", "sde"])
def test_face_seeds_reproduce_the_batch_keyed_entries(c64, data, kind):
    x, crl, crf = data["A"]
    tab = _tables(kind, 12 if kind == "ddpm" else 10)
    n = tab[1].numel()
    ms = kind == "sde"
    c64.prep(crf, crl)
    s = 0x5EED_0F_FACE
    want = c64.rows(x, tab, [0] * 64, n, seed=s)
    got = c64.faces(x, tab, [0] * 64, n, seeds=[s] * 64, resume=[0] * 64 if ms else None, seed=123)
    assert torch.equal(got[0], want[0])                               # slot 0: element index in the face == in the batch
    assert not torch.equal(got[1], want[1])
    rows = (torch.arange(64) * 5 % (n - 1)).tolist()                  # staggered starts, batch keying
    want = c64.rows(x, tab, rows, n - min(rows), seed=77)
    got = c64.faces(x, tab, rows, n - min(rows), seeds=None, resume=[0] * 64 if ms else None, seed=77)
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_per_face_resume_after_a_mid_loop_refill(c64, data):
    x, crl, crf = data["A"]
    xc, crlc, crfc = data["C"]
    tab = _tables("dpm", 10)
    slot, r7 = 7, 2
    c64.prep(crf, crl)
    one_call = c64.faces(x, tab, [0] * 64, 10, resume=[0] * 64)
    c64.prep(crf, crl)
    x4 = c64.faces(x, tab, [0] * 64, 4, resume=[0] * 64)
    c64.refill([slot], crfc[:1], crlc[:1])
    x4[slot] = xc[0]
    rows = [4] * 64
    rows[slot] = r7
    resume = [1] * 64
    rc, _ = c64.faces_rc(x4, tab, rows, 6, resume=resume)             # the refilled face has no history
    assert rc == ERR_INVALID
    rc, _ = c64.rows_rc(x4, tab, rows, 6, resume=1)                   # nor has the batch as a whole
    assert rc == ERR_INVALID
    resume[slot] = 0
    x10 = c64.faces(x4, tab, rows, 6, resume=resume)
    rows = [10] * 64
    rows[slot] = r7 + 6
    final = c64.faces(x10, tab, rows, 2, resume=[1] * 64)
    keep = [f for f in range(64) if f != slot]
    assert torch.equal(final[keep], one_call[keep])
    # the refilled face against its own run started first-order at its row (conditioning through the same refill)
    c64.prep(crf, crl)
    c64.refill([slot], crfc[:1], crlc[:1])
    xs = x.clone()
    xs[slot] = xc[0]
    rows = [10] * 64
    rows[slot] = r7
    alone = c64.faces(xs, tab, rows, 10 - r7, resume=[0] * 64)
    assert torch.equal(final[slot], alone[slot])


@pytest.mark.gpu
def test_refilled_batch_eps_against_oracle(c64, weights16, data):
    from oracle import hifidiff_oracle as O
    x, crl, crf = data["A"]
    xc, crlc, crfc = data["C"]
    c64.prep(crf, crl)
    c64.refill(REFILL, crfc, crlc)
    eps = c64.e.eps(x.cuda(), 500).cpu()
    fl, ff = crl.clone(), crf.clone()
    fl[REFILL], ff[REFILL] = crlc, crfc
    faces = REFILL + [0, 63]
    cond = O.Conditioning(weights16, fl[faces], ff[faces], prec=O.BF16)
    ref = O.fused_denoiser(weights16, x[faces], 500, cond=cond, prec=O.BF16)
    r = rel_l2(eps[faces], ref)
    print(f"refilled batch eps vs oracle (faces {faces}): rel-L2 {r:.3e}")
    assert r <= EPS_TOL, r


def _stream_requests(n, L=16, seed=903):
    from hifidiff_amd import synth
    _, crl, crf = synth.sample_inputs(n, L, seed=seed)
    g = torch.Generator().manual_seed(seed)
    strength = (0.2 + 0.8 * torch.rand(n, generator=g)).tolist()
    return crf, crl, strength


@pytest.mark.gpu
def test_continuous_sampler_matches_each_request_alone(c64, data):
    from hifidiff_amd import sampling
    s, _, _ = _tables("ddim", 10)
    N = 80
    crf, crl, strength = _stream_requests(N)
    cs = sampling.ContinuousSampler(c64.m, s, batch=64, refill_every=3)
    ids = [cs.submit(crf[i], crl[i], seed=500 + i, strength=strength[i]) for i in range(N)]
    out = cs.drain()
    assert sorted(out) == ids and cs.refilled >= N - 64
    worst, exact = 0.0, 0
    for i in ids:
        lat, start = cs._start(crl[i], 500 + i, strength[i])
        rep = lambda t: t[None].expand(64, *t.shape).contiguous()      # noqa: E731  (the request in every slot; slot 0 is compared)
        got = sampling.sample(c64.m, rep(lat).cuda(), rep(crf[i]).cuda(), rep(crl[i]).cuda(), s, start_steps=start,
                              face_seeds=[500 + i] * 64)[0].cpu()
        r = rel_l2(out[i].cpu(), got)
        worst, exact = max(worst, r), exact + int(torch.equal(out[i].cpu(), got))
    print(f"ContinuousSampler vs each request alone: {exact}/{N} bit-identical, worst rel-L2 {worst:.2e}")
    assert worst <= TRAJ_TOL, worst


def _refill_check(c, A, C, slots, tab):
    """Isolation and the refilled conditioning (chain 0's slots) on one context: the short refill loop of the variants."""
    B = A[0].shape[0]
    plain, refilled, before, after = _isolation(c, A, C, slots, tab, n1=4, n2=4)
    keep = [f for f in range(B) if f not in slots]
    assert torch.equal(refilled[keep], plain[keep]) and bool(torch.isfinite(refilled).all())
    assert after == before
    n0 = B // max(1, _L().hd_num_chains(c.ctx))                       # the debug buffers are chain 0's
    s0 = [j for j, s in enumerate(slots) if s < n0]
    got = {k: c.read(k, n0) for k in BUFS}
    c.prep(C[2], C[1])
    for k in BUFS:
        want = c.read(k, C[0].shape[0])
        assert np.array_equal(got[k][[slots[j] for j in s0]], want[s0]), k


@pytest.mark.gpu
def test_variant_two_chains(weights16, data):
    with _env({"HD_EXPERIMENTS": "1", "HD_CHAINS": "2"}):
        m = make_model(weights16)
        c = Ctx(m)
        c.prep(data["A"][2], data["A"][1])
        assert _L().hd_num_chains(c.ctx) == 2
        _refill_check(c, data["A"], data["C"], [3, 17, 40], _tables("ddpm", 10))   # slots of both chains
        free(m)


@pytest.mark.gpu
def test_variant_latent32(weights16, gpu):
    from hifidiff_amd import synth
    w32 = synth.refiner_state_dict(32, reuse=(weights16, 16))
    m = make_model(w32, 32)
    A = synth.sample_inputs(8, 32)
    C = synth.sample_inputs(2, 32, seed=901)
    _refill_check(Ctx(m), A, C, [1, 6], _tables("ddpm", 10))
    free(m)


@pytest.mark.gpu
def test_variant_unconditional_denoiser(weights16, gpu):
    from hifidiff_amd import sampling
    u = make_denoiser(weights16)
    s, _, _ = _tables("ddpm", 8)
    cs = sampling.ContinuousSampler(u, s, batch=8, refill_every=3)
    ids = [cs.submit(None, None, seed=40 + i) for i in range(12)]
    out = cs.drain()
    assert sorted(out) == ids
    for i in ids:
        lat, start = cs._start(None, 40 + i, 1.0)
        got = sampling.sample(u, lat[None].expand(8, 4, 16, 16).contiguous().cuda(), None, None, s, start_steps=start,
                              face_seeds=[40 + i] * 8)[0].cpu()
        assert torch.equal(out[i].cpu(), got), i
    e = u.engine
    z = torch.zeros((1, 4, 16, 16), device="cuda")
    sl = (ctypes.c_int32 * 1)(0)
    assert _L().hd_prepare_slots(e.ctx, 1, sl, z.data_ptr(), None, z.data_ptr(), None) == ERR_INVALID   # nothing to refill
    free(u)


@pytest.mark.gpu
def test_argument_checks(c64, data):
    x, crl, crf = data["A"]
    c64.prep(crf, crl)
    L = _L()
    ctx = c64.ctx
    crlc, crfc = data["C"][1].cuda(), data["C"][2].cuda()
    emb = torch.zeros((3, 2048), device="cuda")

    def ps(slots, n=None, lat=crlc, face=crfc, e=None):
        arr = (ctypes.c_int32 * max(1, len(slots)))(*slots)
        return L.hd_prepare_slots(ctx, len(slots) if n is None else n, arr, None if lat is None else lat.data_ptr(),
                                  None if face is None else face.data_ptr(), None if e is None else e.data_ptr(), None)

    assert ps([3, 3, 4]) == ERR_INVALID and ps([3, 64, 4]) == ERR_INVALID and ps([-1, 2, 4]) == ERR_INVALID
    assert ps([1, 2, 3], n=0) == ERR_INVALID and ps([1, 2, 3], n=65) == ERR_INVALID
    assert ps([1, 2, 3], face=None) == ERR_INVALID and ps([1, 2, 3], e=emb) == ERR_INVALID and ps([1, 2, 3], lat=None) == ERR_INVALID
    assert L.hd_prepare_slots(ctx, 1, None, crlc.data_ptr(), crfc.data_ptr(), None, None) == ERR_INVALID
    assert ps([1, 2, 3], face=None, e=emb) == 0                         # the identity embedding instead of cr_face
    with pytest.raises(ValueError):
        c64.m.prepare_slots([1, 1], crfc[:2], crlc[:2])
    with pytest.raises(RuntimeError):
        c64.m.prepare_slots([1, 2], crfc[:1], crlc[:1])
    bare = ctypes.c_void_p()                                            # no weights, no batch
    assert L.hd_create(ctypes.byref(bare), 16, 0) == 0
    assert L.hd_prepare_slots(bare, 1, (ctypes.c_int32 * 1)(0), crlc.data_ptr(), crfc.data_ptr(), None, None) == ERR_NOT_READY
    L.hd_destroy(bare)
    cr = ctypes.c_void_p()
    assert L.hd_cr_create(ctypes.byref(cr), 0) == 0
    assert L.hd_prepare_slots(cr, 1, (ctypes.c_int32 * 1)(0), crlc.data_ptr(), crfc.data_ptr(), None, None) == ERR_INVALID
    L.hd_destroy(cr)
    # hd_sample_faces*: rows / n_iters / resume
    ddpm, dpm = _tables("ddpm", 6), _tables("dpm", 6)
    assert c64.faces_rc(x, ddpm, [0] * 64, 7)[0] == ERR_INVALID
    assert c64.faces_rc(x, ddpm, [7] + [0] * 63, 2)[0] == ERR_INVALID
    assert c64.faces_rc(x, dpm, [0] * 64, 2, resume=[2] + [0] * 63)[0] == ERR_INVALID
    c64.prep(crf, crl)
    assert c64.faces_rc(x, dpm, [0] * 64, 2, resume=[1] * 64)[0] == ERR_INVALID    # no history after hd_prepare
    sch = c64.sch(dpm[1], dpm[2])
    rows = (ctypes.c_int32 * 64)()
    assert L.hd_sample_faces_multistep(ctx, x.cuda().data_ptr(), ctypes.byref(sch), rows, 2, None, None, None, 0, None) == ERR_INVALID
    assert L.hd_sample_faces(ctx, x.cuda().data_ptr(), ctypes.byref(c64.sch(ddpm[1], ddpm[2])), None, 2, None, None, 0, None) == ERR_INVALID
    assert L.hd_check(ctx) == 0
