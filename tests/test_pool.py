"""The conditioning pool on the GPU: hd_pool_config / hd_pool_prepare / hd_pool_commit (hd_prepare_slots in two halves, with a pool of
prepared conditioning between them) and sampling.ContinuousSampler(prefetch=...) on top of them.

A pool entry is a copy of the staging chain's face, and a commit a copy of the entry, so everything below that compares conditioning
compares bits: against hd_prepare_slots of the same faces in the same order, and against hd_prepare of those faces as a batch of their
own.  Shapes are the smallest that still take every path of the copy kernel: batch 8 at latent 16 has per-face sizes from 1 float (w_s of
the 1 x 1 level: the scalar path) to 32768 (prior 4: more than one sweep of the 16-byte path is needed at latent 32 only, which has its own
test), 3 new faces, entries and slots out of order."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2, weights16  # noqa: F401  (weights16: session fixture)
from test_slots import BUFS, ERR_INVALID, ERR_NOT_READY, TRAJ_TOL, Ctx, _env, _L, _tables, free, make_denoiser, make_model

B = 8
ENTRIES, SLOTS = [5, 0, 2], [3, 6, 1]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


class PCtx(Ctx):
    def pool(self, capacity):
        self.e.enable_pool(capacity)

    def pprep(self, entries, crf, crl):
        self.e.pool_prepare(entries, crl.cuda(), cr_face=crf.cuda())

    def commit(self, slots, entries):
        self.e.pool_commit(slots, entries)

    def bufs(self, n):
        torch.cuda.synchronize()
        return {k: self.read(k, n) for k in BUFS}

    def counters(self):
        return self.opt(b"graph_captures"), self.opt(b"rows_stage_launches")


@pytest.fixture(scope="module")
def data(gpu):
    from hifidiff_amd import synth
    return {"A": synth.sample_inputs(B, 16), "C": synth.sample_inputs(3, 16, seed=901), "D": synth.sample_inputs(3, 16, seed=905)}


@pytest.fixture(scope="module")
def c8(gpu, weights16):
    m = make_model(weights16)
    yield PCtx(m)
    free(m)


@pytest.fixture(scope="module")
def ref(c8, data):
    """Computed once, read-only: the 17 buffers of hd_prepare(C) as a batch of 3, of the batch A, and of A after hd_prepare_slots(SLOTS, C)."""
    (_, crl, crf), (_, crlc, crfc) = data["A"], data["C"]
    c8.prep(crfc, crlc)
    b3 = c8.bufs(3)
    c8.prep(crf, crl)
    old = c8.bufs(B)
    c8.refill(SLOTS, crfc, crlc)
    return {"b3": b3, "old": old, "refilled": c8.bufs(B)}


def _same(got, want, rows=slice(None), wrows=slice(None)):
    for k in BUFS:
        assert np.array_equal(got[k][rows], want[k][wrows]), k


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.gpu
def test_prepare_then_commit_equals_prepare_slots(c8, data, ref):
    (_, crl, crf), (_, crlc, crfc) = data["A"], data["C"]
    c8.prep(crf, crl)
    c8.pool(6)
    assert (c8.opt(b"pool_capacity"), c8.opt(b"pool_valid")) == (6, 0)
    c8.pprep(ENTRIES, crfc, crlc)
    assert c8.opt(b"pool_valid") == 3
    _same(c8.bufs(B), ref["old"])                                    # the prepare alone writes no slot
    c8.commit(SLOTS, ENTRIES)
    new = c8.bufs(B)
    _same(new, ref["refilled"])                                      # every slot: the three as hd_prepare_slots leaves them, the others untouched
    keep = [f for f in range(B) if f not in SLOTS]
    _same(new, ref["old"], keep, keep)
    _same(new, ref["b3"], SLOTS)
    assert c8.opt(b"pool_valid") == 3                                # entries stay valid after a commit
    assert not np.array_equal(new["prior4"][SLOTS], ref["old"]["prior4"][SLOTS])   # the slots did change: the check is not vacuous
    sizes = sorted({new[k].shape[1] for k in BUFS})
    assert sizes[0] == 1 and sizes[-1] == 32768                      # the scalar path and the largest 16-byte copy were both in it


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.gpu
def test_commits_split_and_reordered(c8, data, ref):
    (x, crl, crf), (xc, crlc, crfc) = data["A"], data["C"]
    tab = _tables("ddim", 8)
    c8.prep(crf, crl)
    c8.pool(6)
    c8.pprep(ENTRIES, crfc, crlc)                                    # entry 5: face C0, entry 0: C1, entry 2: C2
    c8.commit([6], [0])
    x2 = c8.faces(x, tab, [0] * B, 2)
    assert bool(torch.isfinite(x2).all())
    c8.commit([1, 3], [2, 5])
    new = c8.bufs(B)
    _same(new, ref["b3"], SLOTS)                                     # slots 3, 6, 1 hold C0, C1, C2: hd_prepare(C) as a batch of 3
    _same(new, ref["refilled"])


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.gpu
def test_one_entry_into_two_slots(c8, data, ref):
    (x, crl, crf), (xc, crlc, crfc) = data["A"], data["C"]
    tab = _tables("ddpm", 8)
    c8.prep(crf, crl)
    c8.pool(6)
    c8.pprep(ENTRIES, crfc, crlc)
    c8.commit([2, 5], [0, 0])
    new = c8.bufs(B)
    _same(new, ref["b3"], [2, 5], [1, 1])
    xs = x.clone()
    xs[2] = xs[5] = xc[1]
    seeds = np.arange(B, dtype=np.uint64) + 11
    seeds[2] = seeds[5] = 0xFACE5EED
    out = c8.faces(xs, tab, [0] * B, 8, seeds=seeds)
    assert torch.equal(out[2], out[5]) and not torch.equal(out[2], out[4])
    seeds[5] = 77                                                    # several seeds of one face: one prologue, different samples
    assert not torch.equal(c8.faces(xs, tab, [0] * B, 8, seeds=seeds)[5], out[5])


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.gpu
def test_pool_prepare_leaves_the_running_batch_alone(c8, data):
    (x, crl, crf), (_, crlc, crfc) = data["A"], data["C"]
    tab = _tables("ddpm", 8)
    seeds = np.arange(B, dtype=np.uint64) * 7919 + 5
    n1, n2 = 4, 4
    c8.pool(6)
    c8.prep(crf, crl)
    x1 = c8.faces(x, tab, [0] * B, n1, seeds=seeds)
    plain = c8.faces(x1, tab, [n1] * B, n2, seeds=seeds)
    c8.prep(crf, crl)
    x1b = c8.faces(x, tab, [0] * B, n1, seeds=seeds)
    assert torch.equal(x1b, x1)
    before = c8.counters()
    c8.pprep(ENTRIES, crfc, crlc)
    assert c8.counters() == before
    assert torch.equal(c8.faces(x1b, tab, [n1] * B, n2, seeds=seeds), plain)
    c8.commit(SLOTS, ENTRIES)
    assert c8.counters() == before                                   # nothing captured, the same stage launches, through the commit too
    keep = [f for f in range(B) if f not in SLOTS]
    again = c8.faces(x1b, tab, [n1] * B, n2, seeds=seeds)
    assert c8.counters() == before
    assert torch.equal(again[keep], plain[keep]) and not torch.equal(again[SLOTS], plain[SLOTS])


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.gpu
def test_repreparing_a_committed_entry_leaves_its_slot(c8, data, ref):
    (_, crl, crf), (_, crlc, crfc), (_, crld, crfd) = data["A"], data["C"], data["D"]
    c8.prep(crf, crl)
    c8.pool(6)
    c8.pprep([0], crfc[:1], crlc[:1])
    c8.commit([4], [0])
    first = c8.bufs(B)
    assert not np.array_equal(first["prior4"][4], ref["old"]["prior4"][4])
    c8.pprep([0], crfd[:1], crld[:1])                                # entry 0 now holds another face
    _same(c8.bufs(B), first)
    c8.commit([5], [0])
    now = c8.bufs(B)
    keep = [f for f in range(B) if f != 5]
    _same(now, first, keep, keep)
    assert not np.array_equal(now["prior4"][5], now["prior4"][4])


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.gpu
def test_commit_resets_what_prepare_slots_resets(c8, data):
    (x, crl, crf), (xc, crlc, crfc) = data["A"], data["C"]
    tab = _tables("dpm", 8)
    e = c8.e
    e.enable_previews(1, 0)
    try:
        c8.prep(crf, crl)
        c8.pool(6)
        c8.pprep([1], crfc[:1], crlc[:1])
        box = torch.zeros((2, 16, 16))
        box[:, 4:12, 4:12] = 1.0
        e.set_mask(box, crl[[2, 4]], x[[2, 4]], slots=[2, 4])
        e.set_guidance(crl[[2, 4]], 0.5, 4, slots=[2, 4])
        assert (c8.opt(b"masked_faces"), c8.opt(b"guided_faces")) == (2, 2)
        x2 = c8.faces(x, tab, [0] * B, 2, resume=[0] * B)
        assert e.previews([2, 4])[1].cpu().tolist() == [1, 1]
        c8.commit([2], [1])
        assert (c8.opt(b"masked_faces"), c8.opt(b"guided_faces")) == (1, 1)
        assert e.previews([2, 4])[1].cpu().tolist() == [-1, 1]
        assert not bool(e.previews([2])[0].any())                    # a zeroed plane
        x2[2] = xc[0]
        rows = [2] * B
        rows[2] = 0
        rc, _ = c8.faces_rc(x2, tab, rows, 2, resume=[1] * B)         # the committed slot has no history
        assert rc == ERR_INVALID
        rc, _ = c8.rows_rc(x2, tab, rows, 2, resume=1)                # nor has the batch as a whole
        assert rc == ERR_INVALID
        resume = [1] * B
        resume[2] = 0
        assert bool(torch.isfinite(c8.faces(x2, tab, rows, 2, resume=resume)).all())   # an untouched slot resumes
    finally:
        e.clear_mask()
        e.disable_guidance()
        e.disable_previews()


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.gpu
def test_entries_survive_prepare_at_another_batch_size(c8, data, ref):
    (_, crl, crf), (_, crlc, crfc) = data["A"], data["C"]
    c8.prep(crf, crl)
    c8.pool(6)
    c8.pprep(ENTRIES, crfc, crlc)
    c8.prep(crf[:4], crl[:4])                                        # batch 4: another workspace, the batch-8 one is parked
    assert (c8.opt(b"pool_capacity"), c8.opt(b"pool_valid")) == (6, 3)
    old4 = c8.bufs(4)
    c8.commit([1, 3, 0], ENTRIES)
    new4 = c8.bufs(4)
    _same(new4, ref["b3"], [1, 3, 0])
    _same(new4, old4, [2], [2])
    c8.prep(crf, crl)                                                # ... and back
    c8.commit(SLOTS, ENTRIES)
    _same(c8.bufs(B), ref["refilled"])


# ------------------------------------------------------------------------------------------------ 8
@pytest.mark.gpu
def test_variant_two_chains(weights16, data):
    (x, crl, crf), (xc, crlc, crfc) = data["A"], data["C"]
    tab = _tables("ddpm", 8)
    with _env({"HD_EXPERIMENTS": "1", "HD_CHAINS": "2"}):
        m = make_model(weights16)
        c = PCtx(m)
        c.prep(crf, crl)
        assert _L().hd_num_chains(c.ctx) == 2                        # 4 faces per chain: slots 3 and 1 in chain 0, slot 6 in chain 1
        c.refill(SLOTS, crfc, crlc)
        want = c.bufs(4)                                             # the debug names read chain 0
        xs = x.clone()
        xs[SLOTS] = xc
        want_x = c.faces(xs, tab, [0] * B, 4)                        # chain 1's slot is compared through the loop
        c.prep(crf, crl)
        c.e.enable_pool(6)
        c.pprep(ENTRIES, crfc, crlc)
        c.commit(SLOTS, ENTRIES)
        _same(c.bufs(4), want)
        assert torch.equal(c.faces(xs, tab, [0] * B, 4), want_x)
        free(m)


@pytest.mark.gpu
def test_variant_latent32(weights16, gpu):
    from hifidiff_amd import synth
    w32 = synth.refiner_state_dict(32, reuse=(weights16, 16))
    m = make_model(w32, 32)
    c = PCtx(m)
    _, crl, crf = synth.sample_inputs(B, 32)
    _, crlc, crfc = synth.sample_inputs(2, 32, seed=901)
    c.prep(crf, crl)
    c.refill([1, 6], crfc, crlc)
    want = c.bufs(B)
    c.prep(crf, crl)
    c.e.enable_pool(2)
    c.pprep([1, 0], crfc, crlc)
    c.commit([1, 6], [1, 0])
    got = c.bufs(B)
    _same(got, want)
    assert got["prior4"].shape[1] == 4 * 32768 and got["ws0"].shape[1] == 4      # S = 2: every size times 4
    free(m)


@pytest.mark.gpu
def test_variant_id_emb(c8, data):
    (_, crl, crf), (_, crlc, _) = data["A"], data["C"]
    emb = torch.randn((3, 2048), generator=torch.Generator().manual_seed(3)).cuda()
    c8.prep(crf, crl)
    c8.e.prepare_slots(SLOTS, crlc.cuda(), id_emb=emb)
    want = c8.bufs(B)
    assert np.array_equal(want["id_emb"][SLOTS], emb.cpu().numpy())
    c8.prep(crf, crl)
    c8.pool(6)
    c8.e.pool_prepare(ENTRIES, crlc.cuda(), id_emb=emb)
    c8.commit(SLOTS, ENTRIES)
    _same(c8.bufs(B), want)


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.gpu
def test_continuous_sampler_with_prefetch(c8, data):
    """20 requests through 8 slots at refill_every=1 with a pool of 8: every request against the same request sampled alone, replicated
    into every slot, within TRAJ_TOL as tests/test_slots.py compares them (a pooled request's conditioning is computed at the batch size
    of its pool_prepare call: the ResNet-50's GEMMs pick their launch form by row count)."""
    from hifidiff_amd import sampling, synth
    N = 20
    _, crl, crf = synth.sample_inputs(N, 16, seed=903)
    strength = (0.2 + 0.8 * torch.rand(N, generator=torch.Generator().manual_seed(903))).tolist()
    s, _, _ = _tables("ddim", 10)
    box = torch.zeros((16, 16))
    box[4:12, 2:14] = 1.0
    masks = {9: box, 14: box}                                        # both arrive through the pool, as do the guided ones
    fid = {11: (0.5, 4), 14: (0.7, 8)}
    m = c8.m
    cs = sampling.ContinuousSampler(m, s, batch=B, refill_every=1, prefetch=8)
    ids = []
    for i in range(N):
        kw = {} if i not in fid else dict(fidelity=fid[i][0], fidelity_scale=fid[i][1])
        ids.append(cs.submit(crf[i], crl[i], seed=500 + i, strength=strength[i], mask=masks.get(i), **kw))
    try:
        out = cs.drain()
        assert sorted(out) == ids
        assert cs.refilled == N - B == cs.pool_prepared
        print(f"ContinuousSampler(prefetch=8): {cs.refilled} requests refilled by {cs.pool_calls} pool_prepare calls in {cs.calls} steps")
        assert 1 <= cs.pool_calls <= -(-(N - B) // B) + 1
        worst, exact = 0.0, 0
        rep = lambda t: t[None].expand(B, *t.shape).contiguous()      # noqa: E731  (the request in every slot; slot 0 is compared)
        for i in ids:
            lat, start = cs._start(crl[i], 500 + i, strength[i], i in masks)
            kw = {}
            if i in masks:
                kw.update(mask=rep(masks[i]), known=rep(crl[i]), known_noise=rep(cs._z(500 + i)[0]))
            if i in fid:
                kw.update(guide=rep(crl[i]), guide_weight=fid[i][0], guide_scale=fid[i][1])
            got = sampling.sample(m, rep(lat).cuda(), rep(crf[i]).cuda(), rep(crl[i]).cuda(), s, start_steps=start,
                                  face_seeds=[500 + i] * B, **kw)[0].cpu()
            r = rel_l2(out[i].cpu(), got)
            worst, exact = max(worst, r), exact + int(torch.equal(out[i].cpu(), got))
            if i in masks:
                keep = (masks[i] == 0)[None].expand(4, 16, 16)
                assert torch.equal(out[i].cpu()[keep], crl[i].float()[keep]), i
        print(f"ContinuousSampler(prefetch=8) vs each request alone: {exact}/{N} bit-identical, worst rel-L2 {worst:.2e}")
        assert worst <= TRAJ_TOL, worst
    finally:
        m.clear_mask()
        m.disable_guidance()
        m.disable_pool()


# ------------------------------------------------------------------------------------------------ 10
@pytest.mark.gpu
def test_argument_checks(c8, data, weights16):
    (x, crl, crf), (_, crlc, crfc) = data["A"], data["C"]
    L, ctx = _L(), c8.ctx
    crlc, crfc = crlc.cuda(), crfc.cuda()
    emb = torch.zeros((3, 2048), device="cuda")
    i32 = lambda v: (ctypes.c_int32 * max(1, len(v)))(*v)            # noqa: E731

    def pp(entries, n=None, lat=crlc, face=crfc, e=None, c=None):
        return L.hd_pool_prepare(c or ctx, len(entries) if n is None else n, i32(entries), None if lat is None else lat.data_ptr(),
                                 None if face is None else face.data_ptr(), None if e is None else e.data_ptr(), None)

    def pc(slots, entries, n=None, c=None):
        return L.hd_pool_commit(c or ctx, len(slots) if n is None else n, i32(slots), i32(entries), None)

    c8.prep(crf, crl)
    assert L.hd_pool_config(ctx, -1) == ERR_INVALID and L.hd_pool_config(ctx, 4097) == ERR_INVALID
    assert L.hd_pool_config(ctx, 0) == 0 and c8.opt(b"pool_capacity") == 0
    assert pp([0, 1, 2]) == ERR_NOT_READY and pc([0], [0]) == ERR_NOT_READY          # no pool
    assert b"hd_pool_config" in L.hd_last_error(ctx)
    c8.pool(6)
    assert pc([0], [0]) == ERR_INVALID and b"entries[0]" in L.hd_last_error(ctx)    # never prepared
    assert pp([0, 1, 1]) == ERR_INVALID and b"entries" in L.hd_last_error(ctx)      # a duplicate entry
    assert pp([0, 6, 1]) == ERR_INVALID and pp([-1, 2, 1]) == ERR_INVALID
    assert pp([0, 1, 2], n=0) == ERR_INVALID and b"n = 0" in L.hd_last_error(ctx)
    assert pp(list(range(7)), n=7) == ERR_INVALID                                   # n beyond the capacity (6 < B)
    assert pp([0, 1, 2], face=None) == ERR_INVALID and pp([0, 1, 2], e=emb) == ERR_INVALID and pp([0, 1, 2], lat=None) == ERR_INVALID
    assert L.hd_pool_prepare(ctx, 1, None, crlc.data_ptr(), crfc.data_ptr(), None, None) == ERR_INVALID
    assert c8.opt(b"pool_valid") == 0                                               # a refused call marks nothing
    assert pp([0, 1, 2]) == 0 and c8.opt(b"pool_valid") == 3
    assert pc([1, 1], [0, 1]) == ERR_INVALID and b"slots" in L.hd_last_error(ctx)   # a duplicate slot
    assert pc([8], [0]) == ERR_INVALID and pc([-1], [0]) == ERR_INVALID and pc([0], [6]) == ERR_INVALID and pc([0], [-1]) == ERR_INVALID
    assert pc([0], [3]) == ERR_INVALID                                              # in range, never prepared
    assert pc([0], [0], n=0) == ERR_INVALID and pc(list(range(9)), [0] * 9) == ERR_INVALID
    assert L.hd_pool_commit(ctx, 1, None, i32([0]), None) == ERR_INVALID and L.hd_pool_commit(ctx, 1, i32([0]), None, None) == ERR_INVALID
    assert pc([0, 7], [1, 1]) == 0                                                  # an entry may repeat
    L.hd_pool_config(ctx, 12)                                                       # a pool larger than the batch: n is limited by B
    assert c8.opt(b"pool_valid") == 0 and pp(list(range(9)), n=9) == ERR_INVALID
    c8.pool(6)
    # the Python wrappers
    with pytest.raises(ValueError):
        c8.m.pool_prepare([1, 1], crfc[:2], crlc[:2])
    with pytest.raises(RuntimeError):
        c8.m.pool_prepare([1, 2], crfc[:1], crlc[:1])
    with pytest.raises(ValueError):
        c8.m.pool_commit([1, 2], [0])
    with pytest.raises(ValueError):
        c8.m.enable_pool(0)
    bare = ctypes.c_void_p()                                                        # no weights, no batch
    assert L.hd_create(ctypes.byref(bare), 16, 0) == 0
    assert L.hd_pool_config(bare, 2) == 0
    assert pp([0], n=1, c=bare) == ERR_NOT_READY and pc([0], [0], c=bare) == ERR_NOT_READY
    L.hd_destroy(bare)
    cr = ctypes.c_void_p()
    assert L.hd_cr_create(ctypes.byref(cr), 0) == 0
    assert L.hd_pool_config(cr, 2) == ERR_INVALID and pp([0], n=1, c=cr) == ERR_INVALID and pc([0], [0], c=cr) == ERR_INVALID
    L.hd_destroy(cr)
    vae = ctypes.c_void_p()
    assert L.hd_vae_create(ctypes.byref(vae), 0) == 0
    assert L.hd_pool_config(vae, 2) == ERR_INVALID and pp([0], n=1, c=vae) == ERR_INVALID and pc([0], [0], c=vae) == ERR_INVALID
    assert b"VAE" in L.hd_last_error(vae)
    L.hd_destroy(vae)
    u = make_denoiser(weights16)
    u.engine.ensure(torch.device("cuda", 0))
    assert L.hd_pool_config(u.engine.ctx, 2) == ERR_INVALID and pp([0], n=1, c=u.engine.ctx) == ERR_INVALID
    assert pc([0], [0], c=u.engine.ctx) == ERR_INVALID
    with pytest.raises(RuntimeError):
        u.engine.enable_pool(2)
    free(u)
    # the context is still usable
    assert pp([3, 4, 5]) == 0 and pc([2], [4]) == 0
    tab = _tables("ddim", 8)
    assert bool(torch.isfinite(c8.faces(x, tab, [0] * B, 2)).all())
    assert L.hd_check(ctx) == 0
