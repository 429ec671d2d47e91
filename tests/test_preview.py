"""Progress previews: hd_preview_config / hd_preview_read, model.previews(), sampling.sample(previews=...) and ContinuousSampler.previews().

The preview of row k is the x0 the step kernels compute on that row anyway, stored once more.  So every comparison here is bit for bit
(torch.equal): against the multistep history (the parent's own store of the same register), against the final latents where the table's
last row returns x0 itself, against the same loop stopped earlier, and -- the neutrality -- the latents with previews on against off.
Only the oracle comparison carries a bound, the 2e-2 rel-L2 that tests/test_mask.py and tests/test_multistep.py put on the latents of the
same loop.  As in those files, comparisons between hd_sample and the per-face form run with "xcd2" off."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2, weights16  # noqa: F401  (weights16: session fixture)
from test_mask import Runner, _L, _tables, box, free, make_denoiser, make_model

ERR_INVALID, ERR_NOT_READY = -1, -4
I32P = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).contiguous()


class PRunner(Runner):
    """tests/test_mask.py's Runner with the remaining loop entry points and the two preview calls."""

    def config_rc(self, on, every=1, snapshots=0):
        return _L().hd_preview_config(self.ctx, on, every, snapshots)

    def config(self, on, every=1, snapshots=0):
        assert self.config_rc(on, every, snapshots) == 0, _L().hd_last_error(self.ctx)
        assert self.opt("preview") == on

    def read_rc(self, n, slots, snapshot, with_rows=True):
        L = self.e.latent_res
        x0 = torch.full((max(n, 1), 4, L, L), float("nan"), device="cuda")
        rows = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
        sl = None if slots is None else _i32(slots)
        rc = _L().hd_preview_read(self.ctx, n, None if sl is None else ctypes.cast(sl.data_ptr(), I32P), snapshot, x0.data_ptr(),
                                  rows.data_ptr() if with_rows else None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, x0.cpu(), rows.cpu()

    def preview(self, snapshot=-1, slots=None):
        rc, x0, rows = self.read_rc(self.e.batch if slots is None else len(slots), slots, snapshot)
        assert rc == 0, _L().hd_last_error(self.ctx)
        return x0, rows

    def faces_ms(self, x, ts, coef, rows, n_iters, resume, seeds=None, seed=0):
        xd = x.cuda().float().contiguous().clone()
        sch, r, res = self._sch(ts, coef), _i32(rows), _i32(resume)
        sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        self._run(_L().hd_sample_faces_multistep(self.ctx, xd.data_ptr(), ctypes.byref(sch), ctypes.cast(r.data_ptr(), I32P), n_iters,
                                                 ctypes.cast(res.data_ptr(), I32P),
                                                 None if sd is None else sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None, seed,
                                                 torch.cuda.current_stream().cuda_stream))
        return xd.cpu()

    def spans(self, x, ts, coef, begin, end, rows, n_iters, resume, seeds=None, seed=0):
        xd = x.cuda().float().contiguous().clone()
        sch, b, e, r, res = self._sch(ts, coef), _i32(begin), _i32(end), _i32(rows), _i32(resume)
        sd = None if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        p = lambda t: ctypes.cast(t.data_ptr(), I32P)  # noqa: E731
        self._run(_L().hd_sample_spans(self.ctx, xd.data_ptr(), ctypes.byref(sch), p(b), p(e), p(r), n_iters, p(res),
                                       None if sd is None else sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None, seed,
                                       torch.cuda.current_stream().cuda_stream))
        return xd.cpu()


def _set_table():
    """A ScheduleSet of DDIM-4 and DPM-8: (sset, ts [12], coef [12,8]); rows [0, 4) and [4, 12)."""
    from hifidiff_amd import sampling
    sset = sampling.ScheduleSet({"ddim4": _tables("ddim", 4)[0], "dpm8": _tables("dpm", 8)[0]})
    ts, coef = sset.coefficient_table()
    return sset, ts.float().contiguous(), coef.float().contiguous()


def _returns_x0(row):
    """Does this coefficient row hand back x0 itself: c3 == 1 and c4 == c5 == c6 (== c7) == 0."""
    r = [float(v) for v in row]
    return r[3] == 1.0 and all(v == 0.0 for v in r[4:])


def _pad8(coef):
    return torch.cat([coef, torch.zeros((coef.shape[0], 1))], dim=1).contiguous()


@pytest.fixture(scope="module")
def data2(gpu):
    from hifidiff_amd import synth
    return synth.sample_inputs(2, 16)


@pytest.fixture(scope="module")
def run2(gpu, weights16, data2):
    x, crl, crf = data2
    m = make_model(weights16)
    run = PRunner(m, crf, crl)
    yield run
    free(m)


def _seven(run, x):
    """Every loop entry point once on a batch of 2 (10 rows: DDIM, DDPM with device Philox, DPM-Solver++ 2M) plus the span form."""
    _, td, cd = _tables("ddim", 10)
    _, tp, cp = _tables("ddpm", 10)
    _, tm, cm = _tables("dpm", 10)
    _, tss, css = _set_table()
    return [
        ("hd_sample ddim", lambda: run.full(x, td, cd)),
        ("hd_sample ddpm", lambda: run.full(x, tp, cp, seed=11)),
        ("hd_sample_multistep", lambda: run.full(x, tm, cm)),
        ("hd_sample_rows", lambda: run.rows(x, td, cd, [0, 3], 10)),
        ("hd_sample_rows ddpm", lambda: run.rows(x, tp, cp, [2, 0], 10, seed=11)),
        ("hd_sample_rows_multistep", lambda: run.rows(x, tm, cm, [0, 3], 10)),
        ("hd_sample_faces", lambda: run.faces(x, tp, cp, [0, 4], 10, [5, 6])),
        ("hd_sample_faces_multistep", lambda: run.faces_ms(x, tm, cm, [1, 0], 10, [0, 0], [5, 6])),
        ("hd_sample_spans", lambda: run.spans(x, tss, css, [0, 4], [4, 12], [0, 5], 7, [0, 0], [5, 6])),
    ]


def _check_neutral(run, x):
    calls = _seven(run, x)
    run.config(0)
    for _, fn in calls:                                               # captures both forms of the graphs and grows the tables to the longest
        fn()                                                          # schedule (12 rows: a FiLM table that grows makes the graphs stale)
    off = [fn() for _, fn in calls]
    before = run.counters()
    run.config(1, 1, 4)
    assert run.counters() == before
    on = [fn() for _, fn in calls]
    x0, rows = run.preview()
    assert bool((rows >= 0).all()) and bool(torch.isfinite(x0).all())  # the previews were on: every face has written one
    run.config(1, 3, 64)                                              # resized: nothing recaptured
    on2 = [fn() for _, fn in calls]
    run.config(0)
    again = [fn() for _, fn in calls]
    assert run.counters() == before, (run.counters(), before)
    for (name, _), a, b, c, d in zip(calls, off, on, on2, again):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d), name


def _check_last_row(run, x, kinds=("ddim", "dpm"), n=10):
    """Where the table's last row returns x0 itself the latest preview after a full loop is the returned latents."""
    run.config(1, 1, 0)
    for kind in kinds:
        _, ts, coef = _tables(kind, n)
        assert _returns_x0(coef[-1]), (kind, coef[-1].tolist())       # what the table says, not what we assume
        out = run.full(x, ts, coef)
        x0, rows = run.preview()
        assert rows.tolist() == [n - 1] * x.shape[0], (kind, rows.tolist())
        assert torch.equal(x0, out), (kind, float((x0 - out).abs().max()))
    run.config(0)


# ------------------------------------------------------------------------------------------------ 1. neutrality
@pytest.mark.gpu
def test_previews_change_no_bit_of_the_latents(run2, data2):
    assert run2.opt("end_fold") == 1                                  # hca_ending_conv_kernel
    _check_neutral(run2, data2[0])


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["xcd", "face"])
def test_previews_change_no_bit_in_the_unfused_programs(run2, data2, key):
    _L().hd_set_option(run2.ctx, key.encode(), 0)
    try:
        _check_neutral(run2, data2[0])
        _check_last_row(run2, data2[0], kinds=("ddim",))
    finally:
        _L().hd_set_option(run2.ctx, key.encode(), 1)


# ------------------------------------------------------------------------------------------------ 2. last row
@pytest.mark.gpu
def test_last_row_preview_is_the_result(run2, data2):
    _check_last_row(run2, data2[0])


# ------------------------------------------------------------------------------------------------ 3. the value, through the parent's own store
@pytest.mark.gpu
def test_preview_is_the_multistep_history(run2, data2):
    x = data2[0]
    shape = (2, 4, 16, 16)
    run2.config(1, 1, 0)
    _, ts, coef = _tables("dpm", 10)
    xi, at = x.float(), 0
    for it in (1, 2, 3, 1, 3):                                        # a loop split into calls of 1, 2 and 3 iterations
        xi = run2.rows(xi, ts, coef, [at] * 2, it, resume=int(at > 0))
        at += it
        x0, rows = run2.preview()
        assert rows.tolist() == [at - 1] * 2
        assert torch.equal(x0, run2.read("x0_hist", shape)), at
        assert torch.equal(x0, run2.read("x0_preview", shape))        # the debug name reads the same plane
    assert at == 10
    for kind, kw in (("ddim", {}), ("ddpm", {"seed": 11})):           # 7 columns: the same rows with c7 = 0 through the multistep entry
        _, ts7, c7 = _tables(kind, 10)
        want = run2.full(x, ts7, c7, **kw)
        x0_7, rows7 = run2.preview()
        got = run2.full(x, ts7, _pad8(c7), **kw)
        assert torch.equal(got, want), kind                           # the guarantee hd_sample_spans documents for a c7 = 0 row
        x0, rows = run2.preview()
        assert torch.equal(x0, run2.read("x0_hist", shape)) and rows.tolist() == [9, 9], kind
        assert torch.equal(x0, x0_7) and rows7.tolist() == [9, 9], kind   # and hd_sample itself stored the same estimate
    run2.config(0)


# ------------------------------------------------------------------------------------------------ 4. snapshots against the split loop
@pytest.mark.gpu
def test_snapshots_against_the_split_loop(run2, data2):
    x = data2[0]
    _, ts, coef = _tables("ddim", 12)
    _L().hd_set_option(run2.ctx, b"xcd2", 0)                          # hd_sample against hd_sample_rows, bit for bit
    try:
        run2.config(1, 4, 3)
        out = run2.full(x, ts, coef)
        snaps = [run2.preview(s) for s in range(3)]
        latest = run2.preview()
        assert torch.equal(latest[0], out) and torch.equal(latest[0], snaps[2][0]) and latest[1].tolist() == [11, 11]
        snap_bits = run2.read("preview_snaps", (3, 2, 4, 16, 16))
        for s in range(3):
            assert snaps[s][1].tolist() == [4 * (s + 1) - 1] * 2
            assert torch.equal(snap_bits[s], snaps[s][0])
            run2.config(1, 4, 3)                                      # resets: row -1, zero planes
            z, zr = run2.preview()
            assert zr.tolist() == [-1, -1] and not bool(z.any())
            run2.rows(x, ts, coef, [0, 0], 4 * (s + 1))
            x0, rows = run2.preview()
            assert rows.tolist() == [4 * (s + 1) - 1] * 2
            assert torch.equal(x0, snaps[s][0]), s
            assert not torch.equal(x0, snaps[(s + 1) % 3][0])
        run2.config(1, 4, 2)                                          # two planes: the third snapshot is not written
        assert torch.equal(run2.full(x, ts, coef), out)
        for s in range(2):
            x0, rows = run2.preview(s)
            assert torch.equal(x0, snaps[s][0]) and rows.tolist() == [4 * (s + 1) - 1] * 2
        rc, _, _ = run2.read_rc(2, None, 2)
        assert rc == ERR_INVALID and _L().hd_last_error(run2.ctx)
        rows_bits = run2.read("preview_rows", (2,)).numpy().view(np.int32)
        assert rows_bits.tolist() == [11, 11]
    finally:
        run2.config(0)
        _L().hd_set_option(run2.ctx, b"xcd2", 1)


# ------------------------------------------------------------------------------------------------ 5. holds and spans
@pytest.mark.gpu
def test_holds_and_spans(gpu, weights16):
    from hifidiff_amd import synth
    x, crl, crf = synth.sample_inputs(3, 16)
    m = make_model(weights16)
    run = PRunner(m, crf, crl)
    _, ts, coef = _set_table()                                        # DDIM-4: rows [0, 4), DPM-8: rows [4, 12)
    begin, end = [0, 4, 12], [4, 12, 12]                              # face 2: an empty slot, begin == start == end
    run.config(1, 3, 3)
    off = run.spans(x, ts, coef, begin, end, [0, 4, 12], 5, [0, 0, 0], [1, 2, 3])
    x0, rows = run.preview()
    assert rows.tolist() == [3, 8, -1]                                # face 0 held after its 4 rows, face 1 at its 5th, face 2 never ran
    assert _returns_x0(coef[3])
    assert torch.equal(x0[0], off[0])                                 # its last row hands back x0
    assert not bool(x0[2].any()) and torch.equal(off[2], x[2].float())
    s0, r0 = run.preview(0)
    s1, r1 = run.preview(1)
    assert r0.tolist() == [2, 6, -1] and r1.tolist() == [-1, -1, -1]  # rows 3, 6, .. of each face's own schedule: begin_f + 3 (s + 1) - 1
    assert not bool(s0[2].any()) and not bool(s1.any())
    run.spans(x, ts, coef, begin, end, [0, 4, 12], 3, [0, 0, 0], [1, 2, 3])    # the same loop stopped after local row 2
    p3, pr3 = run.preview()
    assert pr3.tolist() == [2, 6, -1] and torch.equal(p3[:2], s0[:2])
    # a second call that runs only face 1 further: faces 0 and 2 are held from its first iteration on
    run.spans(x, ts, coef, begin, end, [0, 4, 12], 5, [0, 0, 0], [1, 2, 3])
    keep0, keep_s0 = run.preview()[0][0].clone(), run.preview(0)[0][0].clone()
    run.spans(off, ts, coef, begin, end, [4, 9, 12], 3, [0, 1, 0], [1, 2, 3])
    x0b, rowsb = run.preview()
    assert rowsb.tolist() == [3, 11, -1]
    assert torch.equal(x0b[0], keep0) and torch.equal(run.preview(0)[0][0], keep_s0) and not bool(x0b[2].any())
    s1b, r1b = run.preview(1)
    assert r1b.tolist() == [-1, 9, -1] and bool(s1b[1].any())         # local row 5 of face 1
    run.config(0)
    free(m)


# ------------------------------------------------------------------------------------------------ 6. against the oracle network
@pytest.mark.gpu
def test_against_the_oracle_network(gpu, weights16):
    """tests/test_mask.py::test_against_the_oracle_network's loop, unmasked: the oracle's x0 of rows 4 and 9 against the snapshots."""
    from hifidiff_amd import sampling, schedulers, synth
    from oracle import hifidiff_oracle as O
    from test_multistep import _update64
    x, crl, crf = synth.sample_inputs(2, 16)
    s = schedulers.DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    ts, coef = s.coefficient_table()
    cond = O.Conditioning(weights16, crl, crf, prec=O.BF16)
    xr, h, want = x.double(), None, {}
    for i, t in enumerate(s.timesteps.tolist()):
        eps = O.fused_denoiser(weights16, xr.float(), torch.full((x.shape[0],), t), prec=O.BF16, cond=cond).double()
        xr, h = _update64(xr, eps, coef[i], h)
        want[i] = h
    model = make_model(weights16)
    got, snaps, rows = sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), s, previews=5)
    assert tuple(snaps.shape) == (2, 2, 4, 16, 16) and rows.cpu().tolist() == [[4, 4], [9, 9]]
    assert model.engine.preview_cfg is None                           # the model's own setting (off) is back
    assert _L().hd_get_option(model.engine.ctx, b"preview") == 0
    for j, k in enumerate((4, 9)):
        r = rel_l2(snaps[j].cpu(), want[k])
        print(f"DPM-Solver++ 2M, 10 steps, x0 of row {k} against the oracle network: rel-L2 {r:.3e}")
        assert r <= 2e-2, (k, r)
    r = rel_l2(got.cpu(), xr)
    print(f"the latents of the same loop: rel-L2 {r:.3e}")
    assert torch.equal(got, sampling.sample(model, x.cuda(), crf.cuda(), crl.cuda(), s))
    free(model)


# ------------------------------------------------------------------------------------------------ 7. masks
@pytest.mark.gpu
def test_masked_faces_preview_the_blend(run2, data2):
    x, crl, _ = data2
    shape = (2, 4, 16, 16)
    mask = box(1, 16, 4, 12, 2, 14)
    run2.config(1, 1, 1)
    try:
        for kind in ("ddim", "dpm"):
            _, ts, coef = _tables(kind, 10)
            run2.rows(x, ts, coef, [0, 0], 1)
            plain, _ = run2.preview()
            hist_plain = run2.read("x0_hist", shape) if kind == "dpm" else None
            run2.mask(mask, crl[:1], x[:1], slots=[0])                # face 0 only
            run2.rows(x, ts, coef, [0, 0], 1)
            got, rows = run2.preview()
            snap, _ = run2.preview(0)
            assert rows.tolist() == [0, 0] and torch.equal(snap, got)
            keep = (mask[0] == 0)[None].expand(4, 16, 16)
            assert torch.equal(got[0][keep], crl[0].float()[keep]), kind      # m == 0: known, exactly
            assert torch.equal(got[0][~keep], plain[0][~keep]), kind          # m == 1: x0 of the row, which no blend of that row enters
            assert not torch.equal(got[0][keep], plain[0][keep])
            assert torch.equal(got[1], plain[1]), kind
            if kind == "dpm":
                assert torch.equal(run2.read("x0_hist", shape), hist_plain)   # the history keeps the unblended x0
            run2.clear()
    finally:
        run2.clear()
        run2.config(0)


# ------------------------------------------------------------------------------------------------ 8. lifetime and arguments
@pytest.mark.gpu
def test_lifetime_and_arguments(gpu, weights16, data2):
    from hifidiff_amd import _lib
    x, crl, crf = data2
    m = make_model(weights16)
    e = m.engine
    err = lambda: _L().hd_last_error(e.ctx)  # noqa: E731
    for on, every, snaps in ((2, 1, 0), (-1, 1, 0), (1, 0, 0), (1, -2, 0), (1, 1, -1), (1, 1, 65)):
        assert _L().hd_preview_config(e.ctx, on, every, snaps) == ERR_INVALID and err(), (on, every, snaps)
    assert _L().hd_get_option(e.ctx, b"preview") == 0
    m.enable_previews(2, 2)                                           # before any batch: the configuration is kept for hd_prepare
    run = PRunner(m, crf, crl)
    assert run.opt("preview") == 1
    x0, rows = run.preview()
    assert rows.tolist() == [-1, -1] and not bool(x0.any())
    _, ts, coef = _tables("ddim", 10)
    run.rows(x, ts, coef, [0, 2], 4)
    x0, rows = run.preview()
    assert rows.tolist() == [3, 5] and bool(x0[0].any()) and bool(x0[1].any())
    # begin_f = 0: snapshot s is row 2 (s + 1) - 1 of the table, wherever the face started -- face 1 (rows 2 .. 5) never ran row 1
    assert run.preview(0)[1].tolist() == [1, -1] and run.preview(1)[1].tolist() == [3, 3]
    assert not bool(run.preview(0)[0][1].any())
    only1, r1 = run.preview(slots=[1])
    assert r1.tolist() == [5] and torch.equal(only1[0], x0[1])
    swapped, rs = run.preview(slots=[1, 0])
    assert rs.tolist() == [5, 3] and torch.equal(swapped[0], x0[1]) and torch.equal(swapped[1], x0[0])
    rc, y, _ = run.read_rc(2, None, -1, with_rows=False)              # rows_out may be NULL
    assert rc == 0 and torch.equal(y, x0)
    for n, slots, snap in ((2, [0, 0], -1), (2, [0, 2], -1), (1, [-1], -1), (1, None, -1), (3, [0, 1, 1], -1), (0, [0], -1), (3, None, -1),
                           (2, None, 2), (2, None, -2)):
        rc, _, _ = run.read_rc(n, slots, snap)
        assert rc == ERR_INVALID and err(), (n, slots, snap, rc)
    assert run.preview()[1].tolist() == [3, 5]                        # still there: hd_sample* and failed reads reset nothing
    e.prepare_slots([1], crl[:1].cuda(), cr_face=crf[:1].cuda())      # resets slot 1 only
    x0b, rows = run.preview()
    assert rows.tolist() == [3, -1] and torch.equal(x0b[0], x0[0]) and not bool(x0b[1].any())
    assert run.preview(0)[1].tolist() == [1, -1] and run.preview(1)[1].tolist() == [3, -1] and not bool(run.preview(1)[0][1].any())
    e.prepare(crl.cuda(), cr_face=crf.cuda())                         # hd_prepare resets every face; the configuration survives
    x0, rows = run.preview()
    assert run.opt("preview") == 1 and rows.tolist() == [-1, -1] and not bool(x0.any())
    assert run.preview(1)[1].tolist() == [-1, -1]
    m.prepare(torch.cat([crf, crf]).cuda(), torch.cat([crl, crl]).cuda())     # another batch size: the planes follow it
    x0, rows = m.previews()
    assert tuple(x0.shape) == (4, 4, 16, 16) and rows.cpu().tolist() == [-1] * 4 and rows.dtype == torch.int32
    run.config(0)
    rc, _, _ = run.read_rc(4, None, -1)
    assert rc == ERR_NOT_READY and err()
    with pytest.raises(RuntimeError):
        m.previews()
    # a CoarseRestoration / VAE context has no sampling loop
    ctx = ctypes.c_void_p()
    _lib.check(_L().hd_vae_create(ctypes.byref(ctx), 0))
    assert _L().hd_preview_config(ctx, 1, 1, 0) == ERR_INVALID and _L().hd_last_error(ctx)
    _L().hd_destroy(ctx)
    ctx = ctypes.c_void_p()
    _lib.check(_L().hd_cr_create(ctypes.byref(ctx), 0))
    assert _L().hd_preview_config(ctx, 1, 1, 0) == ERR_INVALID and _L().hd_last_error(ctx)
    _L().hd_destroy(ctx)
    free(m)


# ------------------------------------------------------------------------------------------------ 9. the unconditional Denoiser
@pytest.mark.gpu
def test_unconditional_denoiser(gpu, weights16, data2):
    u = make_denoiser(weights16)
    run = PRunner(u, B=2)
    assert run.opt("end_fold") == 0                                   # ending_conv_kernel
    _check_neutral(run, data2[0])
    _check_last_row(run, data2[0])
    free(u)


# ------------------------------------------------------------------------------------------------ 10. latent 32
@pytest.mark.gpu
def test_latent32(gpu):
    from hifidiff_amd import synth
    m = make_model(synth.refiner_state_dict(32), 32)
    x, crl, crf = synth.sample_inputs(2, 32)
    run = PRunner(m, crf, crl)
    assert run.opt("end_fold") == 0                                   # the strip / wide program and the unfused ending
    _check_neutral(run, x)
    _check_last_row(run, x)
    free(m)


# ------------------------------------------------------------------------------------------------ 11. batch 64: the timed program's shape
@pytest.mark.gpu
def test_batch64_and_the_continuous_sampler(gpu, weights16):
    from hifidiff_amd import sampling, synth
    x, crl, crf = synth.sample_inputs(64, 16)
    m = make_model(weights16)
    run = PRunner(m, crf, crl)
    _check_last_row(run, x, kinds=("ddim",))
    # 6 requests over 4 slots, mixed strengths; every preview against the same request alone in a batch of 4, stopped after as many rows
    s, _, _ = _tables("ddpm", 10)
    strength = [1.0, 0.35, 0.6, 0.85, 0.5, 1.0]
    cs = sampling.ContinuousSampler(m, s, batch=4, refill_every=3, previews=True)
    ids = [cs.submit(crf[i], crl[i], seed=700 + i, strength=strength[i]) for i in range(6)]
    seen, refill_group = [], {}
    while cs.busy():
        before, queued = cs.refilled, [q[0] for q in cs.queue]
        cs.step()
        for rid in queued[:cs.refilled - before]:
            refill_group[rid] = cs.refilled - before                  # how many slots hd_prepare_slots refilled together with this one
        pr = cs.previews()
        t = cs.table
        assert sorted(pr) == sorted(t.req[i] for i in t.occupied() if not t.fresh[i])
        for slot in t.occupied():
            rid = t.req[slot]
            if rid in pr:                                             # rows_done is the SlotTable's: the slot's next row, counted from begin
                assert pr[rid][:2] == (t.row[slot] - t.begin[slot], t.end[slot] - t.begin[slot]), (rid, pr[rid][:2])
        seen.append({rid: (d, n, p.cpu()) for rid, (d, n, p) in pr.items()})
    assert sorted(cs.poll()) == ids
    assert refill_group == {4: 1, 5: 1}                               # requests 0 .. 3 came with hd_prepare(4), 4 and 5 each as a refill of one slot
    m.enable_previews(1, 0)
    checked = set()
    zf, zl = torch.zeros((4, 3, 128, 128), device="cuda"), torch.zeros((4, 4, 16, 16), device="cuda")
    for pr in seen:
        for rid, (done, total, x0) in pr.items():
            lat, start = cs._start(crl[rid], 700 + rid, strength[rid])
            assert total == 10 and start < done <= 10
            # alone: the other three slots empty (held), the request's conditioning computed as the sampler computed it -- with the first
            # batch of 4 (hd_prepare), or as a refill of one slot (hd_prepare_slots) -- and in another slot than it had there
            ff, fl = zf.clone(), zl.clone()
            if rid in refill_group:
                m.prepare(ff, fl)
                m.prepare_slots([3], crf[rid][None].cuda(), crl[rid][None].cuda())
            else:
                ff[3], fl[3] = crf[rid].cuda(), crl[rid].cuda()
                m.prepare(ff, fl)
            xa = zl.clone()
            xa[3] = lat.cuda()
            sampling.sample(m, xa, None, None, s, prepare=False, start_steps=[10, 10, 10, start], n_iters=done - start,
                            face_seeds=[0, 0, 0, 700 + rid])
            alone, row = m.previews()
            assert row.cpu().tolist() == [-1, -1, -1, done - 1]
            assert torch.equal(x0, alone[3].cpu()), (rid, done, float((x0 - alone[3].cpu()).abs().max()))
            checked.add(rid)
    assert checked == set(ids) - {1}                                  # request 1 (strength 0.35: 3 rows) finishes inside its first call
    free(m)
