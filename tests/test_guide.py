"""Low-pass fidelity guidance in the graph-replayed loop: hd_guide_config / hd_guide_faces, model.set_guidance, sampling.sample(guide=...)
and ContinuousSampler.submit(fidelity=...).

On a guided row the ending launch stores eps and leaves the face's latents alone; guided_update_kernel then forms x0, pulls it towards the
stored LP_N(target) -- x0g = x0 + w (LP_N(g) - LP_N(x0)) -- and runs the second half of the update on x0g.  Rows that are not guided run
the code they ran before, so everything that compares unguided rows, or the same guided arithmetic reached two ways (a window against
one-row calls, the shared against the per-face form, a face in a mixed batch against the batch that carries its setting everywhere), is
bit for bit.  Against the float64 formula the bound is GUIDE_TOL = 1e-5, as BLEND_TOL of tests/test_mask.py: a handful of fp32 roundings
on magnitudes <= 5 (the block sums of LP_N add less than that in any order).  As in tests/test_mask.py the bit-for-bit comparisons
between hd_sample and the per-face form run with "xcd2" off.

Measured on an MI355X (max abs from the float64 formula, worst of N in {1, 4, 16} x w in {0.3, 1.0}): DDIM row 20 of 50 (|x0| <= 3):
new latents 4.7e-07, preview 3.8e-07.  The two DPM-Solver++ 2M rows start from a latent at which the synthetic network's x0 has the
magnitude of a real one (_settled_latent): from pure noise |x0g| is 150 there and the stored x0g 1.4e-05 - 2.0e-05 (about one fp32 ulp)
from the formula, above the bound, while the new latents are within 4e-06."""
import ctypes
import math

import pytest
import torch

from conftest import rel_l2, weights16  # noqa: F401  (weights16: session fixture)
from test_mask import _L, _kn64, _tables, free, make_denoiser, make_model
from test_preview import PRunner, _i32, _set_table
from test_spans import _env

ERR_INVALID, ERR_NOT_READY = -1, -4
GUIDE_TOL = 1e-5                                  # a handful of fp32 roundings on magnitudes <= 5 (module docstring)
TRAJ_TOL = 1e-2                                   # tests/test_slots.py: a request in a batch against the same request alone
I32P = ctypes.POINTER(ctypes.c_int32)
F32P = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


class GRunner(PRunner):
    """tests/test_preview.py's Runner with the two guidance calls."""

    def guide_config(self, on):
        assert _L().hd_guide_config(self.ctx, on) == 0, _L().hd_last_error(self.ctx)
        assert self.opt("guide") == on

    def guide_rc(self, target, weight=None, scale=None, rows=None, slots=None, n=None):
        """hd_guide_faces; target None clears.  weight / scale: a number or a list per face; rows: None or (j0, j1) or a list of pairs."""
        sl = None if slots is None else _i32(slots)
        if n is None:
            n = sl.numel() if sl is not None else self.e.batch
        g = None if target is None else target.cuda().float().contiguous()
        per = lambda v, dt: None if v is None else (torch.as_tensor(v, dtype=dt).flatten().expand(n) if torch.as_tensor(v).numel() == 1  # noqa: E731
                                                    else torch.as_tensor(v, dtype=dt).flatten()).contiguous()
        w, N = per(weight, torch.float32), per(scale, torch.int32)
        r0 = r1 = None
        if rows is not None:
            r = torch.as_tensor(rows, dtype=torch.int32).reshape(-1, 2)
            r = r.expand(n, 2) if r.shape[0] == 1 else r
            r0, r1 = r[:, 0].contiguous(), r[:, 1].contiguous()
        p = lambda t, ty=I32P: None if t is None else ctypes.cast(t.data_ptr(), ty)  # noqa: E731
        rc = _L().hd_guide_faces(self.ctx, n, p(sl), None if g is None else g.data_ptr(), p(w, F32P), p(N), p(r0), p(r1),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def guide(self, target, weight, scale, rows=None, slots=None):
        assert self.guide_rc(target, weight, scale, rows, slots) == 0, _L().hd_last_error(self.ctx)

    def unguide(self, slots=None):
        assert self.guide_rc(None, slots=slots) == 0, _L().hd_last_error(self.ctx)

    def read_i32(self, name, n):
        return self.read(name, (n,)).view(torch.int32)


@pytest.fixture(scope="module")
def data(gpu):
    """B = 4 at latent 16: (x, crl, crf) and two targets that are not the coarse latent."""
    from hifidiff_amd import synth
    x, crl, crf = synth.sample_inputs(4, 16)
    g = torch.Generator().manual_seed(41)
    ga, gb = torch.randn((4, 4, 16, 16), generator=g), 0.5 * torch.randn((4, 4, 16, 16), generator=g) + 0.25
    return x, crl, crf, ga, gb


@pytest.fixture(scope="module")
def model4(gpu, weights16):
    m = make_model(weights16)
    yield m
    free(m)


@pytest.fixture(scope="module")
def run4(model4, data):
    """Batch 4 on the refiner, "xcd2" off, guidance switched on (the first test takes its baseline before that)."""
    x, crl, crf = data[:3]
    run = GRunner(model4, crf, crl)
    _L().hd_set_option(model4.engine.ctx, b"xcd2", 0)
    return run


def _lp64(t, N):
    """LP_N in float64, per face when N is a list."""
    from hifidiff_amd import sampling
    if isinstance(N, int):
        return sampling.low_pass(t.double(), N)
    return torch.stack([sampling.low_pass(t[f].double(), int(N[f])) for f in range(t.shape[0])])


def _guided64(x, eps, c, target, w, N, h=None, z=None, first=False):
    """The guided update of one row in float64 from the table's fp32 coefficients (c: 7 or 8 of them): returns (x', x0g)."""
    c = [float(v) for v in c] + ([0.0] if len(c) == 7 else [])
    x, eps = x.double(), eps.double()
    x0 = (x - c[0] * eps) / c[1]
    if math.isfinite(c[2]):
        x0 = x0.clamp(-c[2], c[2])
    wv = torch.as_tensor(w, dtype=torch.float64).reshape(-1, 1, 1, 1)
    x0g = x0 + wv * (_lp64(target, N) - _lp64(x0, N))
    e = (x - c[1] * x0g) / c[0] if c[5] != 0.0 else eps
    c3, c7 = (c[3] + c[7], 0.0) if first else (c[3], c[7])
    r = c3 * x0g + c[4] * x + c[5] * e
    if c[6] != 0.0:
        r = r + c[6] * z.double()
    if c7 != 0.0:
        r = r + c7 * h.double()
    return r, x0g


def _shape(x):
    return tuple(x.shape)


# ------------------------------------------------------------------------------------------------ 1. the unguided path is untouched
@pytest.mark.gpu
def test_unguided_path_is_untouched(run4, data):
    x, crl, _, ga, _ = data
    _, ts, coef = _tables("ddim", 50)
    rows = [0, 7, 25, 49]
    assert run4.opt("guide") == 0 and run4.opt("guided_faces") == 0
    base, base_rows = run4.full(x, ts, coef), run4.rows(x, ts, coef, rows, 50)
    ops = _L().hd_num_ops(run4.ctx, 0)
    # on, every face guided, cleared, off: the bits of a context that never had it on
    run4.guide_config(1)
    run4.guide(crl, 0.5, 4)
    assert run4.opt("guided_faces") == 4
    run4.unguide()
    assert run4.opt("guided_faces") == 0
    run4.guide_config(0)
    assert torch.equal(run4.full(x, ts, coef), base) and torch.equal(run4.rows(x, ts, coef, rows, 50), base_rows)
    # on, nobody guided: still those bits, through the step that ends with the guided launch
    run4.guide_config(1)
    assert torch.equal(run4.full(x, ts, coef), base) and torch.equal(run4.rows(x, ts, coef, rows, 50), base_rows)
    captures = run4.opt("graph_captures")
    # faces 0 and 1 guided: faces 2 and 3 keep their bits, and setting / changing / clearing faces captures nothing
    run4.guide(ga[:2], [0.3, 1.0], [4, 16], slots=[0, 1])
    assert run4.opt("guided_faces") == 2
    part, part_rows = run4.full(x, ts, coef), run4.rows(x, ts, coef, rows, 50)
    assert torch.equal(part[2:], base[2:]) and torch.equal(part_rows[2:], base_rows[2:])
    assert not torch.equal(part[0], base[0]) and not torch.equal(part[1], base[1])
    assert not torch.equal(part_rows[0], base_rows[0]) and not torch.equal(part_rows[1], base_rows[1])
    assert torch.equal(part_rows[3], base_rows[3])                    # (a face that runs one row only)
    run4.guide(crl, 1.0, 1, rows=(3, 9))
    run4.unguide(slots=[2])
    assert run4.opt("guided_faces") == 3
    run4.full(x, ts, coef)
    run4.unguide()
    assert torch.equal(run4.full(x, ts, coef), base) and torch.equal(run4.rows(x, ts, coef, rows, 50), base_rows)
    assert run4.opt("graph_captures") == captures, (run4.opt("graph_captures"), captures)
    assert _L().hd_num_ops(run4.ctx, 0) == ops
    run4.guide_config(0)
    assert torch.equal(run4.full(x, ts, coef), base) and torch.equal(run4.rows(x, ts, coef, rows, 50), base_rows)
    run4.guide_config(1)                                              # the module's other tests run with it on


# ------------------------------------------------------------------------------------------------ 2. one guided row against the float64 formula
def _settled_latent(run, x, y, kind, n, k, iters=10):
    """A latent for row k whose own denoised estimate is about y (|y| <= 3), as a trained network's would be.  The synthetic network is no
    noise estimator: from the module's pure-noise x its x0 = (x - c0 eps)/c1 of a high-noise row (c1 = 0.03 on row 0 of DPM-20) reaches 150,
    where one fp32 ulp is 1.5e-5 and GUIDE_TOL's premise (magnitudes <= 5) does not hold for the stored x0g.  x <- c0 eps(x) + c1 y, one
    unguided row of the device per iteration, settles in under ten (measured: |x0| 151 -> 37 -> 11 -> 5.5 -> 4.0 -> 3.0 -> 2.8)."""
    B = x.shape[0]
    _, ts, coef = _tables(kind, n)
    c0, c1 = float(coef[k, 0]), float(coef[k, 1])
    xi = x.float()
    for _ in range(iters):
        run.rows(xi, ts, coef, [k] * B, 1)
        xi = (c0 * run.read("eps", _shape(x)).double() + c1 * y.double()).float()
    return xi


def _check_row(run, x, target, kind, n, k, resume=0, lead=0, settle=None):
    """Row k (per-face form, n_iters = 1) for N in {1, 4, L} x w in {0.3, 1.0} against _guided64 on the device's own eps; then the history
    (multistep) and the preview plane against the float64 x0g.  lead > 0: the `lead` rows before k run first in the same guided loop and
    row k resumes their history.  settle: row k itself starts from _settled_latent(.., y = settle) instead (the lead still runs from x and
    leaves its history).  Returns the worst error per quantity: {"x", "x0_hist" (multistep), "preview"}, and "|x0g|", the largest magnitude."""
    B, L = x.shape[0], x.shape[-1]
    _, ts, coef = _tables(kind, n)
    ms = coef.shape[1] == 8
    worst = {}
    xs = None if settle is None else _settled_latent(run, x, settle, kind, n, k)
    run.config(1)
    try:
        for N in (1, 4, L):
            for w in (0.3, 1.0):
                run.guide(target, w, N)
                xk, h = x.float(), None
                if lead:
                    xk = run.rows(x, ts, coef, [k - lead] * B, lead)
                    h = run.read("x0_hist", _shape(x))
                if xs is not None:
                    xk = xs
                got = run.rows(xk, ts, coef, [k] * B, 1, resume=resume)
                eps = run.read("eps", _shape(x))
                want, x0g = _guided64(xk, eps, coef[k], target, w, N, h=h, first=ms and not resume)
                errs = {"x": float((got.double() - want).abs().max())}
                if ms:
                    errs["x0_hist"] = float((run.read("x0_hist", _shape(x)).double() - x0g).abs().max())
                pv, pv_rows = run.preview()
                assert pv_rows.tolist() == [k] * B
                errs["preview"] = float((pv.double() - x0g).abs().max())
                print(f"guided {kind} row {k} of {n}, L = {L}, N = {N}, w = {w}: max abs from the float64 formula " +
                      ", ".join(f"{a} {b:.3e}" for a, b in errs.items()) + f"   (max |x0g| {float(x0g.abs().max()):.2f})")
                worst = {a: max(b, worst.get(a, 0.0)) for a, b in {**errs, "|x0g|": float(x0g.abs().max())}.items()}
                assert float((got.double() - xk.double()).abs().max()) > 1e-3          # the row did run
    finally:
        run.unguide()
        run.config(0)
    return worst


@pytest.mark.gpu
def test_one_guided_row_ddim_middle_row(run4, data):
    """DDIM, clip 3.0, 50 steps, row 20: c1 <= c0 and c5 != 0, so eps is re-derived from x0g with |x0| <= 3."""
    x, crl = data[0], data[1]
    _, _, coef = _tables("ddim", 50)
    assert float(coef[20, 1]) <= float(coef[20, 0]) and float(coef[20, 5]) != 0.0 and float(coef[20, 2]) == 3.0
    worst = _check_row(run4, x, crl, "ddim", 50, 20)
    assert max(worst["x"], worst["preview"]) <= GUIDE_TOL and worst["|x0g|"] <= 5.0, worst


@pytest.mark.gpu
def test_one_guided_row_dpm_row_0(run4, data):
    """DPM-Solver++ 2M, 20 steps, row 0: first-order (c7 folded into c3), no clamp.  The row starts from a latent whose own x0 is about
    the second target of the module (_settled_latent), so that the magnitudes are those the bound is reasoned for.  From the module's
    pure-noise x the new latents were within 4.2e-07 but the stored x0g, at |x0g| = 149, 1.98e-05 (1.3 fp32 ulp) from the formula."""
    x, crl, gb = data[0], data[1], data[4]
    worst = _check_row(run4, x, crl, "dpm", 20, 0, settle=gb.clamp(-3.0, 3.0))
    assert max(worst["x"], worst["x0_hist"], worst["preview"]) <= GUIDE_TOL, worst
    assert worst["|x0g|"] <= 5.0, worst                                # the premise of the bound


@pytest.mark.gpu
def test_one_guided_row_dpm_row_5_resumed(run4, data):
    """Row 5 with resume = 1 after five guided rows from x: the history term c7*h with h the x0g of row 4, read from the device (at
    |h| = 150 and c7 = -0.03 its fp32 product is good to 3e-07).  Row 5 itself starts from a settled latent, as row 0 does above.  From
    the lead's own output the new latents were within 3.9e-06 but the stored x0g, at |x0g| = 158, 1.37e-05 from the formula."""
    x, crl, gb = data[0], data[1], data[4]
    _, _, coef = _tables("dpm", 20)
    assert float(coef[5, 7]) != 0.0
    worst = _check_row(run4, x, crl, "dpm", 20, 5, resume=1, lead=5, settle=gb.clamp(-3.0, 3.0))
    assert max(worst["x"], worst["x0_hist"], worst["preview"]) <= GUIDE_TOL, worst
    assert worst["|x0g|"] <= 5.0, worst


# ------------------------------------------------------------------------------------------------ 3. the row window composes bit for bit
def _check_window(run, x, target, kind, n, w=0.5, N=4, window=(2, 5), iters=8):
    """A guided loop with a row window against the same rows rebuilt from one-row calls: unguided calls outside the window, calls guided on
    all rows inside it; the multistep form steps with resume = 1, so the history has to be x0g on guided rows and x0 on the others."""
    B = x.shape[0]
    _, ts, coef = _tables(kind, n)
    try:
        run.guide(target, w, N, rows=window)
        loop = [run.rows(x, ts, coef, [0] * B, i + 1) for i in range(iters)]
        run.unguide()
        plain = run.rows(x, ts, coef, [0] * B, iters)
        xi = x.float()
        for i in range(iters):
            if window[0] <= i < window[1]:
                run.guide(target, w, N)
            else:
                run.unguide()
            xi = run.rows(xi, ts, coef, [i] * B, 1, resume=int(i > 0))
            assert torch.equal(xi, loop[i]), (kind, i, float((xi - loop[i]).abs().max()))
    finally:
        run.unguide()
    assert not torch.equal(loop[-1], plain)                           # the window did something
    return loop[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("ddim", 50), ("dpm", 20)])
def test_row_window_composes_with_one_row_calls(run4, data, kind, n):
    x, crl = data[0], data[1]
    assert run4.opt("end_fold") == 1                                  # the fused ending launch (hca_ending_conv_kernel)
    _check_window(run4, x, crl, kind, n)


@pytest.mark.gpu
def test_row_window_composes_on_the_unconditional_denoiser(gpu, weights16, data):
    x, crl = data[0], data[1]
    u = make_denoiser(weights16)
    run = GRunner(u, B=4)
    _L().hd_set_option(u.engine.ctx, b"xcd2", 0)
    run.guide_config(1)
    assert run.opt("end_fold") == 0                                   # ending_conv_kernel
    _check_window(run, x, crl, "ddim", 20)
    _check_window(run, x, crl, "dpm", 20, w=1.0, N=16)
    free(u)


@pytest.mark.gpu
def test_row_window_counts_rows_from_the_span(run4, data):
    """A ScheduleSet table (DDIM-4 in rows [0, 4), DPM-8 in rows [4, 12)): faces 0 and 1 run the first member and are held after it, faces 2
    and 3 the second, whose begin is 4 -- the window [2, 5) is rows 6 .. 8 of the table for them (j = k - begin_f)."""
    x, crl = data[0], data[1]
    _, ts, coef = _set_table()
    begin, end = [0, 0, 4, 4], [4, 4, 12, 12]
    at = lambda i: [min(i, 4), min(i, 4), 4 + i, 4 + i]  # noqa: E731
    try:
        run4.guide(crl, 0.5, 4, rows=(2, 5))
        loop = [run4.spans(x, ts, coef, begin, end, at(0), i + 1, [0] * 4) for i in range(8)]
        run4.unguide()
        plain = run4.spans(x, ts, coef, begin, end, at(0), 8, [0] * 4)
        xi = x.float()
        for i in range(8):
            if 2 <= i < 5:
                run4.guide(crl, 0.5, 4)
            else:
                run4.unguide()
            xi = run4.spans(xi, ts, coef, begin, end, at(i), 1, [int(0 < i < 4), int(0 < i < 4), int(i > 0), int(i > 0)])
            assert torch.equal(xi, loop[i]), (i, float((xi - loop[i]).abs().max()))
    finally:
        run4.unguide()
    assert not torch.equal(loop[-1][:2], plain[:2]) and not torch.equal(loop[-1][2:], plain[2:])
    assert torch.equal(loop[1], run4.spans(x, ts, coef, begin, end, at(0), 2, [0] * 4))      # rows 0 and 1 of a span are not guided


# ------------------------------------------------------------------------------------------------ 4. the shared and the per-face forms agree
@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("ddim", 10), ("dpm", 10), ("ddpm", 10)])
def test_shared_and_per_face_forms_agree(run4, data, kind, n):
    x, _, _, ga, _ = data
    _, ts, coef = _tables(kind, n)
    kw = {"seed": 11} if kind == "ddpm" else {}
    assert run4.opt("xcd2") == 0
    try:
        run4.guide(ga, [0.3, 1.0, 0.5, 0.7], [1, 4, 16, 8], rows=[(0, 10), (2, 5), (0, 3), (9, 10)])
        a, b = run4.full(x, ts, coef, **kw), run4.rows(x, ts, coef, [0] * 4, n, **kw)
    finally:
        run4.unguide()
    assert torch.equal(a, b), (kind, float((a - b).abs().max()))
    assert not torch.equal(a, run4.full(x, ts, coef, **kw))


# ------------------------------------------------------------------------------------------------ 5. the DC property
@pytest.mark.gpu
def test_full_weight_at_plane_scale_fixes_the_channel_means(run4, data):
    """2M, 10 steps, w = 1, N = L on every row: the last row lands on x0g (c3 = 1, the rest 0), whose plane means are the target's."""
    x, _, _, ga, _ = data
    _, ts, coef = _tables("dpm", 10)
    assert float(coef[9, 3]) == 1.0 and all(float(v) == 0.0 for v in coef[9, 4:])
    try:
        run4.guide(ga, 1.0, 16)
        got = run4.full(x, ts, coef)
    finally:
        run4.unguide()
    err = float((got.double().mean(dim=(2, 3)) - ga.double().mean(dim=(2, 3))).abs().max())
    free_run = float((run4.full(x, ts, coef).double().mean(dim=(2, 3)) - ga.double().mean(dim=(2, 3))).abs().max())
    print(f"channel means after 10 guided 2M rows (w = 1, N = L): max abs {err:.3e} from the target's (unguided: {free_run:.3e})")
    assert err <= 1e-5, err
    assert free_run > 1e-3


# ------------------------------------------------------------------------------------------------ 6. against the oracle network
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dpm", "ddim"])
def test_against_the_oracle_network(gpu, weights16, model4, data, kind):
    """The loops of tests/test_multistep.py and tests/test_mask.py (B = 2, 10 steps, the oracle network with bf16 operands) with the
    guided update applied in float64: w = 0.5, N = 4, rows [0, 8)."""
    from hifidiff_amd import sampling, synth
    from oracle import hifidiff_oracle as O
    from test_multistep import _update64
    x, crl, crf = synth.sample_inputs(2, 16)
    s, _, _ = _tables(kind, 10)
    ts, coef = s.coefficient_table()
    cond = O.Conditioning(weights16, crl, crf, prec=O.BF16)
    xr, h = x.double(), None
    for i, t in enumerate(s.timesteps.tolist()):
        eps = O.fused_denoiser(weights16, xr.float(), torch.full((x.shape[0],), t), prec=O.BF16, cond=cond).double()
        if i < 8:
            xr, h = _guided64(xr, eps, coef[i], crl, 0.5, 4, h=h)
        else:
            xr, h = _update64(xr, eps, [float(v) for v in coef[i]] + [0.0] * (8 - coef.shape[1]), h)
    got = sampling.sample(model4, x.cuda(), crf.cuda(), crl.cuda(), s, guide=crl, guide_weight=0.5, guide_scale=4, guide_rows=(0, 8)).cpu()
    r = rel_l2(got, xr)
    print(f"guided {kind}, 10 steps, w = 0.5, N = 4, rows [0, 8), against the oracle network: rel-L2 {r:.3e}")
    assert r <= 2e-2, r
    model4.prepare(data[2].cuda(), data[1].cuda())                    # the batch of the module's other tests (a prepare clears the guidance)


# ------------------------------------------------------------------------------------------------ 7. per face, and the lifetime
@pytest.mark.gpu
def test_guidance_is_per_face(run4, data):
    from hifidiff_amd import sampling
    x, _, _, ga, gb = data
    _, ts, coef = _tables("dpm", 10)
    try:
        run4.guide(ga[:2], 0.3, 2, slots=[0, 1])
        run4.guide(gb[2:], 1.0, 8, rows=(1, 7), slots=[3, 2])         # slot 3 gets gb[2], slot 2 gets gb[3]
        assert run4.opt("guided_faces") == 4
        mixed = run4.rows(x, ts, coef, [0] * 4, 10)
        lp = run4.read("guide_lp", (4, 4, 16, 16))
        want = torch.cat([sampling.low_pass(ga[:2].double(), 2), sampling.low_pass(gb[[3, 2]].double(), 8)])
        err = float((lp.double() - want).abs().max())
        print(f"guide_lp against sampling.low_pass in float64: max abs {err:.3e}")
        assert err <= 1e-6, err
        assert run4.read("guide_weight", (4,)).tolist() == [pytest.approx(0.3), pytest.approx(0.3), 1.0, 1.0]
        assert run4.read_i32("guide_scale", 4).tolist() == [2, 2, 8, 8]
        run4.guide(ga, 0.3, 2)
        all_a = run4.rows(x, ts, coef, [0] * 4, 10)
        run4.guide(torch.cat([gb[:2], gb[[3, 2]]]), 1.0, 8, rows=(1, 7))
        all_b = run4.rows(x, ts, coef, [0] * 4, 10)
    finally:
        run4.unguide()
    assert torch.equal(mixed[:2], all_a[:2]) and torch.equal(mixed[2:], all_b[2:])
    assert not torch.equal(mixed[:2], all_b[:2]) and not torch.equal(mixed[2:], all_a[2:])
    assert run4.read("guide_weight", (4,)).tolist() == [0.0] * 4


@pytest.mark.gpu
def test_guidance_lifetime(run4, data):
    from hifidiff_amd import sampling
    x, crl, crf, ga, _ = data
    m, e = run4.m, run4.e
    run4.guide(ga, 0.5, 4)
    assert run4.opt("guided_faces") == 4
    e.prepare_slots([1, 3], crl[:2].cuda(), cr_face=crf[:2].cuda())   # clears the refilled slots only
    assert run4.opt("guided_faces") == 2
    assert run4.read("guide_weight", (4,)).tolist() == [0.5, 0.0, 0.5, 0.0]
    e.prepare(crl.cuda(), cr_face=crf.cuda())                         # hd_prepare clears every face
    assert run4.opt("guided_faces") == 0 and run4.opt("guide") == 1
    assert run4.read("guide_weight", (4,)).tolist() == [0.0] * 4
    # the Python calls on the same conditioning tensors: the cache hits, hd_prepare does not run, and the guidance must still be gone
    s, _, _ = _tables("dpm", 10)
    xd, crfd, crld = x.cuda(), crf.cuda(), crl.cuda()
    never = sampling.sample(m, xd, crfd, crld, s).cpu()
    guided = sampling.sample(m, xd, crfd, crld, s, guide=ga, guide_weight=0.5, guide_scale=4).cpu()
    assert run4.opt("guided_faces") == 4 and not torch.equal(guided, never)
    assert e.cond_key is not None                                     # the next call hits the cache
    again = sampling.sample(m, xd, crfd, crld, s).cpu()
    assert run4.opt("guided_faces") == 0
    assert torch.equal(again, never)
    # a loop split over calls with prepare=False keeps the guidance
    kw = dict(guide=ga, guide_weight=torch.tensor([0.3, 1.0, 0.5, 0.7]), guide_scale=torch.tensor([1, 4, 16, 8]), guide_rows=(2, 9))
    one = sampling.sample(m, xd, crfd, crld, s, start_steps=0, **kw).cpu()
    y = sampling.sample(m, xd, crfd, crld, s, start_steps=0, n_iters=4, **kw)
    y = sampling.sample(m, y, None, None, s, prepare=False, start_steps=4, n_iters=6, resume=True).cpu()
    assert run4.opt("guided_faces") == 4 and torch.equal(y, one)
    assert not torch.equal(one, never)
    m.clear_guidance(slots=[0])
    assert run4.opt("guided_faces") == 3
    m.clear_guidance()
    assert run4.opt("guided_faces") == 0
    m.disable_guidance()
    assert run4.opt("guide") == 0 and torch.equal(sampling.sample(m, xd, crfd, crld, s).cpu(), never)
    m.set_guidance(ga, 0.5, 4)                                        # switches it on again by itself
    assert run4.opt("guide") == 1 and run4.opt("guided_faces") == 4
    assert torch.equal(sampling.sample(m, xd, None, None, s, prepare=False).cpu(), guided)
    m.clear_guidance()


# ------------------------------------------------------------------------------------------------ 8. with a mask and previews
@pytest.mark.gpu
def test_guided_row_with_a_soft_mask_and_previews(run4, data):
    from hifidiff_amd import sampling
    x, crl, _, ga, _ = data
    m1 = sampling.region_mask([(24, 16, 104, 96)], 16, feather=2)
    assert bool(((m1 > 0) & (m1 < 1)).any())
    mask = m1[None].expand(4, 16, 16).contiguous()
    md = mask[:, None].double()
    run4.config(1)
    try:
        for kind, k in (("ddim", 4), ("dpm", 0)):
            _, ts, coef = _tables(kind, 20)
            run4.mask(mask, crl, x)
            run4.guide(ga, 0.5, 4)
            got = run4.rows(x, ts, coef, [k] * 4, 1)
            eps = run4.read("eps", (4, 4, 16, 16))
            r, x0g = _guided64(x, eps, coef[k], ga, 0.5, 4, first=True)
            want = md * r + (1.0 - md) * _kn64(coef, k + 1, crl, x)
            pv, _ = run4.preview()
            e1 = float((got.double() - want).abs().max())
            e2 = float((pv.double() - (md * x0g + (1.0 - md) * crl.double())).abs().max())
            print(f"guided + soft mask + preview, one {kind} row: blend {e1:.3e}, preview {e2:.3e} from the float64 formula")
            assert e1 <= GUIDE_TOL and e2 <= GUIDE_TOL, (kind, e1, e2)
    finally:
        run4.unguide()
        run4.clear()
        run4.config(0)


# ------------------------------------------------------------------------------------------------ 9. continuous batching
@pytest.mark.gpu
def test_continuous_sampler_with_fidelity(run4, data):
    """16 requests through 4 slots, every other one guided towards its own coarse latent (weights, scales, windows and strengths mixed):
    each result against the same request sampled alone, within TRAJ_TOL as tests/test_slots.py compares a request of a batch with the
    request alone (the conditioning of a refill is computed at another batch size)."""
    from hifidiff_amd import sampling, synth
    _, crl, crf = synth.sample_inputs(16, 16)
    s, _, _ = _tables("ddpm", 10)
    n_req = 16
    strength = [(1.0, 0.35, 0.6, 0.85)[i % 4] for i in range(n_req)]
    fid = [None if i % 2 else ((0.3, 4, None), (1.0, 16, (0, 6)), (0.7, 1, (2, 10)), (0.5, 8, None))[(i // 2) % 4] for i in range(n_req)]
    m = run4.m
    cs = sampling.ContinuousSampler(m, s, batch=4, refill_every=3)
    ids = []
    for i in range(n_req):
        kw = {} if fid[i] is None else dict(fidelity=fid[i][0], fidelity_scale=fid[i][1], fidelity_rows=fid[i][2])
        ids.append(cs.submit(crf[i], crl[i], seed=500 + i, strength=strength[i], **kw))
    out = cs.drain()
    assert sorted(out) == ids and cs.refilled >= n_req - 4
    worst, exact, moved = 0.0, 0, 0.0
    for i in ids:
        lat, start = cs._start(crl[i], 500 + i, strength[i])
        args = (m, lat[None].cuda(), crf[i][None].cuda(), crl[i][None].cuda(), s)
        kw = {} if fid[i] is None else dict(guide=crl[i][None], guide_weight=fid[i][0], guide_scale=fid[i][1], guide_rows=fid[i][2])
        got = sampling.sample(*args, start_steps=start, face_seeds=[500 + i], **kw)[0].cpu()
        r = rel_l2(out[i].cpu(), got)
        worst, exact = max(worst, r), exact + int(torch.equal(out[i].cpu(), got))
        if fid[i] is not None:
            moved = max(moved, rel_l2(sampling.sample(*args, start_steps=start, face_seeds=[500 + i])[0].cpu(), got))
    print(f"ContinuousSampler with fidelity vs each request alone: {exact}/{n_req} bit-identical, worst rel-L2 {worst:.2e} "
          f"(guided vs unguided, alone: up to {moved:.2e})")
    assert worst <= TRAJ_TOL, worst
    assert moved > TRAJ_TOL                                           # the guidance is not lost in the tolerance
    m.prepare(data[2].cuda(), data[1].cuda())                         # the batch of the module's other tests
    run4.guide_config(1)


# ------------------------------------------------------------------------------------------------ 10. argument checks through the C-ABI
@pytest.mark.gpu
def test_argument_checks(gpu, weights16):
    from hifidiff_amd import synth
    m = make_model(weights16)
    e = m.engine
    x, crl, crf = synth.sample_inputs(2, 16)
    gd = crl.cuda().contiguous()
    s = torch.cuda.current_stream().cuda_stream
    err = lambda: _L().hd_last_error(e.ctx)  # noqa: E731
    f32 = lambda *v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    sl = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    p = lambda t, ty=I32P: None if t is None else ctypes.cast(t.data_ptr(), ty)  # noqa: E731
    call = lambda n, slots, g, w, N, r0=None, r1=None: _L().hd_guide_faces(  # noqa: E731
        e.ctx, n, p(slots), g.data_ptr() if g is not None else None, p(w, F32P), p(N), p(r0), p(r1), s)
    assert _L().hd_guide_config(e.ctx, 1) == 0
    assert call(2, None, gd, f32(0.5, 0.5), sl(4, 4)) == ERR_NOT_READY and err()
    assert _L().hd_guide_config(e.ctx, 0) == 0
    run = GRunner(m, crf, crl)
    _, ts, coef = _tables("ddim", 10)
    ok_w, ok_n = f32(0.5, 0.5), sl(4, 4)
    assert call(2, None, gd, ok_w, ok_n) == ERR_INVALID and err()     # a target while the config is off
    assert run.opt("guided_faces") == 0 and bool(torch.isfinite(run.full(x, ts, coef)).all())
    assert _L().hd_guide_config(e.ctx, 2) == ERR_INVALID and err()
    run.guide_config(1)
    bad = [(2, sl(0, 0), ok_w, ok_n, None, None), (2, sl(0, 2), ok_w, ok_n, None, None), (1, sl(-1), ok_w, ok_n, None, None),
           (1, None, ok_w, ok_n, None, None), (3, sl(0, 1, 1), ok_w, ok_n, None, None), (0, sl(0), ok_w, ok_n, None, None),
           (2, None, f32(0.5, 0.0), ok_n, None, None),                # weight 0
           (2, None, f32(1.5, 0.5), ok_n, None, None),                # weight 1.5
           (2, None, f32(0.5, float("nan")), ok_n, None, None),       # weight NaN
           (2, None, f32(float("inf"), 0.5), ok_n, None, None),
           (2, None, f32(-0.5, 0.5), ok_n, None, None),
           (2, None, ok_w, sl(4, 3), None, None),                     # N = 3 at L = 16
           (2, None, ok_w, sl(0, 4), None, None), (2, None, ok_w, sl(4, 32), None, None),
           (2, None, ok_w, ok_n, sl(0, 3), sl(4, 3)),                 # row_from >= row_to
           (2, None, ok_w, ok_n, sl(5, 0), sl(2, 4)), (2, None, ok_w, ok_n, sl(-1, 0), sl(2, 4)),
           (2, None, ok_w, ok_n, sl(0, 0), None), (2, None, ok_w, ok_n, None, sl(4, 4)),
           (2, None, None, ok_n, None, None), (2, None, ok_w, None, None, None)]
    for n, slots, w, N, r0, r1 in bad:
        rc = call(n, slots, gd, w, N, r0, r1)
        assert rc == ERR_INVALID and err(), (n, slots, w, N, r0, r1, rc)
        assert run.opt("guided_faces") == 0
        assert bool(torch.isfinite(run.full(x, ts, coef)).all())      # the context is still usable
    base = run.full(x, ts, coef)
    assert call(1, sl(1), gd, f32(1.0), sl(16), sl(0), sl(10)) == 0
    torch.cuda.synchronize()
    assert run.opt("guided_faces") == 1
    out = run.full(x, ts, coef)
    assert torch.equal(out[0], base[0]) and not torch.equal(out[1], base[1])
    dc = float((out[1].double().mean(dim=(1, 2)) - crl[0].double().mean(dim=(1, 2))).abs().max())
    assert dc <= 1e-5, dc                                             # slot 1 carries face 0 of the call's tensors
    assert call(1, sl(1), None, None, None) == 0 and run.opt("guided_faces") == 0
    assert call(2, None, None, None, None) == 0                       # nothing to clear
    free(m)


# ------------------------------------------------------------------------------------------------ 11. latent 32, and two chains
@pytest.mark.gpu
def test_latent32(gpu):
    from hifidiff_amd import synth
    m = make_model(synth.refiner_state_dict(32), 32)
    x, crl, crf = synth.sample_inputs(2, 32)
    run = GRunner(m, crf, crl)
    _L().hd_set_option(m.engine.ctx, b"xcd2", 0)
    run.guide_config(1)
    _, ts, coef = _tables("ddim", 10)
    run.config(1)
    try:
        worst = 0.0
        for k in (4, 9):
            run.guide(crl, 0.5, 8)
            got = run.rows(x, ts, coef, [k] * 2, 1)
            eps = run.read("eps", (2, 4, 32, 32))
            want, x0g = _guided64(x, eps, coef[k], crl, 0.5, 8)
            pv, _ = run.preview()
            e1, e2 = float((got.double() - want).abs().max()), float((pv.double() - x0g).abs().max())
            print(f"guided ddim row {k} of 10, L = 32, N = 8, w = 0.5: max abs from the float64 formula x {e1:.3e}, preview {e2:.3e}")
            worst = max(worst, e1, e2)
        assert worst <= GUIDE_TOL, worst
    finally:
        run.unguide()
        run.config(0)
    _check_window(run, x, crl, "ddim", 10, w=0.5, N=8)
    free(m)


@pytest.mark.gpu
def test_two_chains(gpu, weights16, data):
    """Face indices are chain-local and noise indices batch-global: B = 4 as two chains of two faces, every face with its own setting, one
    guided DDPM row (device Philox) against the float64 formula with z taken from the unguided row, and the window against one-row calls."""
    x, crl, crf, ga, _ = data
    with _env({"HD_EXPERIMENTS": "1", "HD_CHAINS": "2"}):
        m = make_model(weights16)
        run = GRunner(m, crf, crl)
        assert _L().hd_num_chains(run.ctx) == 2
        _L().hd_set_option(m.engine.ctx, b"xcd2", 0)
        run.guide_config(1)
        _, ts, coef = _tables("ddpm", 10)
        k, w, N = 3, [0.3, 1.0, 0.5, 0.7], [1, 4, 16, 8]
        plain = run.rows(x, ts, coef, [k] * 4, 1, seed=11)
        eps = run.read("eps", (4, 4, 16, 16))
        c = [float(v) for v in coef[k]]
        x0 = ((x.double() - c[0] * eps.double()) / c[1]).clamp(-c[2], c[2])
        z = (plain.double() - c[3] * x0 - c[4] * x.double() - c[5] * eps.double()) / c[6]      # the row's z as the device drew it
        run.guide(ga, w, N)
        got = run.rows(x, ts, coef, [k] * 4, 1, seed=11)
        assert torch.equal(run.read("eps", (4, 4, 16, 16)), eps)
        want, _ = _guided64(x, eps, coef[k], ga, w, N, z=z)
        err = float((got.double() - want).abs().max())
        print(f"two chains, guided ddpm row {k}: max abs {err:.3e} from the float64 formula")
        assert err <= 2 * GUIDE_TOL, err                              # (z itself is recovered from fp32 values: one more term of the same size)
        run.unguide()
        _check_window(run, x, crl, "dpm", 10)
        free(m)
