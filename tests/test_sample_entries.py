"""The seven sampling-loop entry points on ONE context, one after the other, at batch 2 and then at batch 3 (latent 16).

They share the library's call path: the pinned staging buffer, the per-face argument block (which grows at batch 3 while the batch-2
workspace is parked), the FiLM table, and the plain / per-face graph pairs.  Every result must be bit for bit what the same call gives
on a context that has made no other call, and the shared context must have captured exactly the graphs that one plain and one per-face
call per batch size need.  The two-chain form (HD_CHAINS=2, as tests/test_spans.py::test_variant_two_chains) repeats it at batch 4: the
second chain reads the per-face arrays at its face offset.

Tables: DDPM and SDE-DPM-Solver++ 2M, 3 rows each, z from device Philox; hd_sample_spans runs their concatenation with the faces
alternating between the two members.  It is called first: its 6-row table sizes the FiLM table before any graph is captured."""
import ctypes

import pytest
import torch

from conftest import weights16  # noqa: F401  (session fixture)
from test_spans import Ctx, _L, _env, _i32, _sched, free, make_model

ENTRIES = ("hd_sample_spans", "hd_sample", "hd_sample_multistep", "hd_sample_rows", "hd_sample_rows_multistep", "hd_sample_faces",
           "hd_sample_faces_multistep")
TWO_CHAINS = {"HD_EXPERIMENTS": "1", "HD_CHAINS": "2"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def data(gpu):
    from hifidiff_amd import synth
    return synth.sample_inputs(4, 16)


def _tables():
    from hifidiff_amd.sampling import ScheduleSet
    ddpm, sde = _sched("ddpm", 3), _sched("sde", 3)
    return ddpm.coefficient_table(), sde.coefficient_table(), ScheduleSet({"ddpm": ddpm, "sde": sde})


def _call(c, entry, x, tab=None):
    """One call of `entry` on the prepared batch of context c: staggered start rows (face 2 is past its last row: held), per-face keys.
    tab: a 7-column table for the single-step entry points in place of the DDPM one."""
    B = x.shape[0]
    ddpm, sde, sset = _tables()
    ddpm = tab or ddpm
    rows = [0, 1, 3, 2][:B]
    seeds = [11 + f for f in range(B)]
    if entry == "hd_sample_spans":
        spans = [sset.span(("ddpm", "sde")[f % 2]) for f in range(B)]
        begin, end = [b for b, _ in spans], [e for _, e in spans]
        return c.spans(x, sset.coefficient_table(), begin, end, [b + r for b, r in zip(begin, rows)], 3, seeds=seeds, seed=5)
    if entry.startswith("hd_sample_faces"):
        return c.faces(x, sde if entry.endswith("multistep") else ddpm, rows, 3, seeds=seeds, seed=5)
    ts, coef = sde if entry.endswith("multistep") else ddpm
    xd = x.cuda().float().contiguous().clone()
    sch = c.sch(ts, coef)
    _r, rp = _i32(rows)
    s = torch.cuda.current_stream().cuda_stream
    head = (c.ctx, xd.data_ptr(), ctypes.byref(sch))
    if entry in ("hd_sample", "hd_sample_multistep"):
        rc = getattr(_L(), entry)(*head, None, 5, s)
    elif entry == "hd_sample_rows":
        rc = _L().hd_sample_rows(*head, rp, 3, None, 5, s)
    else:
        rc = _L().hd_sample_rows_multistep(*head, rp, 3, 0, None, 5, s)
    return c.done((rc, xd))


def _fresh(weights, data, B, entry, env=None):
    """(result, graph_captures) of `entry` at batch B on a context that makes no other call."""
    with _env(env or {}):
        m = make_model(weights)
        c = Ctx(m)
        c.prep(data[2][:B], data[1][:B])
        out = _call(c, entry, data[0][:B]), c.opt(b"graph_captures")
        free(m)
    return out


def _all_entries(weights, data, batches, env=None):
    """Every entry point in turn on one context at each batch size: ({(B, entry): result}, graph_captures, chains at the last batch)."""
    with _env(env or {}):
        m = make_model(weights)
        c = Ctx(m)
        got = {}
        for B in batches:
            c.prep(data[2][:B], data[1][:B])
            for entry in ENTRIES:
                got[(B, entry)] = _call(c, entry, data[0][:B])
        out = got, c.opt(b"graph_captures"), _L().hd_num_chains(c.ctx)
        free(m)
    return out


@pytest.fixture(scope="module")
def shared(gpu, weights16, data):
    return _all_entries(weights16, data, (2, 3))


@pytest.fixture(scope="module")
def shared_two_chains(gpu, weights16, data):
    return _all_entries(weights16, data, (4,), TWO_CHAINS)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_on_the_shared_context_equals_a_fresh_context(shared, weights16, data, entry):
    for B in (2, 3):
        got = shared[0][(B, entry)]
        want, _ = _fresh(weights16, data, B, entry)
        assert bool(torch.isfinite(got).all()) and not torch.equal(got[0], data[0][0])      # face 0 runs every row
        if B == 3 and entry not in ("hd_sample", "hd_sample_multistep"):
            assert torch.equal(got[2], data[0][2])                                          # start row 3: held
        assert torch.equal(got, want), (B, entry)


@pytest.mark.gpu
def test_shared_context_captures_one_plain_and_one_per_face_pair_per_batch(shared, weights16, data):
    want = 0
    for entry in ("hd_sample", "hd_sample_rows"):
        with _env({}):
            m = make_model(weights16)
            c = Ctx(m)
            for B in (2, 3):
                c.prep(data[2][:B], data[1][:B])
                _call(c, entry, data[0][:B])
            want += c.opt(b"graph_captures")
            free(m)
    assert want > 0 and shared[1] == want


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_with_two_chains_equals_a_fresh_context(shared_two_chains, weights16, data, entry):
    got, captures, chains = shared_two_chains
    assert chains == 2
    want, fresh_captures = _fresh(weights16, data, 4, entry, TWO_CHAINS)
    assert torch.equal(got[(4, entry)], want), entry
    assert not torch.equal(want[3], data[0][3])                        # a face of the second chain ran
    assert captures == 2 * fresh_captures                              # one plain and one per-face pair per chain, whatever the order


# Which kind of evaluation a launch of the denoiser program belongs to is state of the context that every call sets for itself: one
# timestep or one per face (hd_eps), the loop's shared staged row (hd_sample) or per-face rows (hd_sample_rows).  The order of the calls
# on one context must not matter.
MODE_SEQUENCE = ("eps_one", "eps_faces", "hd_sample_rows", "eps_one", "hd_sample", "eps_faces")


def _mode_call(c, what, x):
    if what.startswith("eps"):
        t = 500 if what == "eps_one" else torch.tensor([500.0, 37.0])
        out = c.e.eps(x.cuda(), t)
        return c.done((0, out))
    return _call(c, what, x, _sched("ddim", 3).coefficient_table())          # hd_sample_rows: start rows (0, 1)


def _mode_ctx(weights, data, stages):
    m = make_model(weights)
    c = Ctx(m)
    if not stages:                                                           # the per-GEMM form of the same closures
        for key in (b"xcd", b"face"):
            assert _L().hd_set_option(c.ctx, key, 0) == 0
    c.prep(data[2][:2], data[1][:2])
    return m, c


@pytest.mark.gpu
@pytest.mark.parametrize("stages", (True, False), ids=("stages", "per_gemm"))
def test_evaluation_modes_in_any_order_equal_a_fresh_context(gpu, weights16, data, stages):
    x = data[0][:2]
    with _env({}):
        want = {}
        for what in sorted(set(MODE_SEQUENCE)):
            m, c = _mode_ctx(weights16, data, stages)
            want[what] = _mode_call(c, what, x)
            free(m)
        m, c = _mode_ctx(weights16, data, stages)
        got = [_mode_call(c, what, x) for what in MODE_SEQUENCE]
        launches = c.opt(b"sample_stage_launches"), c.opt(b"rows_stage_launches")
        free(m)
    assert (min(launches) > 0) if stages else (launches == (0, 0)), launches
    for i, what in enumerate(MODE_SEQUENCE):
        assert bool(torch.isfinite(got[i]).all()) and not torch.equal(got[i], x), (i, what)
        assert torch.equal(got[i], want[what]), (i, what)
    assert not torch.equal(want["eps_one"][1], want["eps_faces"][1])         # face 1 has its own timestep
