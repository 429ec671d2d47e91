"""The per-face extras of a prepared batch together -- masks, guidance, previews and the multistep history -- through the events of their
lifetime table (hd_lib.hip): hd_prepare*, a slot refill (hd_prepare_slots, hd_pool_commit), config off, hd_sample*, hd_pool_prepare.

Everything here compares bits or counts (torch.equal, ==): the same launches on the same values reached two ways.  Latent 16, batch 4
(batch 8 once, for buffers with a larger cap than the batch), a 10-row table, the synthetic weights of the sibling tests."""
import pytest
import torch

from conftest import weights16  # noqa: F401  (session fixture)
from test_guide import GRunner
from test_mask import _L, _tables, box, free, make_model
from test_spans import _env


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def data(gpu):
    """(x, crl, crf) of 8 faces, 4 more for refills, and guidance targets that are not the coarse latents."""
    from hifidiff_amd import synth
    x, crl, crf = synth.sample_inputs(12, 16)
    g = torch.Generator().manual_seed(43)
    return x, crl, crf, torch.randn((8, 4, 16, 16), generator=g)


def _planes(run):
    """[(x0, rows)] of the latest plane and the two snapshot planes, whole batch."""
    return [run.preview(s) for s in (-1, 0, 1)]


def _same_planes(a, b, faces):
    return all(torch.equal(pa[0][f], pb[0][f]) and int(pa[1][f]) == int(pb[1][f]) for pa, pb in zip(a, b) for f in faces)


def _refused(run, fn):
    from hifidiff_amd import _lib
    with pytest.raises(_lib.HipError, match="no multistep history"):
        fn()


def _check_refilled(run, before, slot, y, tm, cm, row, masked, guided, captures):
    """What a slot refill leaves: the counts, slot `slot` without previews, the others' planes untouched, and no history to resume there."""
    assert run.opt("masked_faces") == masked and run.opt("guided_faces") == guided
    after = _planes(run)
    for x0, rows in after:
        assert int(rows[slot]) == -1 and not bool(x0[slot].any())
    assert _same_planes(before, after, [f for f in range(4) if f != slot])
    assert any(int(r[slot]) >= 0 and bool(p[slot].any()) for p, r in before)      # there was something to lose
    res = [0] * 4
    res[slot] = 1
    _refused(run, lambda: run.faces_ms(y, tm, cm, [row] * 4, 1, res))
    _refused(run, lambda: run.rows(y, tm, cm, [row] * 4, 1, resume=1))            # nor the whole batch
    other = [0] * 4
    other[0] = 1
    y = run.faces_ms(y, tm, cm, [row] * 4, 1, other)                              # face 0 still has its history
    assert run.opt("graph_captures") == captures
    return y


# ------------------------------------------------------------------------------------------------ 1. the lifetime table, all features at once
@pytest.mark.gpu
def test_lifetime_table_with_every_feature_on(gpu, weights16, data):
    x8, crl8, crf8, ga = data
    x, crl, crf = x8[:4], crl8[:4], crf8[:4]
    m = make_model(weights16)
    e = m.engine
    run = GRunner(m, crf, crl)
    _, tm, cm = _tables("dpm", 10)
    mask = box(4, 16, 4, 12, 2, 12)
    run.config(1, 2, 2)                                               # rows 1 and 3 of a face's schedule go to snapshot planes 0 and 1
    run.guide_config(1)
    run.mask(mask[:2], crl[:2], x[:2], slots=[0, 1])
    run.guide(ga[:2], 0.5, 4, rows=(1, 3), slots=[1, 2])
    assert run.opt("masked_faces") == 2 and run.opt("guided_faces") == 2
    y = run.rows(x, tm, cm, [0] * 4, 4)                               # 4 rows of the multistep table: every face has a history
    captures = run.opt("graph_captures")
    before = _planes(run)
    assert [r.tolist() for _, r in before] == [[3] * 4, [1] * 4, [3] * 4]

    # hd_prepare_slots of slot 1
    e.prepare_slots([1], crl8[8:9].cuda(), cr_face=crf8[8:9].cuda())
    y = _check_refilled(run, before, 1, y, tm, cm, 4, masked=1, guided=1, captures=captures)

    # hd_pool_prepare in between changes none of the counts and none of the planes
    run.mask(mask[:1], crl[2:3], x[2:3], slots=[2])                   # so that slot 2 has a mask to lose, too
    e.enable_pool(2)
    before = _planes(run)
    assert [r.tolist() for _, r in before] == [[4] * 4, [1, -1, 1, 1], [3, -1, 3, 3]]
    e.pool_prepare([0], crl8[9:10].cuda(), cr_face=crf8[9:10].cuda())
    assert run.opt("masked_faces") == 2 and run.opt("guided_faces") == 1
    assert _same_planes(before, _planes(run), range(4))
    y = run.faces_ms(y, tm, cm, [5] * 4, 1, [1] * 4)                  # and every face may still resume
    before = _planes(run)

    # hd_pool_commit into slot 2 does to slot 2 what hd_prepare_slots did to slot 1
    e.pool_commit([2], [0])
    y = _check_refilled(run, before, 2, y, tm, cm, 6, masked=1, guided=0, captures=captures)

    # hd_guide_config(0) sets guided_faces to 0 and leaves the masks; the step graphs are captured again, once
    run.guide(ga[:1], 0.5, 4, slots=[3])
    assert run.opt("guided_faces") == 1 and run.opt("graph_captures") == captures
    run.guide_config(0)
    assert run.opt("guided_faces") == 0 and run.opt("masked_faces") == 1
    y = run.faces_ms(y, tm, cm, [7] * 4, 1, [1] * 4)
    captures2 = run.opt("graph_captures")
    assert captures2 > captures
    y = run.faces_ms(y, tm, cm, [8] * 4, 1, [1] * 4)
    assert run.opt("graph_captures") == captures2

    # hd_prepare of the same batch sets everything to 0, with all preview rows -1
    e.prepare(crl.cuda(), cr_face=crf.cuda())
    assert run.opt("masked_faces") == 0 and run.opt("guided_faces") == 0 and run.opt("preview") == 1 and run.opt("guide") == 0
    for x0, rows in _planes(run):
        assert rows.tolist() == [-1] * 4 and not bool(x0.any())
    _refused(run, lambda: run.faces_ms(y, tm, cm, [9] * 4, 1, [1, 0, 0, 0]))
    _refused(run, lambda: run.rows(y, tm, cm, [9] * 4, 1, resume=1))
    y = run.faces_ms(y, tm, cm, [9] * 4, 1, [0] * 4)
    assert bool(torch.isfinite(y).all()) and run.opt("graph_captures") == captures2
    free(m)


# ------------------------------------------------------------------------------------------------ 2. / 3. buffers with a cap larger than the batch; two chains
def _features4(run, data, reverse=False):
    """Batch 4: masks on faces {0, 3}, windowed guidance on {1, 3}, previews with 2 snapshots (rows 2 and 5), then the 10 DDIM rows with
    per-face start rows.  reverse: the same settings through the slot lists in reversed order.  Returns the final latents and the planes."""
    x8, crl8, _, ga = data
    x, crl = x8[:4], crl8[:4]
    mask = box(4, 16, 4, 12, 2, 12)
    ms, gs = ([3, 0], [3, 1]) if reverse else ([0, 3], [1, 3])
    run.config(1, 3, 2)
    run.guide_config(1)
    run.mask(mask[ms], crl[ms], x[ms], slots=ms)
    run.guide(ga[gs], [0.5, 0.8] if not reverse else [0.8, 0.5], [4, 8] if not reverse else [8, 4], rows=(2, 6), slots=gs)
    assert run.opt("masked_faces") == 2 and run.opt("guided_faces") == 2
    _, td, cd = _tables("ddim", 10)
    out = run.rows(x, td, cd, [0, 1, 0, 2], 10)
    return out, _planes(run)


def _same_result(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]) for pa, pb in zip(a[1], b[1]))


@pytest.fixture(scope="module")
def fresh4(gpu, weights16, data):
    """A context that only ever saw batch 4: computed once, read-only."""
    x8, crl8, crf8, _ = data
    m = make_model(weights16)
    run = GRunner(m, crf8[:4], crl8[:4])
    res = _features4(run, data)
    stages = run.opt("rows_stage_launches")
    free(m)
    return res, stages


@pytest.mark.gpu
def test_cap_larger_than_batch(gpu, weights16, data, fresh4):
    """Buffers that were sized for batch 8 and are used at batch 4: the guidance row windows are two arrays `cap` (8) apart, and a chain's
    pointers are offsets of its first face -- all bit for bit what a context that only ever saw batch 4 gives."""
    x8, crl8, crf8, ga = data
    m = make_model(weights16)
    m.enable_previews(1, 1)                                           # planes of batch 8 with one snapshot: reallocated at batch 4
    run = GRunner(m, crf8[:8], crl8[:8])
    run.guide_config(1)
    run.mask(box(8, 16, 2, 10, 4, 14), crl8[:8], x8[:8])
    run.guide(ga, 1.0, 16, rows=(0, 1))
    assert run.opt("masked_faces") == 8 and run.opt("guided_faces") == 8
    _, td, cd = _tables("ddim", 10)
    run.rows(x8[:8], td, cd, [0] * 8, 2)
    m.prepare(crf8[:4].cuda(), crl8[:4].cuda())
    assert run.opt("masked_faces") == 0 and run.opt("guided_faces") == 0
    got = _features4(run, data)
    want, _ = fresh4
    assert [r.tolist() for _, r in got[1]] == [[9] * 4, [2, 2, 2, 2], [5] * 4]
    assert bool(got[1][1][0].any()) and bool(got[1][2][0].any())
    assert _same_result(got, want)
    free(m)


@pytest.mark.gpu
def test_two_chains(gpu, weights16, data, fresh4):
    """The batch-4 half of the case above as two chains of two faces (tests/test_guide.py::test_two_chains builds the context this way).
    The comparison made is two chains against two chains with every feature set through its slot list in reversed order, not against one
    chain: at latent 16 and batch 4 the one-chain program runs the persistent stages (asserted below on the one-chain context), two chains
    run one launch per GEMM, and the two programs may differ in the last bits of eps.  What this leaves unchecked -- a chain reading another
    chain's faces -- is checked on face 2, the first face of the second chain, which carries no mask and no guidance: its latents must be
    the bits of the same context without any mask or guidance, while the faces that carry one move."""
    x8, crl8, crf8, _ = data
    _, one_chain_stages = fresh4
    assert one_chain_stages > 0, one_chain_stages
    with _env({"HD_EXPERIMENTS": "1", "HD_CHAINS": "2"}):
        m = make_model(weights16)
        run = GRunner(m, crf8[:4], crl8[:4])
        assert _L().hd_num_chains(run.ctx) == 2
        fwd = _features4(run, data)
        assert [r.tolist() for _, r in fwd[1]] == [[9] * 4, [2, 2, 2, 2], [5] * 4]
        run.unguide()
        run.clear()
        _, td, cd = _tables("ddim", 10)
        plain = run.rows(x8[:4], td, cd, [0, 1, 0, 2], 10)
        assert run.opt("masked_faces") == 0 and run.opt("guided_faces") == 0
        rev = _features4(run, data, reverse=True)
        assert _same_result(fwd, rev)
        assert torch.equal(fwd[0][2], plain[2])
        assert all(not torch.equal(fwd[0][f], plain[f]) for f in (0, 1, 3))
        free(m)
