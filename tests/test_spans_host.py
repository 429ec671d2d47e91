"""CPU side of per-request schedules: the C-ABI declaration of hd_sample_spans, sampling.ScheduleSet (concatenated tables and spans),
sampling.SlotTable with a span per slot, and the argument validation of sample(scheduler=ScheduleSet, schedules=...) (no device needed)."""
import re

import pytest
import torch

from conftest import ROOT


def _members():
    from hifidiff_amd import schedulers
    m = {"ddim10": schedulers.DDIMScheduler(clip_sample_range=3.0), "dpm8": schedulers.DPMSolverMultistepScheduler(),
         "ddpm12": schedulers.DDPMScheduler(clip_sample_range=3.0),
         "sde6": schedulers.DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")}
    for k, n in (("ddim10", 10), ("dpm8", 8), ("ddpm12", 12), ("sde6", 6)):
        m[k].set_timesteps(n)
    return m


def test_hd_sample_spans_is_declared_and_bound():
    from hifidiff_amd import _lib
    with open(f"{ROOT}/include/hifidiff_hip.h") as f:
        hdr = f.read()
    assert re.search(r"\bint\s+hd_sample_spans\s*\(", hdr)
    assert "hd_sample_spans" in _lib.EXPORTS
    decl = hdr[hdr.index("int hd_sample_spans"):]
    decl = decl[:decl.index(";")]
    for arg in ("begin_rows", "end_rows", "start_rows", "n_iters", "resume", "face_seeds", "noise", "seed", "stream"):
        assert arg in decl, arg
    with open(f"{ROOT}/INTEGRATION.md") as f:
        assert "hd_sample_spans(" in f.read()


def test_schedule_set_concatenates_the_members_row_for_row():
    from hifidiff_amd.sampling import ScheduleSet
    m = _members()
    ss = ScheduleSet(m)
    ts, coef = ss.coefficient_table()
    assert ts.dtype == torch.float32 and coef.dtype == torch.float32 and coef.shape == (36, 8) and ts.shape == (36,)
    assert ts.is_contiguous() and coef.is_contiguous()
    at = 0
    for k in ("ddim10", "dpm8", "ddpm12", "sde6"):                     # the dict's order
        mt, mc = m[k].coefficient_table()
        b, e = ss.span(k)
        assert (b, e) == (at, at + mt.numel())                        # the spans tile the table
        assert torch.equal(ts[b:e], mt)
        assert torch.equal(coef[b:e, :mc.shape[1]], mc)
        if mc.shape[1] == 7:
            assert bool((coef[b:e, 7] == 0).all())                    # DDIM / DDPM rows: c7 = 0
        assert float(coef[b, 7]) == 0.0                               # a schedule's first row has no history term
        at = e
    assert at == 36
    assert float(coef[ss.span("dpm8")[0] + 1, 7]) != 0.0              # second-order rows keep theirs
    assert ss.coefficient_table()[1] is coef                          # cached


def test_schedule_set_from_a_list_and_refusals():
    from hifidiff_amd import schedulers
    from hifidiff_amd.sampling import ScheduleSet
    m = _members()
    ss = ScheduleSet([m["dpm8"], m["ddim10"]])
    assert ss.keys == [0, 1] and ss.span(0) == (0, 8) and ss.span(1) == (8, 18) and len(ss) == 2
    with pytest.raises(KeyError):
        ss.span(2)
    for bad in ({}, []):
        with pytest.raises(ValueError):
            ScheduleSet(bad)
    unset = schedulers.DPMSolverMultistepScheduler()
    if getattr(unset, "timesteps", None) is not None and len(unset.timesteps):
        unset.timesteps = unset.timesteps[:0]
    with pytest.raises(ValueError):
        ScheduleSet({"a": m["ddim10"], "b": unset})
    with pytest.raises(ValueError):
        ScheduleSet([object()])


def test_schedule_set_cache_follows_set_timesteps():
    from hifidiff_amd.sampling import ScheduleSet
    m = _members()
    ss = ScheduleSet(m)
    ts0, coef0 = ss.coefficient_table()
    assert ss.span("sde6") == (30, 36)
    m["ddim10"].set_timesteps(10)                                     # the same schedule: the member's cache hits, and so does the set's
    assert ss.coefficient_table()[1] is coef0
    m["ddim10"].set_timesteps(25)
    ts1, coef1 = ss.coefficient_table()
    assert coef1.shape == (51, 8) and ss.span("ddim10") == (0, 25) and ss.span("dpm8") == (25, 33) and ss.span("sde6") == (45, 51)
    assert torch.equal(ts1[:25], m["ddim10"].coefficient_table()[0])
    assert torch.equal(coef1[25:], coef0[10:]) and torch.equal(ts1[25:], ts0[10:])


def test_slot_table_holds_a_10_row_and_a_50_row_request_together():
    from hifidiff_amd.sampling import SlotTable
    t = SlotTable(3, 60)                                              # table: rows [0, 10) and [10, 60)
    assert t.begin_rows() == [60] * 3 and t.end_rows() == [60] * 3 and t.start_rows() == [60] * 3   # empty: held, start == end
    assert t.assign("short", 0, 0, 10) == 0 and t.assign("long", 10, 10, 60) == 1
    assert t.begin_rows() == [0, 10, 60] and t.end_rows() == [10, 60, 60] and t.start_rows() == [0, 10, 60]
    assert t.resume_flags() == [0, 0, 0]
    assert t.iters(8) == 8 and t.advance(8) == []
    assert t.start_rows() == [8, 18, 60] and t.resume_flags() == [1, 1, 0]
    assert t.iters(8) == 8                                            # the long request has 42 rows left, the short one 2: held inside the call
    assert t.advance(8) == [(0, "short")]                             # complete at its own end, not the table's
    assert t.start_rows() == [60, 26, 60] and t.free_slots() == [0, 2]
    assert t.assign("img2img", 16, 10, 60) == 0 and t.assign("short2", 4, 0, 10) == 2   # refill in slot order
    assert t.start_rows() == [16, 26, 4] and t.begin_rows() == [10, 10, 0] and t.end_rows() == [60, 60, 10]
    assert t.resume_flags() == [0, 1, 0]
    assert t.iters(100) == 44                                         # the longest remaining run
    assert t.iters(6) == 6 and t.advance(6) == [(2, "short2")]
    assert t.start_rows() == [22, 32, 60] and t.end_rows() == [60, 60, 60]
    assert sorted(t.advance(28)) == [(1, "long")] and t.start_rows() == [50, 60, 60]
    assert t.iters(20) == 10 and t.advance(10) == [(0, "img2img")] and t.iters(5) == 0
    for bad in ((0, 5, 4), (0, -1, 10), (0, 0, 61), (11, 0, 10), (9, 10, 60)):   # (start, begin, end)
        with pytest.raises(ValueError):
            t.assign("bad", *bad)
    t.assign("empty", 10, 0, 10)                                      # strength 0: complete at the next advance without running a row
    assert t.iters(5) == 0 and t.advance(0) == [(0, "empty")]


def test_slot_table_without_spans_is_unchanged():
    from hifidiff_amd.sampling import SlotTable
    t = SlotTable(4, 10)
    assert t.start_rows() == [10] * 4 and t.iters(5) == 0
    assert [t.assign(r, s) for r, s in ((0, 0), (1, 6), (2, 3))] == [0, 1, 2]
    assert t.begin_rows() == [0, 0, 0, 10] and t.end_rows() == [10] * 4
    assert t.start_rows() == [0, 6, 3, 10] and t.iters(5) == 5 and t.advance(5) == [(1, 1)]
    assert t.start_rows() == [5, 10, 8, 10] and t.resume_flags() == [1, 0, 1, 0]
    assert t.assign(3, 8) == 1 and t.assign(4, 9) == 3
    assert t.iters(3) == 3 and t.iters(100) == 5
    assert sorted(t.advance(3)) == [(1, 3), (2, 2), (3, 4)]
    with pytest.raises(ValueError):
        t.assign(9, 11)


class _FakeEngine:
    conditional, latent_res, device = True, 16, None


class _FakeModel:
    engine = _FakeEngine()


def test_sample_argument_errors_come_before_any_device_work():
    from hifidiff_amd import sampling
    m = _members()
    ss = sampling.ScheduleSet(m)
    x = torch.zeros((3, 4, 16, 16))
    call = lambda **kw: sampling.sample(_FakeModel(), x, None, None, ss, **kw)   # noqa: E731
    with pytest.raises(ValueError):
        call()                                                        # a set needs schedules=
    with pytest.raises(KeyError):
        call(schedules="ddim99")                                      # an unknown key
    with pytest.raises(KeyError):
        call(schedules=["ddim10", "dpm8", "nope"])
    with pytest.raises(ValueError):
        call(schedules=["ddim10", "dpm8"])                            # a wrong length
    with pytest.raises(ValueError):
        call(schedules=["ddim10", "dpm8", "sde6"], start_steps=torch.tensor([0, 9, 0]))    # row 9 of an 8-row schedule
    with pytest.raises(ValueError):
        call(schedules="sde6", start_steps=-1)
    with pytest.raises(ValueError):
        call(schedules="sde6", start_steps=torch.tensor([0, 1]))
    with pytest.raises(ValueError):
        sampling.sample(_FakeModel(), x, None, None, m["ddim10"], schedules="ddim10")      # schedules= without a set
    b, e, r = sampling._span_args(ss, ["ddim10", "dpm8", "sde6"], torch.tensor([10, 3, 0]), 3)
    assert b.tolist() == [0, 10, 30] and e.tolist() == [10, 18, 36] and r.tolist() == [10, 13, 30]
    assert b.dtype == e.dtype == r.dtype == torch.int32


def test_continuous_sampler_over_a_set_picks_the_member_for_the_start():
    from hifidiff_amd import sampling
    m = _members()
    ss = sampling.ScheduleSet(m)
    cs = sampling.ContinuousSampler(_FakeModel(), ss, batch=4, refill_every=3)
    assert cs.n_steps == 36 and cs.table.n_steps == 36
    crf, crl = torch.zeros(3, 128, 128), torch.randn(4, 16, 16, generator=torch.Generator().manual_seed(0))
    assert cs.submit(crf, crl, seed=1, strength=0.5) == 0 and cs.queue[0][-1] == "ddim10"     # default: the first member
    assert cs.submit(crf, crl, seed=2, strength=0.5, schedule="dpm8") == 1
    with pytest.raises(KeyError):
        cs.submit(crf, crl, seed=3, schedule="nope")
    z = torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(7))
    for key, n in (("ddim10", 10), ("dpm8", 8), ("ddpm12", 12)):
        lat, start = cs._start(crl, 7, 0.5, schedule=key)
        want, wstart = sampling.img2img_start(m[key], crl[None], 0.5, noise=z)
        assert start == int(wstart[0]) == n - n // 2 and torch.equal(lat, want[0])       # relative to the member's own row count
    plain = sampling.ContinuousSampler(_FakeModel(), m["ddim10"], batch=4)
    with pytest.raises(ValueError):
        plain.submit(crf, crl, seed=1, schedule="ddim10")
