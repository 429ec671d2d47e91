"""CPU side of the progress previews: the C-ABI declarations of hd_preview_config / hd_preview_read, the argument checks of the Python
surface (all before any device work) and the progress arithmetic of ContinuousSampler.previews() over a SlotTable with spans."""
import re

import pytest
import torch

from conftest import ROOT


def test_new_entries_are_declared_and_bound():
    from hifidiff_amd import _lib
    with open(f"{ROOT}/include/hifidiff_hip.h") as f:
        hdr = f.read()
    for name in ("hd_preview_config", "hd_preview_read"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
    for word in ("x0_preview", "preview_rows", "preview_snaps", '"preview"'):
        assert word in hdr, word


def test_argument_errors_come_before_any_device_work():
    from hifidiff_amd import sampling, schedulers
    from hifidiff_amd.refiner import Denoiser, FacialRefiner
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(10)
    x = torch.zeros((2, 4, 16, 16))
    for model in (FacialRefiner(16), Denoiser(16)):                   # no weights, no device: anything past the checks would raise RuntimeError
        for bad in (0, -1, True, 2.0, "2"):
            with pytest.raises(ValueError):
                sampling.sample(model, x, None, None, s, previews=bad)
        for kw in (dict(every=0), dict(every=-3), dict(snapshots=-1), dict(snapshots=65), dict(every=1.5), dict(every=True)):
            with pytest.raises(ValueError):
                model.enable_previews(**kw)
        assert model.engine.preview_cfg is None and model.engine.ctx is None
        model.enable_previews(every=2, snapshots=64)                  # the setting is kept for the context the model will create
        assert model.engine.preview_cfg == (2, 64)
        for bad in (-1, 64):
            with pytest.raises(ValueError):
                model.previews(snapshot=bad)
        model.disable_previews()
        assert model.engine.preview_cfg is None
        with pytest.raises(RuntimeError):
            model.previews()
    s.set_timesteps(130)                                              # 130 rows, every 2nd: 65 snapshots
    with pytest.raises(ValueError):
        sampling.sample(FacialRefiner(16), x, None, None, s, previews=2)
    sset = sampling.ScheduleSet({"a": s})
    with pytest.raises(ValueError):
        sampling.sample(FacialRefiner(16), x, None, None, sset, schedules="a", previews=2)


def test_slot_table_progress_is_relative_to_the_span():
    from hifidiff_amd.sampling import SlotTable
    t = SlotTable(4, 30)                                              # a table of two schedules: rows [0, 10) and [10, 30)
    assert t.assign("a", 4, 0, 10) == 0 and t.assign("b", 10, 10, 30) == 1 and t.assign("c", 30, 10, 30) == 2
    assert [t.progress(i, 5) for i in range(4)] == [None] * 4         # nobody has run a row: a slot may hold its predecessor's preview
    assert t.advance(3) == [(2, "c")]                                 # "c" (strength 0) completes without a row
    assert t.progress(0, 6) == (7, 10)                                # rows 4, 5, 6 of [0, 10): 7 of 10 done
    assert t.progress(1, 12) == (3, 20)                               # rows 10, 11, 12 of [10, 30)
    assert t.progress(1, 9) is None and t.progress(1, 30) is None and t.progress(0, -1) is None     # outside the span / no estimate
    assert t.progress(2, 12) is None and t.progress(3, 12) is None    # empty slots
    assert t.advance(3) == [(0, "a")]
    assert t.progress(0, 9) is None and t.progress(1, 15) == (6, 20)


class _StubEngine:
    conditional, latent_res, device = False, 16, None


class _StubModel:
    """What ContinuousSampler.previews() needs of a model, on the host: previews(slots) hands back the rows the test planted."""

    def __init__(self):
        self.engine, self.rows, self.enabled = _StubEngine(), {}, None

    def enable_previews(self, every=1, snapshots=0):
        self.enabled = (every, snapshots)

    def previews(self, slots=None, snapshot=None):
        x0 = torch.stack([torch.full((4, 16, 16), float(s)) for s in slots])
        return x0, torch.tensor([self.rows[s] for s in slots], dtype=torch.int32)


def test_continuous_sampler_previews_arithmetic():
    from hifidiff_amd import sampling, schedulers
    members = {}
    for n in (4, 8):
        members[n] = schedulers.DDIMScheduler(clip_sample_range=3.0)
        members[n].set_timesteps(n)
    sset = sampling.ScheduleSet(members)                              # table rows [0, 4) and [4, 12)
    model = _StubModel()
    with pytest.raises(RuntimeError):
        sampling.ContinuousSampler(model, sset, batch=3).previews()
    assert model.enabled is None
    cs = sampling.ContinuousSampler(model, sset, batch=3, previews=True)
    assert model.enabled == (1, 0)
    assert cs.previews() == {}                                        # nothing in a slot
    t = cs.table
    t.assign(10, 0, 0, 4); t.assign(11, 4, 4, 12); t.assign(12, 9, 4, 12)     # request 12: strength 3/8 of the 8-row member
    assert cs.previews() == {}                                        # in their slots, but no row run yet
    t.advance(2)
    model.rows = {0: 1, 1: 5, 2: 10}                                  # what the device holds after two iterations
    pr = cs.previews()
    assert {k: v[:2] for k, v in pr.items()} == {10: (2, 4), 11: (2, 8), 12: (7, 8)}
    assert all(torch.equal(pr[rid][2], torch.full((4, 16, 16), float(slot))) for slot, rid in enumerate((10, 11, 12)))
    assert t.advance(2) == [(0, 10), (2, 12)]                         # both reach their last row and leave their slots
    model.rows = {1: 7}
    assert {k: v[:2] for k, v in cs.previews().items()} == {11: (4, 8)}
    t.assign(13, 0, 0, 4)                                             # refills slot 0, whose plane still holds request 10's preview
    model.rows = {0: 3, 1: 7}
    assert sorted(cs.previews()) == [11]
