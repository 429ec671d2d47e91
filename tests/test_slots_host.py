"""CPU side of continuous batching: the C-ABI declarations of hd_prepare_slots / hd_sample_faces*, the slot bookkeeping of
sampling.SlotTable, the per-face Philox key restated in numpy, and argument validation of the Python wrappers (no device needed)."""
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_multistep import _philox_normal


def test_new_entries_are_declared_and_bound():
    from hifidiff_amd import _lib
    with open(f"{ROOT}/include/hifidiff_hip.h") as f:
        hdr = f.read()
    for name in ("hd_prepare_slots", "hd_sample_faces", "hd_sample_faces_multistep"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
    assert '"graph_captures"' in hdr


def test_slot_table_assignment_refill_order_and_completion():
    from hifidiff_amd.sampling import SlotTable
    t = SlotTable(4, 10)
    assert t.start_rows() == [10] * 4 and t.iters(5) == 0            # empty: every slot held, nothing to run
    assert [t.assign(r, s) for r, s in ((0, 0), (1, 6), (2, 3))] == [0, 1, 2]   # lowest free slot first
    assert t.start_rows() == [0, 6, 3, 10] and t.free_slots() == [3]
    assert t.resume_flags() == [0, 0, 0, 0]                           # fresh requests: first row first-order
    assert t.iters(5) == 5                                            # slot 1 finishes inside the call and is held for the rest
    assert t.advance(5) == [(1, 1)]
    assert t.start_rows() == [5, 10, 8, 10] and t.resume_flags() == [1, 0, 1, 0]
    assert t.assign(3, 8) == 1 and t.assign(4, 9) == 3                # refill in slot order
    assert t.resume_flags() == [1, 0, 1, 0] and t.start_rows() == [5, 8, 8, 9]
    assert t.iters(3) == 3 and t.iters(100) == 5                      # no slot has more than 5 rows left
    assert sorted(t.advance(3)) == [(1, 3), (2, 2), (3, 4)]
    assert t.start_rows() == [8, 10, 10, 10] and t.resume_flags() == [1, 0, 0, 0]
    with pytest.raises(ValueError):
        t.assign(9, 11)
    t.assign(5, 10)                                                   # strength 0: done at the next advance without running a row
    assert t.iters(10) == 2
    assert sorted(t.advance(2)) == [(0, 0), (1, 5)] and t.resume_flags() == [0, 0, 0, 0]
    for r in (6, 7, 8, 9):
        t.assign(r, 0)
    with pytest.raises(RuntimeError):
        t.assign(10, 0)


def test_slot_table_start_rows_from_strengths():
    from hifidiff_amd import sampling, schedulers
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(10)
    t = sampling.SlotTable(3, 10)
    cr = torch.zeros((3, 4, 16, 16))
    _, start = sampling.img2img_start(s, cr, torch.tensor([1.0, 0.45, 0.2]), noise=torch.zeros_like(cr))
    for r, st in enumerate(start.tolist()):
        t.assign(r, st)
    assert t.start_rows() == [0, 6, 8]                                # n - min(int(n * s), n)


def test_per_face_key_is_independent_of_the_slot():
    """z of face f at row k, element e is Philox(face_seeds[f]; k, e): the same numbers in slot 0 and slot 40, and in slot 0 exactly the
    batch keying Philox(seed; k, gi) of hd_sample_rows with seed = the face's key (gi = e there)."""
    per_face = 4 * 16 * 16
    e = np.arange(per_face, dtype=np.uint64)
    seed, k = 0x1234_5678_9ABC, 7
    z_face = _philox_normal(seed, k, e)
    # the device computes the element index inside the face from the slot: o - slot * per_face
    for slot in (0, 5, 40):
        gi = np.arange(slot * per_face, (slot + 1) * per_face, dtype=np.uint64)
        assert np.array_equal(_philox_normal(seed, k, gi - np.uint64(slot * per_face)), z_face)
    batch_z = _philox_normal(seed, k, np.arange(64 * per_face, dtype=np.uint64))
    assert np.array_equal(batch_z[:per_face], z_face)                 # slot 0: hd_sample_rows(seed = s), face 0
    assert not np.array_equal(batch_z[40 * per_face:41 * per_face], z_face)   # batch keying depends on the slot
    assert abs(float(z_face.mean())) < 0.1 and abs(float(z_face.std()) - 1) < 0.1


def test_python_argument_validation():
    from hifidiff_amd import sampling
    from hifidiff_amd.refiner import slots_arg
    assert slots_arg([3, 17, 40], 64).tolist() == [3, 17, 40] and slots_arg(torch.tensor([1]), 2).dtype == torch.int32
    for bad in ([3, 3], [64], [-1], [], list(range(65)), [1.5], torch.tensor([True])):
        with pytest.raises(ValueError):
            slots_arg(bad, 64)
    with pytest.raises(RuntimeError):
        slots_arg([0], None)                                          # nothing prepared
    s = sampling.face_seeds_arg(torch.tensor([0, -1, 5]), 3)
    assert s.dtype == np.uint64 and s.tolist() == [0, 2 ** 64 - 1, 5]
    assert sampling.face_seeds_arg([2 ** 64 - 1, 1], 2).tolist() == [2 ** 64 - 1, 1]
    for bad, B in (([1, 2], 3), (torch.tensor([0.5, 1.0]), 2), ([2 ** 64], 1)):
        with pytest.raises(ValueError):
            sampling.face_seeds_arg(bad, B)
    assert sampling.resume_arg(torch.tensor([True, False]), 2).tolist() == [1, 0]
    assert sampling.resume_arg(True, 3).tolist() == [1, 1, 1]
    for bad in (torch.tensor([1, 0, 1]), torch.tensor([2, 0]), torch.tensor([0.5, 1.0])):
        with pytest.raises(ValueError):
            sampling.resume_arg(bad, 2)


class _FakeEngine:
    conditional, latent_res, device = True, 16, None


class _FakeModel:
    engine = _FakeEngine()


def test_continuous_sampler_submit_validation_and_start():
    from hifidiff_amd import sampling, schedulers
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(10)
    cs = sampling.ContinuousSampler(_FakeModel(), s, batch=4, refill_every=3)
    crf, crl = torch.zeros(3, 128, 128), torch.randn(4, 16, 16, generator=torch.Generator().manual_seed(0))
    assert [cs.submit(crf, crl, seed=i, strength=0.5) for i in range(2)] == [0, 1]
    for args in ((crf, crl[:2], 0, 1.0), (crf, crl, 0, 1.5), (crf, crl, -1, 1.0), (None, crl, 0, 1.0)):
        with pytest.raises(ValueError):
            cs.submit(*args)
    with pytest.raises(ValueError):
        sampling.ContinuousSampler(_FakeModel(), s, batch=0)
    # initial latents: a CPU generator seeded by the request, img2img_start's convention -- independent of the slot
    lat, start = cs._start(crl, 7, 0.5)
    want, wstart = sampling.img2img_start(s, crl[None], 0.5, noise=torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(7)))
    assert start == int(wstart[0]) == 5 and torch.equal(lat, want[0])
