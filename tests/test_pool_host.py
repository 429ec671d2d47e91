"""CPU side of the conditioning pool: the C-ABI declarations of hd_pool_config / hd_pool_prepare / hd_pool_commit, the entry bookkeeping of
sampling.PoolTable, the argument checks of ContinuousSampler(prefetch=...) and its top-up rule against a fake model (no device needed)."""
import ctypes
import re

import pytest
import torch

from conftest import ROOT

POOL_CALLS = ("hd_pool_config", "hd_pool_prepare", "hd_pool_commit")


def test_pool_entries_are_declared_and_bound():
    from hifidiff_amd import _lib
    with open(f"{ROOT}/include/hifidiff_hip.h") as f:
        hdr = f.read()
    for name in POOL_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS
    assert '"pool_capacity"' in hdr and '"pool_valid"' in hdr
    L = _lib.lib()
    i32p = ctypes.POINTER(ctypes.c_int32)
    assert L.hd_pool_config.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert L.hd_pool_prepare.argtypes == [ctypes.c_void_p, ctypes.c_int, i32p] + [ctypes.c_void_p] * 4
    assert L.hd_pool_commit.argtypes == [ctypes.c_void_p, ctypes.c_int, i32p, i32p, ctypes.c_void_p]


def test_pool_table_fifo_lowest_entry_reuse_and_exhaustion():
    from hifidiff_amd.sampling import PoolTable
    t = PoolTable(4)
    assert t.free_entries() == [0, 1, 2, 3] and t.pending() == []
    assert t.take([10, 11, 12]) == [0, 1, 2]                          # lowest free entry first
    assert t.pending() == [(10, 0), (11, 1), (12, 2)] and t.free_entries() == [3]
    assert t.pop(2) == [(10, 0), (11, 1)]                             # FIFO: submission order
    assert t.pending() == [(12, 2)] and t.free_entries() == [3]       # popped entries stay taken until they are released
    t.release(1)
    assert t.free_entries() == [1, 3]
    assert t.take([13, 14]) == [1, 3]                                 # reuse after release, lowest first
    assert t.pending() == [(12, 2), (13, 1), (14, 3)]                 # ... and still oldest first, whatever the entry numbers
    with pytest.raises(RuntimeError):
        t.take([15])                                                  # entry 0 is not released yet: none free
    assert t.pending() == [(12, 2), (13, 1), (14, 3)]                 # a refused take changes nothing
    t.release(0)
    with pytest.raises(RuntimeError):
        t.take([15, 16])
    assert t.take([15]) == [0]
    assert t.pop(4) == [(12, 2), (13, 1), (14, 3), (15, 0)] and t.pop(0) == []
    with pytest.raises(ValueError):
        t.pop(1)                                                      # nothing prepared
    for e in range(4):
        t.release(e)
    with pytest.raises(ValueError):
        t.release(0)                                                  # free already
    assert t.take([20]) == [0]
    with pytest.raises(ValueError):
        t.release(0)                                                  # prepared, not committed yet


def test_pool_table_capacity_must_be_at_least_one():
    from hifidiff_amd.sampling import PoolTable
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            PoolTable(bad)
    assert PoolTable(1).free_entries() == [0]


class _FakeEngine:
    latent_res, device = 16, None

    def __init__(self, conditional=True):
        self.conditional = conditional
        self.cond_key = "stale"


class _FakeModel:
    """Records what the sampler asks of the model; entries hold the request (by the value of its cr_latent) they were prepared for."""

    def __init__(self, conditional=True):
        self.engine = _FakeEngine(conditional)
        self.calls, self.pool = [], None

    def enable_pool(self, capacity):
        self.pool = [None] * capacity
        self.calls.append(("enable_pool", capacity))

    def prepare(self, cr_face, cr_latent):
        self.calls.append(("prepare", cr_latent[:, 0, 0, 0].tolist()))

    def prepare_slots(self, slots, cr_face, cr_latent):
        self.calls.append(("prepare_slots", list(slots), cr_latent[:, 0, 0, 0].tolist()))

    def pool_prepare(self, entries, cr_face, cr_latent):
        assert tuple(cr_face.shape) == (len(entries), 3, 128, 128) and tuple(cr_latent.shape) == (len(entries), 4, 16, 16)
        who = cr_latent[:, 0, 0, 0].tolist()
        for e, w in zip(entries, who):
            self.pool[e] = w
        self.calls.append(("pool_prepare", list(entries), who))

    def pool_commit(self, slots, entries):
        self.calls.append(("pool_commit", list(slots), [self.pool[e] for e in entries]))

    def set_mask(self, mask, known, noise, slots=None):
        self.calls.append(("set_mask", list(slots)))

    def set_guidance(self, target, weight, scale, rows=None, slots=None):
        self.calls.append(("set_guidance", list(slots)))


def _ddim(n=10):
    from hifidiff_amd import schedulers
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(n)
    return s


def test_prefetch_argument_checks():
    from hifidiff_amd import sampling
    s = _ddim()
    for bad in (-1, 1.5, "8", True, None):
        with pytest.raises(ValueError):
            sampling.ContinuousSampler(_FakeModel(), s, batch=4, prefetch=bad)
    with pytest.raises(ValueError):
        sampling.ContinuousSampler(_FakeModel(conditional=False), s, batch=4, prefetch=2)   # no conditioning to prepare ahead
    m = _FakeModel()
    cs = sampling.ContinuousSampler(m, s, batch=4)                    # the default: today's path, no pool
    assert cs.prefetch == 0 and cs.pool is None and m.calls == [] and (cs.pool_calls, cs.pool_prepared) == (0, 0)
    cs = sampling.ContinuousSampler(m, s, batch=4, prefetch=6)
    assert m.calls == [("enable_pool", 6)] and cs.pool.capacity == 6
    from hifidiff_amd.refiner import entries_arg, pool_capacity_arg
    assert pool_capacity_arg(4096) == 4096 and entries_arg([5, 0, 2], 6, 3, True).tolist() == [5, 0, 2]
    assert entries_arg([2, 2], 6, 3, False).dtype == torch.int32     # a commit may repeat an entry
    for bad in (0, 4097, 2.0, True):
        with pytest.raises(ValueError):
            pool_capacity_arg(bad)
    for bad, distinct in (([2, 2], True), ([6], True), ([-1], False), ([], False), ([0, 1, 2, 3], False), ([0.5], False)):
        with pytest.raises(ValueError):
            entries_arg(bad, 6, 3, distinct)
    with pytest.raises(RuntimeError):
        entries_arg([0], None, 3, True)                               # no pool


def _scripted(prefetch, n_req, batch=4):
    """A sampler over the fake model with n_req requests; request i is recognisable by cr_latent == i and finishes when the script says
    so (its slot is emptied by hand: no device, no step())."""
    from hifidiff_amd import sampling
    m = _FakeModel()
    cs = sampling.ContinuousSampler(m, _ddim(), batch=batch, refill_every=1, prefetch=prefetch)
    for i in range(n_req):
        cs.submit(torch.zeros(3, 128, 128), torch.full((4, 16, 16), float(i)), seed=i, strength=1.0,
                  mask=torch.ones(16, 16) if i == 5 else None, fidelity=0.5 if i == 6 else None)
    cs.x = torch.zeros((batch, 4, 16, 16))
    m.calls.clear()

    def finish(*slots):
        for sl in slots:
            cs.table.req[sl] = None
    return cs, m, finish


def test_top_up_rule_on_a_scripted_sequence():
    cpu = torch.device("cpu")
    cs, m, finish = _scripted(prefetch=3, n_req=11)
    cs._refill(cpu)                                                   # the first fill: one prepare of the whole batch, nothing pooled
    assert m.calls == [("prepare", [0.0, 1.0, 2.0, 3.0])] and cs.prepared and m.engine.cond_key is None
    assert (cs.pool_calls, cs.pool_prepared, cs.refilled) == (0, 0, 0) and len(cs.queue) == 7
    m.calls.clear()
    cs._refill(cpu)                                                   # no free slot: no top-up, however long the queue
    assert m.calls == []
    finish(2)
    cs._refill(cpu)                                                   # 1 free slot, 0 prepared, 7 unprepared: min(7, 3 entries, 4) in one call
    assert m.calls == [("pool_prepare", [0, 1, 2], [4.0, 5.0, 6.0]), ("pool_commit", [2], [4.0])]
    assert cs.table.req == [0, 1, 4, 3] and cs.pool.pending() == [(5, 1), (6, 2)] and cs.pool.free_entries() == [0]
    m.calls.clear()
    finish(0, 3)
    cs._refill(cpu)                                                   # 2 free slots, 2 prepared: no top-up; oldest first into the lowest slots
    assert m.calls == [("pool_commit", [0, 3], [5.0, 6.0]), ("set_mask", [0]), ("set_guidance", [3])]
    assert cs.table.req == [5, 1, 4, 6] and cs.pool.pending() == [] and cs.pool.free_entries() == [0, 1, 2]
    m.calls.clear()
    finish(0, 1, 2, 3)
    cs._refill(cpu)                                                   # 4 free slots, 0 prepared: the pool limits the refill to its 3 entries
    assert m.calls == [("pool_prepare", [0, 1, 2], [7.0, 8.0, 9.0]), ("pool_commit", [0, 1, 2], [7.0, 8.0, 9.0])]
    assert cs.table.req == [7, 8, 9, None]
    m.calls.clear()
    cs._refill(cpu)                                                   # the slot left over: 1 free, 0 prepared, 1 unprepared
    assert m.calls == [("pool_prepare", [0], [10.0]), ("pool_commit", [3], [10.0])]
    assert cs.table.req == [7, 8, 9, 10] and cs.queue == []
    m.calls.clear()
    finish(1)
    cs._refill(cpu)                                                   # an empty queue: nothing to prepare, nothing to commit
    assert m.calls == []
    assert (cs.pool_calls, cs.pool_prepared, cs.refilled) == (3, 7, 7)
    assert cs.seeds == [7, 8, 9, 10]


def test_top_up_is_limited_by_the_batch_and_prefetch_zero_keeps_prepare_slots():
    cpu = torch.device("cpu")
    cs, m, finish = _scripted(prefetch=16, n_req=12, batch=2)
    cs._refill(cpu)
    m.calls.clear()
    finish(1)
    cs._refill(cpu)                                                   # 10 unprepared, 16 free entries: one call prepares at most a batch
    assert m.calls == [("pool_prepare", [0, 1], [2.0, 3.0]), ("pool_commit", [1], [2.0])]
    m.calls.clear()
    finish(0, 1)
    cs._refill(cpu)                                                   # 2 free slots, 1 prepared: top-up into the lowest free entries
    assert m.calls == [("pool_prepare", [0, 2], [4.0, 5.0]), ("pool_commit", [0, 1], [3.0, 4.0])]
    assert cs.pool.pending() == [(5, 2)]
    # prefetch 0: the refill is prepare_slots, and no pool call is ever made
    cs, m, finish = _scripted(prefetch=0, n_req=4, batch=2)
    cs._refill(cpu)
    finish(0)
    cs._refill(cpu)
    assert m.calls == [("prepare", [0.0, 1.0]), ("prepare_slots", [0], [2.0])] and cs.refilled == 1 and cs.pool_calls == 0
