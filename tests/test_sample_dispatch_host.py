"""Which of the seven sampling-loop entry points sample() and ContinuousSampler.step() call, and with which values (no device needed).

A fake engine and a fake library stand in for the real ones; the fake library records the name and the decoded arguments of every call.
The expected calls are written out from the rules of include/hifidiff_hip.h and sample()'s docstring: 7 columns -> hd_sample*, 8 columns
-> *_multistep; start_steps -> hd_sample_rows*; face_seeds or a per-face resume -> hd_sample_faces*; a ScheduleSet -> hd_sample_spans;
n_iters defaults to the longest remaining run, and a call in which every face is held is not made at all."""
import contextlib

import pytest
import torch

B, CTX, STREAM = 3, 0xC0FFEE, 77


class _FakeLib:
    """Records (name, decoded arguments) of each entry-point call; every call succeeds."""
    I32 = {"hd_sample_rows": ("rows",), "hd_sample_rows_multistep": ("rows",), "hd_sample_faces": ("rows",),
           "hd_sample_faces_multistep": ("rows", "resume"), "hd_sample_spans": ("begin", "end", "rows", "resume")}
    ORDER = {"hd_sample": ("noise", "seed", "stream"), "hd_sample_multistep": ("noise", "seed", "stream"),
             "hd_sample_rows": ("rows", "n_iters", "noise", "seed", "stream"),
             "hd_sample_rows_multistep": ("rows", "n_iters", "resume", "noise", "seed", "stream"),
             "hd_sample_faces": ("rows", "n_iters", "face_seeds", "noise", "seed", "stream"),
             "hd_sample_faces_multistep": ("rows", "n_iters", "resume", "face_seeds", "noise", "seed", "stream"),
             "hd_sample_spans": ("begin", "end", "rows", "n_iters", "resume", "face_seeds", "noise", "seed", "stream")}

    def __init__(self, batch):
        self.batch, self.calls = batch, []

    def __getattr__(self, name):
        if name not in self.ORDER:
            raise AttributeError(name)

        def fn(ctx, x, sched, *rest):
            sc = sched._obj if hasattr(sched, "_obj") else sched.contents
            n = int(sc.n_steps)
            ncoef = 8 if type(sc).__name__ == "ScheduleMS" else 7
            rec = {"ctx": ctx, "x": x, "n_steps": n, "ncoef": ncoef, "timesteps": [sc.timesteps[i] for i in range(n)],
                   "coef": [sc.coef[i] for i in range(n * ncoef)]}
            assert len(rest) == len(self.ORDER[name]), (name, len(rest))
            for key, v in zip(self.ORDER[name], rest):
                if key in self.I32.get(name, ()) or (key == "face_seeds" and v is not None):
                    v = [int(v[i]) for i in range(self.batch)]
                rec[key] = v
            self.calls.append((name, rec))
            return 0
        return fn


class _FakeEngine:
    conditional, latent_res, device, ctx = True, 16, torch.device("cpu"), CTX

    def __init__(self):
        self.checks = 0

    def ensure(self, device):
        pass

    def require_loaded(self):
        pass

    def clear_mask(self):
        pass

    def check(self):
        self.checks += 1


class _FakeModel:
    def __init__(self):
        self.engine = _FakeEngine()

    def prepare(self, cr_face, cr_latent):
        pass

    def prepare_slots(self, slots, cr_face, cr_latent):
        pass


@pytest.fixture
def fake(monkeypatch):
    from hifidiff_amd import sampling

    class _Stream:
        cuda_stream = STREAM
    lib = _FakeLib(B)
    monkeypatch.setattr(sampling._lib, "lib", lambda: lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    return lib


def _schedulers():
    from hifidiff_amd import schedulers
    ddim, dpm = schedulers.DDIMScheduler(clip_sample_range=3.0), schedulers.DPMSolverMultistepScheduler()
    ddim.set_timesteps(6)
    dpm.set_timesteps(5)
    return ddim, dpm


def _table(s):
    ts, coef = s.coefficient_table()
    return {"n_steps": ts.numel(), "ncoef": coef.shape[1], "timesteps": ts.tolist(), "coef": coef.flatten().tolist()}


T, F = True, False
SEEDS = [5, -1, 1 << 63]
KEYS = [5, (1 << 64) - 1, 1 << 63]            # int64 keys keep their bit pattern
# (case, scheduler, sample() arguments, expected entry point or None (no call), expected arguments besides the table)
SAMPLE_CASES = [
    ("plain7", "ddim", dict(seed=9), "hd_sample", dict(noise=None, seed=9)),
    ("plain8", "dpm", dict(seed=4), "hd_sample_multistep", dict(noise=None, seed=4)),
    ("rows7 scalar", "ddim", dict(start_steps=2), "hd_sample_rows", dict(rows=[2, 2, 2], n_iters=4, noise=None, seed=0)),
    ("rows7 per face, n_iters", "ddim", dict(start_steps=torch.tensor([1, 3, 6]), n_iters=2, seed=3), "hd_sample_rows",
     dict(rows=[1, 3, 6], n_iters=2, noise=None, seed=3)),
    ("rows8 per face", "dpm", dict(start_steps=torch.tensor([1, 3, 5])), "hd_sample_rows_multistep",
     dict(rows=[1, 3, 5], n_iters=4, resume=0, noise=None, seed=0)),
    ("rows8 scalar, n_iters, resume", "dpm", dict(start_steps=2, n_iters=1, resume=True), "hd_sample_rows_multistep",
     dict(rows=[2, 2, 2], n_iters=1, resume=1, noise=None, seed=0)),
    ("resume tensor", "dpm", dict(start_steps=torch.tensor([1, 0, 2]), resume=torch.tensor([T, F, T])), "hd_sample_faces_multistep",
     dict(rows=[1, 0, 2], n_iters=5, resume=[1, 0, 1], face_seeds=None, noise=None, seed=0)),
    ("resume tensor, no start_steps, n_iters", "dpm", dict(resume=torch.tensor([F, F, F]), n_iters=3), "hd_sample_faces_multistep",
     dict(rows=[0, 0, 0], n_iters=3, resume=[0, 0, 0], face_seeds=None, noise=None, seed=0)),
    ("face_seeds 7", "ddim", dict(face_seeds=SEEDS, seed=2), "hd_sample_faces",
     dict(rows=[0, 0, 0], n_iters=6, face_seeds=KEYS, noise=None, seed=2)),
    ("face_seeds 7, rows, n_iters", "ddim", dict(face_seeds=torch.tensor([7, 8, 9]), start_steps=torch.tensor([6, 4, 5]), n_iters=1),
     "hd_sample_faces", dict(rows=[6, 4, 5], n_iters=1, face_seeds=[7, 8, 9], noise=None, seed=0)),
    ("face_seeds 8, resume False", "dpm", dict(face_seeds=SEEDS), "hd_sample_faces_multistep",
     dict(rows=[0, 0, 0], n_iters=5, resume=[0, 0, 0], face_seeds=KEYS, noise=None, seed=0)),
    ("face_seeds 8, resume True", "dpm", dict(face_seeds=SEEDS, start_steps=1, resume=True), "hd_sample_faces_multistep",
     dict(rows=[1, 1, 1], n_iters=4, resume=[1, 1, 1], face_seeds=KEYS, noise=None, seed=0)),
    # the set's table: ddim rows [0, 6), dpm rows [6, 11); start_steps is relative to the face's own schedule
    ("set, one key", "set", dict(schedules="dpm", seed=6), "hd_sample_spans",
     dict(begin=[6, 6, 6], end=[11, 11, 11], rows=[6, 6, 6], n_iters=5, resume=[0, 0, 0], face_seeds=None, noise=None, seed=6)),
    ("set, one key, resume True", "set", dict(schedules="ddim", start_steps=2, resume=True, n_iters=1), "hd_sample_spans",
     dict(begin=[0, 0, 0], end=[6, 6, 6], rows=[2, 2, 2], n_iters=1, resume=[1, 1, 1], face_seeds=None, noise=None, seed=0)),
    ("set, per-face keys", "set", dict(schedules=["ddim", "dpm", "dpm"], start_steps=torch.tensor([2, 1, 0]),
                                       resume=torch.tensor([T, T, F]), face_seeds=SEEDS), "hd_sample_spans",
     dict(begin=[0, 6, 6], end=[6, 11, 11], rows=[2, 7, 6], n_iters=5, resume=[1, 1, 0], face_seeds=KEYS, noise=None, seed=0)),
    ("set, per-face keys, n_iters", "set", dict(schedules=["dpm", "ddim", "ddim"], start_steps=torch.tensor([5, 6, 3]), n_iters=2),
     "hd_sample_spans",
     dict(begin=[6, 0, 0], end=[11, 6, 6], rows=[11, 6, 3], n_iters=2, resume=[0, 0, 0], face_seeds=None, noise=None, seed=0)),
    # every face past its last row: nothing to run, no call
    ("all held, rows", "ddim", dict(start_steps=6), None, None),
    ("all held, rows8", "dpm", dict(start_steps=torch.tensor([5, 5, 5])), None, None),
    ("all held, faces", "ddim", dict(start_steps=6, face_seeds=SEEDS), None, None),
    ("all held, faces8", "dpm", dict(start_steps=5, resume=torch.tensor([F, F, F])), None, None),
    ("all held, set", "set", dict(schedules=["ddim", "dpm", "dpm"], start_steps=torch.tensor([6, 5, 5])), None, None),
]


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=[c[0] for c in SAMPLE_CASES])
def test_sample_calls_the_entry_point_the_rules_name(fake, case):
    from hifidiff_amd import sampling
    _, kind, kw, want_fn, want = case
    ddim, dpm = _schedulers()
    sch = {"ddim": ddim, "dpm": dpm, "set": sampling.ScheduleSet({"ddim": ddim, "dpm": dpm})}[kind]
    model = _FakeModel()
    x = torch.randn((B, 4, 16, 16), generator=torch.Generator().manual_seed(0))
    out = sampling.sample(model, x, None, None, sch, **kw)
    assert out is not x and torch.equal(out, x)                       # the fake library leaves the latents alone
    if want_fn is None:
        assert fake.calls == [] and model.engine.checks == 0
        return
    assert len(fake.calls) == 1 and model.engine.checks == 1
    name, got = fake.calls[0]
    assert name == want_fn
    assert got == dict(_table(sch), ctx=CTX, x=out.data_ptr(), stream=STREAM, **want)


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_sample_passes_explicit_noise_and_check_false(fake, kind):
    from hifidiff_amd import sampling
    sch = dict(zip(("ddim", "dpm"), _schedulers()))[kind]
    n = _table(sch)["n_steps"]
    model = _FakeModel()
    x = torch.zeros((B, 4, 16, 16))
    noise = torch.zeros((n, B, 4, 16, 16))
    out = sampling.sample(model, x, None, None, sch, noise=noise, seed=11, check=False)
    (name, got), = fake.calls
    assert name == ("hd_sample" if kind == "ddim" else "hd_sample_multistep") and model.engine.checks == 0
    assert got == dict(_table(sch), ctx=CTX, x=out.data_ptr(), stream=STREAM, noise=noise.data_ptr(), seed=11)
    fake.calls.clear()
    sampling.sample(model, x, None, None, sch, noise=noise, start_steps=torch.tensor([0, 1, 2]), face_seeds=[1, 2, 3])
    (name, got), = fake.calls
    assert name == ("hd_sample_faces" if kind == "ddim" else "hd_sample_faces_multistep")
    assert got["noise"] == noise.data_ptr() and got["rows"] == [0, 1, 2] and got["n_iters"] == n and got["face_seeds"] == [1, 2, 3]
    with pytest.raises(RuntimeError):
        sampling.sample(model, x, None, None, sch, noise=noise[1:])


def test_sample_refusals_make_no_call(fake):
    from hifidiff_amd import sampling
    ddim, dpm = _schedulers()
    x = torch.zeros((B, 4, 16, 16))
    for sch, kw in ((ddim, dict(n_iters=2)), (dpm, dict(resume=True)), (ddim, dict(start_steps=1, resume=True)),
                    (ddim, dict(face_seeds=SEEDS, resume=True)), (ddim, dict(resume=torch.tensor([F, F, F]))),
                    (ddim, dict(start_steps=torch.tensor([0, 1]))), (ddim, dict(face_seeds=[1, 2]))):
        with pytest.raises(ValueError):
            sampling.sample(_FakeModel(), x, None, None, sch, **kw)
    assert fake.calls == []


def _serve(kind, steps):
    """A batch-4 ContinuousSampler with three requests (one slot stays empty), stepped `steps` times: the recorded calls."""
    from hifidiff_amd import sampling
    ddim, dpm = _schedulers()
    sch = {"ddim": ddim, "dpm": dpm, "set": sampling.ScheduleSet({"ddim": ddim, "dpm": dpm})}[kind]
    cs = sampling.ContinuousSampler(_FakeModel(), sch, batch=4, refill_every=2)
    crf, crl = torch.zeros(3, 128, 128), torch.zeros(4, 16, 16)
    if kind == "set":
        reqs = ((21, 1.0, "ddim"), (22, 0.5, "dpm"), (23, 1.0, "dpm"))
    else:
        reqs = ((21, 1.0, None), (22, 0.5, None), (23, 0.34, None))
    for seed, strength, key in reqs:
        cs.submit(crf, crl, seed=seed, strength=strength, schedule=key)
    iters = [cs.step() for _ in range(steps)]
    return cs, sch, iters


def test_continuous_sampler_step_calls(monkeypatch, fake):
    fake.batch = 4
    common = dict(ctx=CTX, stream=STREAM, noise=None, seed=0, n_iters=2, face_seeds=[21, 22, 23, 0])
    # DDIM-6: start rows n - int(n * strength) = 0, 3, 4; the empty slot is held at row 6
    cs, sch, iters = _serve("ddim", 2)
    assert iters == [2, 2] and [n for n, _ in fake.calls] == ["hd_sample_faces"] * 2 and cs.model.engine.checks == 2
    for (_, got), rows in zip(fake.calls, ([0, 3, 4, 6], [2, 5, 6, 6])):
        got.pop("x")
        assert got == dict(_table(sch), rows=rows, **common)
    fake.calls.clear()
    # DPM-Solver++ 2M, 5 rows: 0, 5 - 2 = 3, 5 - 1 = 4; a slot that has run a row resumes its history
    cs, sch, iters = _serve("dpm", 2)
    assert iters == [2, 2] and [n for n, _ in fake.calls] == ["hd_sample_faces_multistep"] * 2
    for (_, got), rows, res in zip(fake.calls, ([0, 3, 4, 5], [2, 5, 5, 5]), ([0, 0, 0, 0], [1, 0, 0, 0])):
        got.pop("x")
        assert got == dict(_table(sch), rows=rows, resume=res, **common)
    fake.calls.clear()
    # the set: ddim rows [0, 6), dpm rows [6, 11); absolute rows 0, 6 + 3, 6; the empty slot is begin == start == end == 11
    cs, sch, iters = _serve("set", 2)
    assert iters == [2, 2] and [n for n, _ in fake.calls] == ["hd_sample_spans"] * 2 and cs.model.engine.checks == 2
    want = (dict(begin=[0, 6, 6, 11], end=[6, 11, 11, 11], rows=[0, 9, 6, 11], resume=[0, 0, 0, 0]),
            dict(begin=[0, 11, 6, 11], end=[6, 11, 11, 11], rows=[2, 11, 8, 11], resume=[1, 0, 1, 0]))
    for (_, got), w in zip(fake.calls, want):
        got.pop("x")
        assert got == dict(_table(sch), **w, **common)
    assert sorted(cs.poll()) == [1]                                   # the dpm request of strength 0.5 finished in the first call
