"""Every selectable form of the refiner's step program (build_denoiser_program, hd_lib.hip) against the bf16-emulating oracle.

The creation-time switches (HD_NO_DOWN_FOLD, HD_NO_UP_FOLD, HD_NO_END_FOLD, HD_FACE_L1_ROWS, HD_NO_FACE, HD_XCD2, HD_CHAINS) each build
another program for the same network, and each is also the fallback path of a refused launch.  Per variant, on a fresh context:
eps at batch 64 (t = 999 / 500 / 0 and a timestep per face) and at batch 3 against the oracle, the same inputs again after a call on
other inputs (a stage that reads a buffer no launch of this call wrote fails one of the two orders), the launch count and the fold
getters, and 24 DDPM / 20 DPM-Solver++ 2M graph-replayed steps against the default program.  Then the run-time switches of one
context (hd_set_option), and the getters of the shapes the folds do not apply to (latent 32, the unconditional Denoiser, batch 65).
"""
import gc
import os

import numpy as np
import pytest
import torch

from conftest import psnr, rel_l2, weights16  # noqa: F401  (weights16: session fixture)

pytestmark = pytest.mark.gpu

FOLDS = (b"intro_fold", b"down_fold", b"up_fold", b"end_fold")

# Launch counts at batch 64, from build_denoiser_program.  With one launch per GEMM (HD_NO_XCD=1) the program has 151 launches:
# intro, 4 downs, 4 ups, 5 hcas, ending, the conditioning adds, and per ConditionalNAFBlock 2 launches at levels 0 / 1 (8 blocks,
# 16 launches) and 5 at levels 2 / 3 (16 blocks, 80 launches).  The XCD-local stages make the 80 four launches (151 - 76 = 75:
# HD_NO_FACE=1).  The face-cluster stages make the 16 four (75 - 12 = 63: HD_NO_INTRO_FOLD=1, which turns every fold off).  Each fold
# then removes one launch: intro (the level-0 encoder stage's entry), downs.0 (the level-1 encoder stage's entry), ups.3 (the level-0
# decoder stage's entry) and hcas.4 (one launch with the ending conv): 63 - 4 = 59, the default.  A single fold turned off adds its
# launch back: 60.  HD_FACE_L1_ROWS=32 picks naf_face_stage_kernel<256,32>, which has no down-conv entry: downs.0 stays a launch (60).
# HD_XCD2 picks the form of the XCD-local stages, not their number (59).  HD_CHAINS=2 builds the batch-64 program per chain of 32
# faces (59 each); the persistent stages step aside at run time (every workgroup must be resident), the ops run their per-launch form.
VARIANTS = {
    # name: (environment, launches at batch 64, chains, getters that differ from the default)
    "default": ({}, 59, 1, {}),
    "no_down_fold": ({"HD_NO_DOWN_FOLD": "1"}, 60, 1, {b"down_fold": 0}),
    "no_up_fold": ({"HD_NO_UP_FOLD": "1"}, 60, 1, {b"up_fold": 0}),
    "no_end_fold": ({"HD_NO_END_FOLD": "1"}, 60, 1, {b"end_fold": 0}),
    "face_l1_rows_32": ({"HD_FACE_L1_ROWS": "32"}, 60, 1, {b"down_fold": 0, b"face_l1_rows": 32}),
    "face_l1_rows_32_no_down_fold": ({"HD_FACE_L1_ROWS": "32", "HD_NO_DOWN_FOLD": "1"}, 60, 1, {b"down_fold": 0, b"face_l1_rows": 32}),
    # no face stages: nothing to fold the intro / downs.0 / ups.3 into, and the fused ending is built only with them
    "no_face": ({"HD_NO_FACE": "1"}, 75, 1, {b"intro_fold": 0, b"down_fold": 0, b"up_fold": 0, b"end_fold": 0, b"face_stages": 0}),
    "xcd2_0": ({"HD_XCD2": "0"}, 59, 1, {b"xcd2": 0}),
    "xcd2_2": ({"HD_XCD2": "2"}, 59, 1, {b"xcd2": 2}),
    # two chains: the face-stage entries do not run (their producers run as launches inside the same ops), the fused ending does
    "chains_2": ({"HD_EXPERIMENTS": "1", "HD_CHAINS": "2"}, 59, 2, {b"intro_fold": 0, b"down_fold": 0, b"up_fold": 0}),
}
DEFAULT_GETTERS = {b"intro_fold": 1, b"down_fold": 1, b"up_fold": 1, b"end_fold": 1, b"face_l1_rows": 16, b"xcd2": 1, b"face_stages": 4}
SWITCHES = sorted({k for env, _, _, _ in VARIANTS.values() for k in env} | {"HD_NO_XCD", "HD_NO_INTRO_FOLD"})
TS = (999, 500, 0)
EPS_TOL, FACE_TOL = 6e-3, 8e-3            # test_eps_at_the_benchmark_batch_against_oracle
TRAJ_TOL = 1e-2                           # test_folded_transitions_against_their_launches
OTHER_SEED = 0x0DDBA11


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


class _env:
    """The switches of one variant, and none of the others, while the block runs."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in SWITCHES:
            os.environ.pop(k, None)
            if self.saved[k] is not None:
                os.environ[k] = self.saved[k]


def make_model(weights, latent=16):
    from hifidiff_amd.refiner import FacialRefiner
    m = FacialRefiner(latent)
    m.load_state_dict(weights)
    m.to("cuda:0")
    return m


def free(m):
    del m
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _L():
    from hifidiff_amd import _lib
    return _lib.lib()


def _opt(m, key, v):
    from hifidiff_amd import _lib
    _lib.check(_L().hd_set_option(m.engine.ctx, key.encode(), int(v)), m.engine.ctx)


def getters(m, keys=FOLDS):
    return {k: _L().hd_get_option(m.engine.ctx, k) for k in keys}


def op_names(m):
    L = _L()
    return [L.hd_debug_op_name(m.engine.ctx, 0, i).decode() for i in range(L.hd_num_ops(m.engine.ctx, 0))]


def folds_from_names(names, conditional=True):
    """What the program does, read from its op list: a folded producer has no launch of its own."""
    return {b"intro_fold": int("intro" not in names), b"down_fold": int("downs.0" not in names), b"up_fold": int("ups.3" not in names),
            b"end_fold": int(conditional and "hcas.4" not in names)}


def _cuda(*ts):
    return [t.cuda() for t in ts]


@pytest.fixture(scope="module")
def data(gpu):
    from hifidiff_amd import synth
    x, crl, crf = synth.sample_inputs(64, 16)
    xa, crla, crfa = synth.sample_inputs(64, 16, seed=OTHER_SEED)
    return {"B": (x, crl, crf), "A": (xa, crla, crfa), "tf": (torch.arange(64) * 37 % 1000).float(),
            "noise": torch.randn((24, 64, 4, 16, 16), generator=torch.Generator().manual_seed(11))}


@pytest.fixture(scope="module")
def refs(gpu, weights16, data):
    """The oracle's eps (bf16 operands) of the inputs B, computed once for every variant."""
    from oracle import hifidiff_oracle as O
    x, crl, crf = data["B"]
    cond = O.Conditioning(weights16, crl, crf, prec=O.BF16)
    r = {t: O.fused_denoiser(weights16, x, t, cond=cond, prec=O.BF16) for t in TS}
    r["tf"] = O.fused_denoiser(weights16, x, data["tf"], cond=cond, prec=O.BF16)
    cond3 = O.Conditioning(weights16, crl[:3], crf[:3], prec=O.BF16)
    r["b3"] = O.fused_denoiser(weights16, x[:3], 500, cond=cond3, prec=O.BF16)
    return r


def _ddpm24(m, x, crl, crf, noise):
    from hifidiff_amd import sampling, schedulers
    sch = schedulers.DDPMScheduler(clip_sample_range=3.0)
    sch.timesteps = sch.timesteps[:24]
    return sampling.sample(m, x, crf, crl, sch, noise=noise).cpu()


def _dpm20(m, x, crl, crf):
    from hifidiff_amd import sampling, schedulers
    sch = schedulers.DPMSolverMultistepScheduler()
    sch.set_timesteps(20)
    return sampling.sample(m, x, crf, crl, sch).cpu()


def _dpm20_eager(m, x, crl, crf):
    """One model(...) + scheduler.step(...) per step: the history term is kept by the Python scheduler."""
    from hifidiff_amd import schedulers
    sch = schedulers.DPMSolverMultistepScheduler()
    sch.set_timesteps(20)
    for t in sch.timesteps:
        x = sch.step(m(x, int(t), crf, crl).sample, t, x).prev_sample
    return x.cpu()


@pytest.fixture(scope="module")
def default_traj(gpu, weights16, data):
    """The default program's trajectories (its eps against the oracle is the "default" row below)."""
    x, crl, crf = _cuda(*data["B"])
    with _env({}):
        m = make_model(weights16)
        m(x, 500, crf, crl)
    out = {"ddpm": _ddpm24(m, x, crl, crf, data["noise"].cuda()), "dpm": _dpm20(m, x, crl, crf)}
    free(m)
    return out


def _eps_errors(e, ref):
    e = e.cpu()
    return rel_l2(e, ref), max(rel_l2(e[f], ref[f]) for f in range(e.shape[0]))


@pytest.mark.parametrize("name", list(VARIANTS))
def test_variant_against_oracle_and_default(gpu, weights16, data, refs, default_traj, name):
    env, n_ops, n_chains, changed = VARIANTS[name]
    L = _L()
    x, crl, crf = _cuda(*data["B"])
    xa, crla, crfa = _cuda(*data["A"])
    err = {}
    with _env(env):                                                   # creation and the first call at each batch size
        m = make_model(weights16)
        err["fresh t500"] = _eps_errors(m(x, 500, crf, crl).sample, refs[500])
        err["b3 fresh"] = _eps_errors(m(x[:3], 500, crf[:3], crl[:3]).sample, refs["b3"])
    m(xa[:3], 500, crfa[:3], crla[:3])
    err["b3 after A"] = _eps_errors(m(x[:3], 500, crf[:3], crl[:3]).sample, refs["b3"])
    for t in TS:
        err[f"t{t}"] = _eps_errors(m(x, t, crf, crl).sample, refs[t])
    err["per-face t"] = _eps_errors(m(x, data["tf"].cuda(), crf, crl).sample, refs["tf"])
    m(xa, 500, crfa, crla)
    err["after A"] = _eps_errors(m(x, 500, crf, crl).sample, refs[500])
    print(f"\n[{name}] worst eps rel-L2 vs oracle: {max(v[0] for v in err.values()):.3e} (per face {max(v[1] for v in err.values()):.3e}); "
          + ", ".join(f"{k} {v[0]:.2e}" for k, v in err.items()))
    for k, (whole, face) in err.items():
        assert whole <= EPS_TOL and face <= FACE_TOL, (name, k, whole, face)

    # the program that ran (batch 64 is the workspace in use again)
    want = {**DEFAULT_GETTERS, **changed}
    got = getters(m, tuple(want))
    assert (L.hd_num_ops(m.engine.ctx, 0), L.hd_num_chains(m.engine.ctx)) == (n_ops, n_chains), name
    assert got == want, (name, got)
    if n_chains == 1 and want[b"face_stages"]:
        assert got == {**got, **folds_from_names(op_names(m))}, (name, got, op_names(m))

    # trajectories against the default program's
    ddpm = _ddpm24(m, x, crl, crf, data["noise"].cuda())
    dpm = _dpm20(m, x, crl, crf)
    hist = np.zeros(dpm.numel(), np.float32)
    assert L.hd_debug_read(m.engine.ctx, b"x0_hist", hist.ctypes.data, hist.size) == hist.size
    rd, rm = rel_l2(ddpm, default_traj["ddpm"]), rel_l2(dpm, default_traj["dpm"])
    print(f"[{name}] vs default program: DDPM 24 steps {rd:.3e}, DPM-Solver++ 2M 20 steps {rm:.3e}")
    assert bool(torch.isfinite(ddpm).all()) and bool(torch.isfinite(dpm).all()), name
    assert rd <= TRAJ_TOL and rm <= TRAJ_TOL, (name, rd, rm)
    if name == "default":
        assert torch.equal(ddpm, default_traj["ddpm"]) and torch.equal(dpm, default_traj["dpm"])
    if name in ("chains_2", "no_end_fold"):
        # the history term: x0_hist per chain / in the two-launch ending against the Python scheduler's (test_multistep.py bound);
        # row 0 has c7 = 0, so the 20 steps exercise it from step 1 on
        assert np.array_equal(hist.reshape(dpm.shape), dpm.numpy()), name     # the last step lands on x0, which the history holds
        eager = _dpm20_eager(m, x, crl, crf)
        assert psnr(eager, dpm) >= 50.0, (name, psnr(eager, dpm))
    free(m)


def test_runtime_switches_against_the_default_trajectory(gpu, weights16, data, default_traj):
    """hd_set_option "xcd" / "xcd2" / "face" on a live context: the captured graphs are re-captured with the other form of the
    same ops, the trajectory stays within the bound of the default one, and restoring the option restores its bits."""
    x, crl, crf = _cuda(*data["B"])
    noise = data["noise"].cuda()
    with _env({}):
        m = make_model(weights16)
        m(x, 500, crf, crl)
    base = _ddpm24(m, x, crl, crf, noise)
    assert torch.equal(base, default_traj["ddpm"])
    # what each switch turns off, as the getters report it (the face-stage entries go with the face stages; the fused ending stays)
    reports = {"xcd": {b"xcd": 0, **dict.fromkeys(FOLDS, 1)}, "xcd2": {b"xcd2": 0, **dict.fromkeys(FOLDS, 1)},
               "face": {b"intro_fold": 0, b"down_fold": 0, b"up_fold": 0, b"end_fold": 1}}
    for key, want in reports.items():
        _opt(m, key, 0)
        got = _ddpm24(m, x, crl, crf, noise)
        off = getters(m, tuple(want))
        _opt(m, key, 1)
        r = rel_l2(got, base)
        print(f"\n[{key} = 0] DDPM 24 steps vs default: {r:.3e}")
        assert off == want and bool(torch.isfinite(got).all()) and r <= TRAJ_TOL, (key, off, r)
        assert torch.equal(_ddpm24(m, x, crl, crf, noise), base), key
        assert getters(m) == dict.fromkeys(FOLDS, 1), key
    free(m)


def test_fold_getters_report_the_built_program(gpu, weights16):
    """Batch 65 (one launch per GEMM), latent 32 and the unconditional Denoiser have no folds; the getters must say so, and must say
    it again when the context goes back to batch 64."""
    from hifidiff_amd import synth
    from hifidiff_amd.refiner import Denoiser
    L = _L()
    with _env({}):
        m = make_model(weights16)
        x, crl, crf = _cuda(*synth.sample_inputs(65, 16))
        m(x[:64], 500, crf[:64], crl[:64])
        assert getters(m) == dict.fromkeys(FOLDS, 1) and L.hd_num_ops(m.engine.ctx, 0) == 59
        m(x, 500, crf, crl)
        assert L.hd_num_ops(m.engine.ctx, 0) == 151
        assert getters(m) == dict.fromkeys(FOLDS, 0) == folds_from_names(op_names(m))
        m(x[:64], 500, crf[:64], crl[:64])
        assert getters(m) == dict.fromkeys(FOLDS, 1)
        free(m)

        n = len("denoiser.")
        u = Denoiser(16)
        u.load_state_dict({k[n:]: v for k, v in weights16.items() if k.startswith("denoiser.") and ".hcas." not in k and ".idc_conv" not in k})
        u.to("cuda:0")
        xu = x[:2]
        assert bool(torch.isfinite(u(xu, 500).sample).all())
        g = getters(u)
        assert g[b"end_fold"] == 0 and g == folds_from_names(op_names(u), conditional=False), g
        free(u)

        w32 = synth.refiner_state_dict(32)
        m32 = make_model(w32, 32)
        x, crl, crf = _cuda(*synth.sample_inputs(2, 32))
        assert bool(torch.isfinite(m32(x, 500, crf, crl).sample).all())
        g = getters(m32)
        assert g == dict.fromkeys(FOLDS, 0) == folds_from_names(op_names(m32)), g
        free(m32)
