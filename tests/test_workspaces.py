"""Batch workspaces (hd_internal.hpp: struct Workspace, switch_workspace): one context keeps the workspace of the batch in use and parks up
to three others -- buffers, launch programs and captured graphs travel together and come back as they were.  Every comparison is bit for
bit: a workspace that is taken back, or built again after its eviction, runs the same launches on the same inputs.  Latent 16, at most 5
faces, 3 DDIM steps."""
import numpy as np
import pytest
import torch

from conftest import weights16  # noqa: F401  (session fixture)

pytestmark = pytest.mark.gpu

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    torch.set_grad_enabled(False)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def inputs(gpu):
    from hifidiff_amd import synth
    x, crl, crf = [t.cuda() for t in synth.sample_inputs(6, 16)]
    return x, crl, crf


def _L():
    from hifidiff_amd import _lib
    return _lib.lib()


def make_model(weights):
    from hifidiff_amd.refiner import FacialRefiner
    m = FacialRefiner(16)
    m.load_state_dict(weights)
    m.to("cuda:0")
    return m


def _schedule():
    from hifidiff_amd import schedulers
    sch = schedulers.DDIMScheduler(clip_sample_range=3.0)
    sch.set_timesteps(50)
    sch.timesteps = sch.timesteps[:3]
    return sch


def _sample(m, inputs, B):
    from hifidiff_amd import sampling
    x, crl, crf = inputs
    return sampling.sample(m, x[:B], crf[:B], crl[:B], _schedule())


def _captures(m):
    return _L().hd_get_option(m.engine.ctx, b"graph_captures")


def _numel(m, name):
    n = _L().hd_debug_read(m.engine.ctx, name.encode(), None, 0)
    assert n >= 0, (name, n)
    return n


def test_eviction_and_return(gpu, weights16, inputs):
    """Batches 1..5 through one model: three workspaces are parked at most, so some are destroyed on the way; then batch 2, batch 1 and
    batch 5 again.  Every repeat equals its first run.  graph_captures counts the step graphs instantiated (capture_step_graphs: the
    one-step and the multi-step graph of the one chain): 2 on the first use of a batch size, 2 when a destroyed workspace is built again,
    0 when a parked one is taken back."""
    m = make_model(weights16)
    first, grew = {}, []
    for B in (1, 2, 3, 4, 5):
        before = _captures(m)
        first[B] = _sample(m, inputs, B).clone()
        grew.append(_captures(m) - before)
    again = {}
    for B in (2, 1, 5):
        before = _captures(m)
        again[B] = _sample(m, inputs, B)
        grew.append(_captures(m) - before)
    print("graph_captures grew by", grew)
    for B in again:
        assert torch.equal(again[B], first[B]), B
    # The active workspace is parked before the one asked for is looked up, and the least recently used beyond three is destroyed at that
    # point.  So batch 5 destroys batch 1's, the return to batch 2 finds 2, 3, 4, 5 parked and destroys its own (the oldest) before it looks,
    # and the return to batch 1 destroys batch 3's: both are built and captured again.  Batch 5, parked since, is then taken back with its
    # graphs.  (These are the counts of the build before struct Workspace; the switch keeps that order.)
    assert grew == [2, 2, 2, 2, 2, 2, 2, 0], grew


def test_option_switch_invalidates_parked_graphs(gpu, weights16, inputs):
    """Batch 4, then batch 3, then hd_set_option("xcd", 0) while batch 4's workspace is parked, then batch 4: its graphs captured the
    persistent stages and must be captured again.  Equal to a fresh model that had the option before its first call."""
    from hifidiff_amd import _lib
    m = make_model(weights16)
    _sample(m, inputs, 4); _sample(m, inputs, 3)
    _lib.check(_L().hd_set_option(m.engine.ctx, b"xcd", 0), m.engine.ctx)
    before = _captures(m)
    got = _sample(m, inputs, 4)
    assert _captures(m) - before == 2
    fresh = make_model(weights16)
    _lib.check(_L().hd_set_option(fresh.engine.ctx, b"xcd", 0), fresh.engine.ctx)
    assert torch.equal(got, _sample(fresh, inputs, 4))


def test_staging_chain_travels_with_its_workspace(gpu, weights16, inputs):
    """hd_prepare_slots runs on a private chain of the workspace.  Prepare batch 4, refill slot 2, sample; a batch-2 call parks that
    workspace; the same prepare, refill and sampling afterwards give the first result."""
    from hifidiff_amd import sampling
    x, crl, crf = inputs
    m = make_model(weights16)

    def run():
        m.prepare(crf[:4], crl[:4])
        m.prepare_slots([2], crf[5:6], crl[5:6])
        return sampling.sample(m, x[:4], None, None, _schedule(), prepare=False).clone()
    a = run()
    _sample(m, inputs, 2)
    b = run()
    assert torch.equal(a, b)
    assert not torch.equal(a[2], _sample(m, inputs, 4)[2])            # the refill did change slot 2


def test_debug_names_follow_the_workspace(gpu, weights16, inputs):
    """The per-batch debug names belong to the workspace in use, `film` to the context: batch 3, then 2, then 3 again."""
    m = make_model(weights16)
    film = None
    for B in (3, 2, 3):
        _sample(m, inputs, B)
        assert _numel(m, "X0") == B * 16 * 16 * 128
        assert _numel(m, "lat") == B * 4 * 16 * 16
        film = film or _numel(m, "film")
        assert film > 0 and _numel(m, "film") == film


def test_vae_program_travels_with_its_workspace(gpu):
    """The VAE's workspaces are keyed by (batch, resolution); encode at 64 px and decode at latent 8 share one.  Encode batch 1 at 64 px,
    encode batch 2, decode batch 1 at latent 8, encode at 128 px, then the first encode again with the same tensors: the same latents."""
    from hifidiff_amd import _lib, synth
    from hifidiff_amd.vae import AutoencoderKL
    v = AutoencoderKL()
    v.load_state_dict(synth.vae_state_dict())
    v.to("cuda:0")
    img = {(B, R): T(np.stack([synth.rand(f"cr_face_vae/{f}", (3, R, R)) for f in range(B)])).cuda() for B, R in ((1, 64), (2, 64), (1, 128))}
    noise = T(synth.randn("vae_noise/0", (4, 8, 8))[None]).cuda()
    out = {k: torch.zeros(k[0], 4, k[1] // 8, k[1] // 8, device="cuda") for k in img}
    v._ready(img[1, 64])
    stream = torch.cuda.current_stream().cuda_stream

    def encode(B, R, nz):
        _lib.check(_L().hd_vae_encode(v._ctx, B, R, R, img[B, R].data_ptr(), 0, nz.data_ptr() if nz is not None else None, 0, None,
                                      out[B, R].data_ptr(), stream), v._ctx)
        return out[B, R]
    first = encode(1, 64, noise).clone()
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
    encode(2, 64, None)
    dec = v.decode_scaled(first)
    assert tuple(dec.shape) == (1, 3, 64, 64) and bool(torch.isfinite(dec).all())
    encode(1, 128, None)
    out[1, 64].zero_()
    assert torch.equal(encode(1, 64, noise), first)
