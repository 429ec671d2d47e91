"""The four owners of a weight context (CoarseRestoration, AutoencoderKL, LPIPS, refiner._Engine) share one implementation of the device
plumbing (hifidiff_amd/_context.py), and the GPU-only refusal is one string.  No GPU: the library is a stub that records its calls."""
import contextlib
import ctypes

import pytest
import torch

from hifidiff_amd import _context, _lib, color, metrics, photo, synth
from hifidiff_amd.cr import CoarseRestoration
from hifidiff_amd.metrics import LPIPS
from hifidiff_amd.refiner import Denoiser, _Engine
from hifidiff_amd.vae import AutoencoderKL

GPU_ONLY = "hifidiff_amd runs on an MI355X (gfx950) GPU only; got device cpu (no CPU fallback)"


def test_the_four_owners_share_the_plumbing():
    for cls in (CoarseRestoration, AutoencoderKL, LPIPS, _Engine):
        assert issubclass(cls, _context.WeightContext)
        for name in ("to", "cuda", "_ensure", "_upload", "__del__"):
            assert getattr(cls, name) is getattr(_context.WeightContext, name), (cls.__name__, name)
    assert _Engine.ensure is _context.WeightContext._ensure
    e = _Engine(16)
    e.loaded, e.ctx = True, 5                                   # the engine's names are views of the owner's fields
    assert (e._loaded, e._ctx, e.device, e.state) == (True, 5, None, None)
    e.ctx = None


def test_gpu_only_message_is_one_string():
    img = torch.zeros((1, 3, 64, 64))
    calls = [lambda: CoarseRestoration().to("cpu"), lambda: AutoencoderKL().to("cpu"), lambda: LPIPS().to("cpu"), lambda: Denoiser(16).to("cpu"),
             lambda: color.color_fix(img, img), lambda: metrics.image_range(img),
             lambda: photo.ingest(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), [[0, 0, 8, 8]])]
    for call in calls:
        with pytest.raises(RuntimeError) as err:
            call()
        assert str(err.value) == GPU_ONLY


class _StubLib:
    """The five entry points WeightContext uses; finalize fails while `fail` is set."""

    def __init__(self):
        self.calls, self.fail, self.made = [], False, 0

    def _create(self, out, idx):
        self.made += 1
        out._obj.value = 0x1000 * self.made                     # out: ctypes.byref(c_void_p)
        self.calls.append("create")
        return 0

    hd_cr_create = hd_lpips_create = _create

    def hd_destroy(self, ctx):
        self.calls.append("destroy")

    def hd_load_weights(self, ctx, descs, n):
        self.calls.append(("load", ctx.value, n, descs[0].name, descs[n - 1].name))
        return 0

    def hd_finalize_weights(self, ctx):
        self.calls.append("finalize")
        return -3 if self.fail else 0

    def hd_last_error(self, ctx):
        return b"stub: finalize failed"


@pytest.fixture
def stub(monkeypatch):
    s = _StubLib()
    monkeypatch.setattr(_lib, "lib", lambda: s)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    return s


@pytest.mark.parametrize("cls,state", [(CoarseRestoration, synth.cr_state_dict), (LPIPS, synth.lpips_state_dict)])
def test_reload_is_unusable_until_finalize_succeeds(stub, cls, state):
    sd = state()
    m = cls()
    try:
        m.load_state_dict(sd)
        assert stub.calls == [] and not m._loaded               # no context yet: nothing is uploaded
        m.to("cuda:0")
        first = m._ctx.value
        assert [c if isinstance(c, str) else c[0] for c in stub.calls] == ["create", "load", "finalize"] and m._loaded
        load = stub.calls[1]
        assert load[1] == first and load[2] == len(sd) and load[3] == next(iter(m._items()))[0].encode()
        with pytest.raises(RuntimeError, match="already lives on cuda:0"):
            m.to("cuda:1")
        if cls is CoarseRestoration:
            m._batch = 4
        del stub.calls[:]
        stub.fail = True
        with pytest.raises(_lib.HipError, match="stub: finalize failed"):
            m.load_state_dict(sd)                               # a finalized context is replaced, and the new one fails to finalize
        assert [c if isinstance(c, str) else c[0] for c in stub.calls] == ["destroy", "create", "load", "finalize"]
        assert not m._loaded and m._ctx.value != first and getattr(m, "_batch", None) is None
        del stub.calls[:]
        stub.fail = False
        m.load_state_dict(sd)                                   # not finalized: the same context takes the weights again
        assert [c if isinstance(c, str) else c[0] for c in stub.calls] == ["load", "finalize"] and m._loaded
    finally:
        m._ctx = None                                           # nothing for __del__ to hand to the real library
