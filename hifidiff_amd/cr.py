"""Drop-in mirror of `CoarseRestoration` (models/cr/model.py:33-88) — the network that turns the low-quality face
into `cr_face` before the diffusion loop (`cr_face = cr_module(ln_face)`, test_refiner.py:77; infer_cr.py:48-60).
SURVEY §8 f1.

Same constructor (no arguments), `load_state_dict` with the reference's keys (`torch.load(ckpt)["model_state_dict"]`,
test_refiner.py:180), `.eval()`, `.to(device)`, `forward(x) -> tensor`.  All compute runs in libhifidiff_hip.so
(`hd_cr_create` / `hd_cr_forward`): the 32 NAF blocks, down- and up-convs on the refiner path's kernels, the STN
(localisation net in fp32, affine bilinear resampling) and the 3<->32 channel image convs on the kernels of
csrc/hd_cr.hpp.  There is no CPU path.
"""
import ctypes

import torch
from torch import nn

from . import _lib, arch
from ._context import WeightContext, stream_ptr


class CoarseRestoration(WeightContext, nn.Module):
    def __init__(self):
        super().__init__()
        self._batch = None

    def load_state_dict(self, state_dict, strict=True):
        man = arch.cr_manifest()
        missing = [k for k in man if k not in state_dict]
        unexpected = [k for k in state_dict if k not in man]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for CoarseRestoration: Missing key(s): %s; Unexpected key(s): %s"
                               % (missing[:4], unexpected[:4]))
        for k, (shape, _, _) in man.items():
            if k in state_dict and tuple(state_dict[k].shape) != tuple(shape):
                raise RuntimeError("size mismatch for %s: got %s, expected %s" % (k, tuple(state_dict[k].shape), tuple(shape)))
        base = self._state or {}
        self._state = {k: (state_dict[k] if k in state_dict else base[k]).detach() for k in man if (k in state_dict or k in base)}
        if self._ctx is not None:
            self._upload()                                 # a context whose weights are finalized is replaced (self._loaded)
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def state_dict(self, *a, **k):
        return dict(self._state or {})

    # ---- library plumbing (_context.WeightContext) ----
    _manifest = staticmethod(arch.cr_manifest)

    def _create(self, idx):
        ctx = ctypes.c_void_p()
        _lib.check(_lib.lib().hd_cr_create(ctypes.byref(ctx), idx))
        return ctx

    def _reset(self):
        self._batch = None

    def forward(self, x):
        self._ensure(x.device)
        if not self._loaded:
            raise RuntimeError("weights are not loaded: call load_state_dict(...) and move the model to a cuda device")
        B = x.shape[0]
        if tuple(x.shape) != (B, 3, 128, 128):
            raise RuntimeError("CoarseRestoration input must be (B,3,128,128), got %s" % (tuple(x.shape),))
        if B == 0:
            return torch.empty_like(x, dtype=torch.float32)
        self._batch = B                                        # any batch size: the library keeps a workspace per recent size
        xin = x.to(device=self._device, dtype=torch.float32).contiguous()
        out = torch.empty_like(xin)
        with torch.cuda.device(self._device):
            _lib.check(_lib.lib().hd_cr_forward(self._ctx, B, xin.data_ptr(), out.data_ptr(),
                                                stream_ptr(self._device)), self._ctx)
        self._keep = (xin, out)              # the launch program holds these pointers until the next call
        return out
