"""What every wrapper of a weight context shares: the GPU-only check, the stream pointer, the face-image shape check, and
`WeightContext`, the one owner of an `hd_ctx` (create, upload, finalize, replace on re-load, destroy)."""
import torch

from . import _lib


def require_cuda(device):
    if device.type != "cuda":
        raise RuntimeError("hifidiff_amd runs on an MI355X (gfx950) GPU only; got device %s (no CPU fallback)" % device)


def stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


def check_face_images(name, t):
    if t.dim() != 4 or t.shape[1] != 3 or t.shape[2] != t.shape[3] or t.shape[2] % 64 or not 64 <= t.shape[2] <= 512:
        raise ValueError("%s must be (B,3,R,R) with R a multiple of 64 in [64, 512], got %s" % (name, tuple(t.shape)))


class WeightContext:
    """Owns one hd_ctx on one device.  A subclass says how to create it (`_create(idx)`), which tensors it takes (`_manifest()`, or
    `_items()` itself) and what else a replaced context invalidates (`_reset()`)."""

    def __init__(self):
        super().__init__()
        self._ctx, self._device, self._state, self._loaded, self._keep = None, None, None, False, None

    def _create(self, idx):
        raise NotImplementedError

    def _manifest(self):
        raise NotImplementedError

    def _items(self):
        """The (name, tensor) pairs to upload, in order."""
        man = self._manifest()
        if any(k not in self._state for k in man):
            raise RuntimeError("state dict incomplete: %d of %d tensors loaded" % (len(self._state), len(man)))
        return [(k, self._state[k]) for k in man]

    def _reset(self):
        """Forget what was derived from the weights of the context that has just been replaced or re-loaded."""

    def to(self, *args, **kwargs):
        device = kwargs.get("device", args[0] if args else None)
        if isinstance(device, (str, torch.device, int)):
            self._ensure(torch.device("cuda", device) if isinstance(device, int) else device)
        return self

    def cuda(self, device=None):
        return self.to(torch.device("cuda", device if device is not None else torch.cuda.current_device()))

    def _ensure(self, device):
        device = torch.device(device)
        require_cuda(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._ctx is not None:
            if idx != self._device.index:
                raise RuntimeError("this model already lives on cuda:%d" % self._device.index)
            return
        self._ctx, self._device = self._create(idx), torch.device("cuda", idx)
        if self._state is not None:
            self._upload()

    def _upload(self):
        items = self._items()
        L = _lib.lib()
        keep, descs = [], (_lib.TensorDesc * len(items))()
        for d, (k, t) in zip(descs, items):
            if t.dtype != torch.int64:
                t = t.to(torch.float32)
            t = t.contiguous()
            keep.append(t)
            d.name, d.data, d.ndim, d.is_device = k.encode(), t.data_ptr(), t.dim(), 1 if t.is_cuda else 0
            for j, s in enumerate(t.shape):
                d.shape[j] = s
        if self._loaded:                     # re-load: weights are packed once per context, so it is replaced
            L.hd_destroy(self._ctx)
            self._ctx = None
            self._loaded = False             # nothing usable until finalize has succeeded
            self._reset()
            self._ctx = self._create(self._device.index)
        with torch.cuda.device(self._device):
            _lib.check(L.hd_load_weights(self._ctx, descs, len(items)), self._ctx)
            _lib.check(L.hd_finalize_weights(self._ctx), self._ctx)
        self._loaded = True
        self._reset()

    def __del__(self):
        try:
            if self._ctx is not None:
                _lib.lib().hd_destroy(self._ctx)
        except Exception:
            pass
