"""Per-face PSNR, SSIM and LPIPS of images against a reference: the scores of the reference's evaluation loop (`val_loop`,
test_refiner.py:107-123: F.interpolate to the target's size, min-max normalise, pyiqa's psnr, ssim and lpips).  NIQE needs a fitted
model file and is not offered.  pyiqa and the `lpips` package are absent, so parity with their defaults is unpinned, like the
schedulers'; the formulas in include/hifidiff_hip.h (hd_image_metrics, hd_lpips) are the contract.

`image_metrics`, `image_range` and `evaluate` run in libhifidiff_hip.so (hd_image_metrics: a fused windowed-moment stencil and a
fixed-order fp64 reduction, GPU only, bit-reproducible and independent of a face's position in the batch).  The `*_reference` functions
state the same formulas in plain torch, in any dtype and on any device: the role `color.*_reference` play for the colour fix.

`LPIPS` is a module-shaped object in the style of `vae.AutoencoderKL` (AlexNet, v0.1 lin weights, hd_lpips); `lpips_reference` states its
contract in plain torch.  The weights come from the caller (`load_state_dict`, `from_files`) or, for tests, from `synth`."""
import collections
import ctypes
import math

import torch
import torch.nn.functional as F

from . import _lib, arch
from ._context import WeightContext, check_face_images, require_cuda, stream_ptr

CHANNELS = {"rgb": 1, "y": 2}
NORMALIZE = (None, "face", "batch")
WINDOW, SIGMA = 11, 1.5

Metrics = collections.namedtuple("Metrics", "mse psnr ssim ssim_map lpips", defaults=(None,))
Metrics.__doc__ = ("Per-face scores: mse, psnr, ssim are [B]; ssim_map is [B,P,Rb-10,Rb-10] (P = 3 for rgb, 1 for y) or None; lpips is [B] "
                   "where a loaded LPIPS model was given, else None.")


# ------------------------------------------------------------------------------------------------ reference formulas, plain torch
def gaussian_window(dtype=torch.float64, device=None):
    """g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1 in float64 and then cast."""
    k = torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2
    g = torch.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype=dtype, device=device)


def window_blur(x, window=None):
    """The separable window over the "valid" positions of every plane of [B,C,H,W]: a horizontal then a vertical pass; [B,C,H-10,W-10]."""
    g = gaussian_window(x.dtype, x.device) if window is None else window
    C, n = x.shape[1], g.numel()
    x = F.conv2d(x, g.reshape(1, 1, 1, n).repeat(C, 1, 1, 1), groups=C)
    return F.conv2d(x, g.reshape(1, 1, n, 1).repeat(C, 1, 1, 1), groups=C)


def rgb_to_y(x, data_range=1.0):
    """BT.601 studio luma of [B,3,H,W], as basicsr / pyiqa: (65.481 R + 128.553 G + 24.966 B + 16 L) / 255; [B,1,H,W]."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("rgb_to_y needs (B,3,H,W), got %s" % (tuple(x.shape),))
    return (65.481 * x[:, 0:1] + 128.553 * x[:, 1:2] + 24.966 * x[:, 2:3] + 16.0 * data_range) / 255.0


def _check_pair(a, b):
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape):
        raise ValueError("the two images must be (B,C,H,W) of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))


def ssim_map_reference(a, b, data_range=1.0):
    """The SSIM map of Wang et al. 2004 per plane over the valid window positions; [B,C,H-10,W-10]."""
    _check_pair(a, b)
    b = b.to(a.dtype)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    g = gaussian_window(a.dtype, a.device)
    mua, mub = window_blur(a, g), window_blur(b, g)
    va, vb, cab = window_blur(a * a, g) - mua * mua, window_blur(b * b, g) - mub * mub, window_blur(a * b, g) - mua * mub
    return ((2 * mua * mub + C1) * (2 * cab + C2)) / ((mua * mua + mub * mub + C1) * (va + vb + C2))


def ssim_reference(a, b, data_range=1.0):
    """Per face: the mean of the map over planes and positions; [B]."""
    return ssim_map_reference(a, b, data_range).mean(dim=(1, 2, 3))


def mse_reference(a, b):
    """Per face: the mean of (a - b)^2 over planes and pixels; [B]."""
    _check_pair(a, b)
    d = a - b.to(a.dtype)
    return (d * d).mean(dim=(1, 2, 3))


def psnr_from_mse(mse, data_range=1.0):
    """10 log10(L^2 / mse); +inf where mse == 0."""
    return 10.0 * torch.log10((data_range * data_range) / mse)


def psnr_reference(a, b, data_range=1.0):
    return psnr_from_mse(mse_reference(a, b), data_range)


def resample(images, size):
    """F.interpolate(mode="bicubic", align_corners=False) to size x size; the tensor itself when it has that size."""
    if size is None or int(size) == images.shape[-1] == images.shape[-2]:
        return images
    return F.interpolate(images, size=(int(size), int(size)), mode="bicubic", align_corners=False)


def range_reference(images, size=None):
    """Per face: (min, max) over channels and pixels of the images resampled to `size`; [B,2]."""
    x = resample(images, size)
    return torch.stack([x.amin(dim=(1, 2, 3)), x.amax(dim=(1, 2, 3))], dim=1)


def normalize_reference(x, rng):
    """(x - lo) / (hi - lo) with rng [B,2]; 0 for a face with hi <= lo (torch's own expression gives NaN there)."""
    lo, hi = rng[:, 0].reshape(-1, 1, 1, 1), rng[:, 1].reshape(-1, 1, 1, 1)
    ok = hi > lo
    return torch.where(ok, (x - lo) / torch.where(ok, hi - lo, torch.ones_like(hi)), torch.zeros_like(x))


def _batch_range(rng):
    return torch.stack([rng[:, 0].amin(), rng[:, 1].amax()]).expand(rng.shape[0], 2).contiguous()


def image_metrics_reference(images, ref, channels="y", data_range=1.0, normalize=None, ssim_map=False):
    """What `image_metrics` computes, from torch ops in the dtype and on the device of `images`: resample to ref's size, normalise,
    reduce to the scored planes, MSE / PSNR / SSIM per face."""
    _check_mode(channels, data_range, normalize)
    a, b = resample(images, ref.shape[-1]), ref.to(images.dtype)
    if normalize is not None:
        ra, rb = range_reference(a), range_reference(b)
        if normalize == "batch":
            ra, rb = _batch_range(ra), _batch_range(rb)
        a, b = normalize_reference(a, ra), normalize_reference(b, rb)
    if channels == "y":
        a, b = rgb_to_y(a, data_range), rgb_to_y(b, data_range)
    mse = mse_reference(a, b)
    m = ssim_map_reference(a, b, data_range)
    return Metrics(mse, psnr_from_mse(mse, data_range), m.mean(dim=(1, 2, 3)), m if ssim_map else None)


# ------------------------------------------------------------------------------------------------ the library calls
def _check_mode(channels, data_range, normalize):
    if channels not in CHANNELS:
        raise ValueError("channels must be one of %s, got %r" % (sorted(CHANNELS), channels))
    if normalize not in NORMALIZE:
        raise ValueError("normalize must be None, 'face' or 'batch', got %r" % (normalize,))
    if isinstance(data_range, bool) or not isinstance(data_range, (int, float)) or not math.isfinite(data_range) or not data_range > 0:
        raise ValueError("data_range must be a finite number > 0, got %r" % (data_range,))


def _check_images(name, t):
    if not torch.is_tensor(t):
        raise ValueError("%s must be a tensor" % name)
    check_face_images(name, t)


def _range(x, size):
    B = int(x.shape[0])
    out = torch.empty((B, 2), dtype=torch.float32, device=x.device)
    if B:
        _lib.check(_lib.lib().hd_image_range(x.data_ptr(), B, int(x.shape[2]), int(size), out.data_ptr(), stream_ptr(x.device)))
    return out


def image_range(images, size=None):
    """hd_image_range on the current stream of images' device: per face (min, max) over the three channels of images [B,3,R,R] as
    resampled to size x size (None: as they are, and then exactly amin / amax); a float32 [B,2] tensor."""
    _check_images("images", images)
    size = int(images.shape[2]) if size is None else size
    if isinstance(size, bool) or not isinstance(size, int) or size % 64 or not 64 <= size <= 512:
        raise ValueError("size must be a multiple of 64 in [64, 512], got %r" % (size,))
    require_cuda(images.device)
    with torch.cuda.device(images.device):
        return _range(images.to(dtype=torch.float32).contiguous(), size)


def image_metrics(images, ref, channels="y", data_range=1.0, normalize=None, ssim_map=False):
    """hd_image_metrics on the current stream of images' device: images [B,3,R,R] scored against ref [B,3,Rb,Rb] at ref's size (R, Rb
    multiples of 64 in [64, 512]).  channels "rgb" (three planes) or "y" (BT.601 luma); normalize None, "face" (each face min-max
    normalised by its own hd_image_range, images and ref separately) or "batch" (one pair per tensor: the reference's result.min() /
    result.max()).  Returns Metrics(mse, psnr, ssim, ssim_map): float64 [B] tensors and, with ssim_map=True, the float32 map.  The
    inputs are only read; nothing synchronises."""
    _check_mode(channels, data_range, normalize)
    _check_images("images", images)
    _check_images("ref", ref)
    if images.shape[0] != ref.shape[0]:
        raise ValueError("images and ref must hold the same number of faces, got %d and %d" % (images.shape[0], ref.shape[0]))
    require_cuda(images.device)
    dev = images.device
    a = images.to(dtype=torch.float32).contiguous()
    b = ref.to(device=dev, dtype=torch.float32).contiguous()
    B, R, Rb, P = int(a.shape[0]), int(a.shape[2]), int(b.shape[2]), 3 if channels == "rgb" else 1
    out = torch.empty((B, 2), dtype=torch.float64, device=dev)
    smap = torch.empty((B, P, Rb - WINDOW + 1, Rb - WINDOW + 1), dtype=torch.float32, device=dev) if ssim_map else None
    if B:
        with torch.cuda.device(dev):
            L = _lib.lib()
            ra = rb = None
            if normalize is not None:
                ra, rb = _range(a, Rb), _range(b, Rb)
                if normalize == "batch":
                    ra, rb = _batch_range(ra), _batch_range(rb)
            nbytes = _lib.check(L.hd_image_metrics_workspace(B, Rb, CHANNELS[channels]))
            ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=dev)
            _lib.check(L.hd_image_metrics(a.data_ptr(), R, b.data_ptr(), Rb, B, CHANNELS[channels], float(data_range),
                                          ra.data_ptr() if ra is not None else None, rb.data_ptr() if rb is not None else None,
                                          out.data_ptr(), smap.data_ptr() if smap is not None else None, ws.data_ptr(), nbytes,
                                          stream_ptr(dev)))     # ws: freed to the stream it was used on
    mse = out[:, 0]
    return Metrics(mse, psnr_from_mse(mse, float(data_range)), out[:, 1], smap)


Evaluation = collections.namedtuple("Evaluation", "psnr ssim lpips", defaults=(None,))


def evaluate(result, target, lpips=None):
    """The reference loop's scoring as one call (test_refiner.py:107-123): `result` resampled to the target's size, both tensors
    min-max normalised over the whole batch, data_range 1; per-face PSNR over the rgb planes and SSIM on luma (pyiqa's defaults for
    "psnr" and "ssim", unpinned).  lpips: a loaded `LPIPS` model, and then the third score (normalize=True on the batch-normalised
    tensors, which reach the kernel as their two ranges and are not materialised), else None.  Evaluation(psnr, ssim, lpips), float64
    [B] on the device."""
    psnr = image_metrics(result, target, channels="rgb", normalize="batch").psnr
    ssim = image_metrics(result, target, channels="y", normalize="batch").ssim
    return Evaluation(psnr, ssim, None if lpips is None else lpips(result, target, normalize=True, input_normalize="batch"))


def evaluate_reference(result, target):
    """`evaluate` written out in torch ops, in the dtype of `result`."""
    r = resample(result, target.shape[-1])
    t = target.to(r.dtype)
    rn = (r - r.min()) / (r.max() - r.min())
    tn = (t - t.min()) / (t.max() - t.min())
    return Evaluation(psnr_reference(rn, tn, 1.0), ssim_reference(rgb_to_y(rn, 1.0), rgb_to_y(tn, 1.0), 1.0))


# ------------------------------------------------------------------------------------------------ LPIPS
def _bf16(x):
    """The value a kernel stores as bf16 (fp32 arithmetic, then round to nearest even), back in x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def lpips_features(state, x, emulate_bf16=False):
    """The five tapped AlexNet activations of the prepared input x [N,3,R,R] (after the scaling layer), in x's dtype."""
    q = _bf16 if emulate_bf16 else (lambda t: t)
    h, feats = q(x), []
    for i, (name, _, _, _, stride, pad) in enumerate(arch.LPIPS_CONVS):
        if i in (1, 2):
            h = F.max_pool2d(h, 3, 2)
        w, b = state[name + ".weight"].to(device=x.device, dtype=x.dtype), state[name + ".bias"].to(device=x.device, dtype=x.dtype)
        h = q(torch.relu(F.conv2d(h, q(w), b, stride=stride, padding=pad)))
        feats.append(h)
    return feats


def lpips_distance(state, fa, fb):
    """Steps 6 of the contract for the feature lists fa, fb: [N,5] per-layer distances d_k."""
    out = []
    for k, (a, b) in enumerate(zip(fa, fb)):
        w = state["lin%d.model.1.weight" % k].to(device=a.device, dtype=a.dtype).reshape(1, -1, 1, 1)
        na = a / (a.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        nb = b / (b.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
        out.append((w * (na - nb).pow(2)).sum(dim=1).mean(dim=(1, 2)))
    return torch.stack(out, dim=1)


def lpips_prepare(state, x, rng, normalize):
    """Steps 2 - 4 for a tensor already at the scored size: min-max with rng [B,2] (None: none), 2x - 1, the scaling layer."""
    if rng is not None:
        x = normalize_reference(x, rng.to(x.dtype))
    if normalize:
        x = 2 * x - 1
    shift = state.get(arch.LPIPS_SCALING_KEYS[0], torch.tensor(arch.LPIPS_SHIFT, dtype=torch.float64)).to(device=x.device, dtype=x.dtype)
    scale = state.get(arch.LPIPS_SCALING_KEYS[1], torch.tensor(arch.LPIPS_SCALE, dtype=torch.float64)).to(device=x.device, dtype=x.dtype)
    return (x - shift.reshape(1, 3, 1, 1)) / scale.reshape(1, 3, 1, 1)


def lpips_reference(state, images, ref, normalize=True, input_normalize=None, per_layer=False, emulate_bf16=False):
    """The contract of hd_lpips (include/hifidiff_hip.h) from torch ops, in the dtype and on the device of `images`: LPIPS-AlexNet v0.1
    of images [B,3,R,R] against ref [B,3,Rb,Rb] at ref's size.  state: the weights under arch.lpips_manifest's names.  normalize: the
    inputs are in [0, 1] (2x - 1 first).  input_normalize: None, "face" or "batch" min-max normalisation first, as in `image_metrics`.
    emulate_bf16: round to bf16 where the kernels do (the conv weights, the prepared input, every stored activation).  Returns [B], or
    ([B], [B,5]) with per_layer."""
    if input_normalize not in NORMALIZE:
        raise ValueError("input_normalize must be None, 'face' or 'batch', got %r" % (input_normalize,))
    a, b = resample(images, ref.shape[-1]), ref.to(images.dtype)
    ra = rb = None
    if input_normalize is not None:
        ra, rb = range_reference(a), range_reference(b)
        if input_normalize == "batch":
            ra, rb = _batch_range(ra), _batch_range(rb)
    fa = lpips_features(state, lpips_prepare(state, a, ra, normalize), emulate_bf16)
    fb = lpips_features(state, lpips_prepare(state, b, rb, normalize), emulate_bf16)
    layers = lpips_distance(state, fa, fb)
    total = layers.sum(dim=1)
    return (total, layers) if per_layer else total


class LPIPS(WeightContext):
    """LPIPS-AlexNet v0.1 in libhifidiff_hip.so (hd_lpips).  GPU only.  `load_state_dict` takes the `lpips` package's full-model names
    (arch.lpips_manifest; unpinned, the package is absent), or a torchvision AlexNet file's `features.{0,3,6,8,10}.*` (`classifier.*` is
    ignored) together with the lin layers as `lin{k}.model.1.weight` or `lins.{k}.model.1.weight`."""

    _FEATURES = {"features.%s" % n.rsplit(".", 1)[1]: n for n, *_ in arch.LPIPS_CONVS}     # features.0 -> net.slice1.0, ...

    def __init__(self):
        super().__init__()
        self._complete = False

    @classmethod
    def from_files(cls, alexnet_path, lin_path):
        """Two local files (torch.save'd state dicts): the AlexNet features and the lin layers.  No hub access."""
        sd = {}
        for path in (alexnet_path, lin_path):
            part = torch.load(path, map_location="cpu", weights_only=True)
            if not isinstance(part, dict):
                raise RuntimeError("%s does not hold a state dict" % path)
            sd.update(part)
        m = cls()
        m.load_state_dict(sd)
        return m

    @classmethod
    def _canonical_keys(cls, sd):
        out = {}
        for k, v in sd.items():
            if k.startswith("classifier."):
                continue
            head, _, leaf = k.rpartition(".")
            if head in cls._FEATURES:
                k = cls._FEATURES[head] + "." + leaf
            elif k.startswith("lins."):
                k = "lin" + k[len("lins."):]
            if not torch.is_tensor(v):
                continue                                   # non-weight entries (metadata some exporters add)
            out[k] = v
        return out

    def load_state_dict(self, sd, strict=True):
        man = arch.lpips_manifest()
        sd = self._canonical_keys(sd)
        shapes = {k: v[0] for k, v in man.items()}
        if any(k in sd for k in arch.LPIPS_SCALING_KEYS):    # optional, but both or neither
            shapes.update({k: (1, 3, 1, 1) for k in arch.LPIPS_SCALING_KEYS})
        missing = [k for k in shapes if k not in sd]
        unexpected = [k for k in sd if k not in shapes]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for LPIPS: Missing key(s): %s; Unexpected key(s): %s" % (missing[:4], unexpected[:4]))
        for k, shape in shapes.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise RuntimeError("size mismatch for %s: got %s, expected %s" % (k, tuple(sd[k].shape), tuple(shape)))
        self._state = {k: sd[k].detach() for k in shapes if k in sd}
        self._complete = not missing
        if self._ctx is not None:
            self._upload()                                 # a context whose weights are finalized is replaced (self._loaded)
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def state_dict(self, *a, **k):
        return dict(self._state or {})

    def _create(self, idx):
        ctx = ctypes.c_void_p()
        _lib.check(_lib.lib().hd_lpips_create(ctypes.byref(ctx), idx))
        return ctx

    def _items(self):
        if not self._complete:
            raise RuntimeError("state dict incomplete: %d tensors loaded" % len(self._state))
        return list(self._state.items())         # the optional scaling keys included

    def __call__(self, images, ref, normalize=True, input_normalize=None, per_layer=False):
        """hd_lpips on the current stream of images' device: images [B,3,R,R] against ref [B,3,Rb,Rb] at ref's size (R, Rb multiples of
        64 in [64, 512]).  normalize: the inputs are in [0, 1].  input_normalize: None, "face" or "batch" min-max normalisation first
        (hd_image_range; the normalised tensors are not materialised).  Returns float64 [B], or ([B], [B,5]) with per_layer.  The
        inputs are only read; nothing synchronises."""
        if input_normalize not in NORMALIZE:
            raise ValueError("input_normalize must be None, 'face' or 'batch', got %r" % (input_normalize,))
        _check_images("images", images)
        _check_images("ref", ref)
        if images.shape[0] != ref.shape[0]:
            raise ValueError("images and ref must hold the same number of faces, got %d and %d" % (images.shape[0], ref.shape[0]))
        require_cuda(images.device)
        self._ensure(images.device)
        if not self._loaded:
            raise RuntimeError("weights are not loaded: call load_state_dict(...) first")
        dev = self._device
        a = images.to(dtype=torch.float32).contiguous()
        b = ref.to(device=dev, dtype=torch.float32).contiguous()
        B, R, Rb = int(a.shape[0]), int(a.shape[2]), int(b.shape[2])
        out = torch.empty((B,), dtype=torch.float64, device=dev)
        layers = torch.empty((B, 5), dtype=torch.float64, device=dev) if per_layer else None
        if B:
            with torch.cuda.device(dev):
                ra = rb = None
                if input_normalize is not None:
                    ra, rb = _range(a, Rb), _range(b, Rb)
                    if input_normalize == "batch":
                        ra, rb = _batch_range(ra), _batch_range(rb)
                _lib.check(_lib.lib().hd_lpips(self._ctx, B, a.data_ptr(), R, b.data_ptr(), Rb, 1 if normalize else 0,
                                               ra.data_ptr() if ra is not None else None, rb.data_ptr() if rb is not None else None,
                                               out.data_ptr(), layers.data_ptr() if layers is not None else None,
                                               stream_ptr(dev)), self._ctx)
            self._keep = (a, b, ra, rb, out, layers)         # the launch program holds these pointers until the next call
        return (out, layers) if per_layer else out
