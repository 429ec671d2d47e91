"""Colour correction of decoded faces against a reference image: the step restoration stacks apply after `vae.decode`
(StableSR's `wavelet_color_fix` / `adain_color_fix`).  Low-pass guidance works on the four latent channels during sampling; this ties
the colour of the decoded RGB image to the input.  The reference project has no such step.

`color_fix` runs in libhifidiff_hip.so (hd_color_fix: one launch, GPU only, like the schedulers).  `wavelet_color_fix_reference` and
`adain_color_fix_reference` state the same formulas in plain torch, in any dtype and on any device: the role `sampling.low_pass` plays
for guidance.  include/hifidiff_hip.h has the arithmetic."""
import torch
import torch.nn.functional as F

from . import _lib
from ._context import check_face_images, require_cuda, stream_ptr

MODES = {"wavelet": 1, "adain": 2}
MAX_LEVELS = 5


def to_vae_range(x):
    """train_refiner.py's to_vae_range: [0, 1] images to the VAE's [-1, 1]."""
    return x.clamp(0, 1) * 2 - 1


def wavelet_blur(x, radius):
    """One a-trous level: the 3x3 binomial kernel with dilation `radius` under replicate padding, per channel plane of [B,C,H,W]."""
    C = x.shape[1]
    k = torch.tensor([0.25, 0.5, 0.25], dtype=x.dtype, device=x.device)
    k = (k[:, None] * k[None, :])[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(F.pad(x, (radius,) * 4, mode="replicate"), k, groups=C, dilation=radius)


def wavelet_decomposition(x, levels=MAX_LEVELS):
    """(high, low) of StableSR's wavelet_decomposition: high = sum_i (x_i - blur_i(x_i)), low = x_levels."""
    high = torch.zeros_like(x)
    for i in range(levels):
        low = wavelet_blur(x, 2 ** i)
        high = high + (x - low)
        x = low
    return high, x


def _weight_planes(weight, images):
    if weight is None:
        return None
    w = torch.as_tensor(weight, dtype=images.dtype, device=images.device)
    if w.dim() == 0:
        w = w.expand(images.shape[0])
    if tuple(w.shape) != (images.shape[0],):
        raise ValueError("weight must be a number or one value per face, got shape %s" % (tuple(w.shape),))
    return w[:, None, None, None]


def _check_pair(images, ref):
    if images.dim() != 4 or ref.dim() != 4 or images.shape[:2] != ref.shape[:2]:
        raise ValueError("images and ref must be (B,C,H,W) with equal B and C, got %s and %s" % (tuple(images.shape), tuple(ref.shape)))


def _check_levels(levels):
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError("levels must be an integer in [1, %d], got %r" % (MAX_LEVELS, levels))


def wavelet_color_fix_reference(images, ref, levels=MAX_LEVELS, weight=None, ref_vae_range=False):
    """high(images) + low(ref) in StableSR's decomposition form; with a weight, images + w * (that - images).  `ref` of another size
    is first resampled with F.interpolate(mode="bicubic", align_corners=False), after the range mapping.  A face with w == 0 keeps
    its image exactly."""
    _check_pair(images, ref)
    _check_levels(levels)
    s = ref.to(images.dtype)
    if ref_vae_range:
        s = to_vae_range(s)
    if s.shape[-2:] != images.shape[-2:]:
        s = F.interpolate(s, size=images.shape[-2:], mode="bicubic", align_corners=False)
    high, _ = wavelet_decomposition(images, levels)
    _, low = wavelet_decomposition(s, levels)
    fixed = high + low
    w = _weight_planes(weight, images)
    if w is None:
        return fixed
    return torch.where(w == 0, images, images + w * (fixed - images))


def adain_color_fix_reference(images, ref, weight=None, ref_vae_range=False, eps=1e-5):
    """Per channel plane: (images - mean) * std(ref) / std(images) + mean(ref), std = sqrt(unbiased variance + eps), the statistics of
    `ref` at its own resolution; with a weight, images + w * (that - images)."""
    _check_pair(images, ref)
    s = ref.to(images.dtype)
    if ref_vae_range:
        s = to_vae_range(s)
    mc, ms = images.mean(dim=(-2, -1), keepdim=True), s.mean(dim=(-2, -1), keepdim=True)
    sc = (images.var(dim=(-2, -1), keepdim=True, unbiased=True) + eps).sqrt()
    ss = (s.var(dim=(-2, -1), keepdim=True, unbiased=True) + eps).sqrt()
    fixed = (images - mc) * (ss / sc) + ms
    w = _weight_planes(weight, images)
    if w is None:
        return fixed
    return torch.where(w == 0, images, images + w * (fixed - images))


def color_fix(images, ref, mode="wavelet", levels=MAX_LEVELS, weight=None, ref_vae_range=False):
    """hd_color_fix on the current stream of images' device: images [B,3,R,R] corrected towards ref [B,3,Rr,Rr] (R, Rr multiples of 64
    in [64, 512]); weight: None, a number or one value per face in [0, 1].  Returns a new fp32 tensor; the inputs are only read."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
    if mode == "wavelet":
        _check_levels(levels)
    if not torch.is_tensor(images) or not torch.is_tensor(ref):
        raise ValueError("images and ref must be tensors")
    check_face_images("images", images)
    check_face_images("ref", ref)
    if images.shape[0] != ref.shape[0]:
        raise ValueError("images and ref must hold the same number of faces, got %d and %d" % (images.shape[0], ref.shape[0]))
    B = int(images.shape[0])
    w = None
    if weight is not None:
        w = torch.as_tensor(weight, dtype=torch.float32)
        if w.dim() == 0:
            w = w.expand(B)
        if tuple(w.shape) != (B,):
            raise ValueError("weight must be a number or one value per face, got shape %s" % (tuple(w.shape),))
        if not bool(((w >= 0) & (w <= 1)).all()):
            raise ValueError("weight must lie in [0, 1]")
    require_cuda(images.device)
    dev = images.device
    c = images.to(dtype=torch.float32).contiguous()
    s = ref.to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty_like(c)
    if B == 0:
        return out
    if w is not None:
        w = w.to(device=dev).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().hd_color_fix(c.data_ptr(), out.data_ptr(), B, int(c.shape[2]), s.data_ptr(), int(s.shape[2]),
                                           1 if ref_vae_range else 0, MODES[mode], int(levels), w.data_ptr() if w is not None else None, stream_ptr(dev)))
    return out
