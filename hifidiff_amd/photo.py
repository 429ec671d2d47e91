"""The two ends that touch a photograph: `ingest` cuts head boxes out of uint8 photos and makes the reference's `ln_face`
(crop -> resize((lr, lr), BICUBIC) -> resize((res, res), BICUBIC) -> to_tensor; dataset_kface.py:86-98) or its ground truth (lr = 0:
crop -> resize((res, res), BICUBIC) -> to_tensor); `paste` puts restored faces back into the photos, resized to their boxes and
feathered at the box edge.  Both are Pillow's 8-bit two-pass antialiased bicubic resize, which is integer arithmetic on coefficients
computed in float64, so the results equal Pillow's byte for byte.

`ingest` and `paste` run in libhifidiff_hip.so (hd_face_ingest / hd_face_paste: GPU only, like color.color_fix).
`pil_bicubic_reference`, `ingest_reference` and `paste_reference` state the same rule in plain torch on any device: the role
`color.*_reference` plays for the colour fix.  include/hifidiff_hip.h has the arithmetic."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._context import require_cuda, stream_ptr

PRECISION_BITS = 22                                                   # Pillow's 32 - 8 - 2
MAX_SIDE = 2048
MAX_FEATHER = 256
MAX_BATCH = 4096


# ------------------------------------------------------------------------------------------------ the resize rule
def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resize_coefficients(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis: (xmin [n_out], count [n_out], K [n_out, max count]) with K the
    22-bit fixed-point weights (int64).  Everything is float64 and numpy does not contract a multiply and an add; the sum runs in index
    order, as Pillow's does."""
    n_in, n_out = int(n_in), int(n_out)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    xmins, counts, rows = [], [], []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        k = _bicubic((np.arange(xmax - xmin, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = np.cumsum(k)[-1]                                         # sequential, not pairwise
        if ww != 0.0:
            k = k / ww
        K = (k * float(1 << PRECISION_BITS) + np.where(k < 0, -0.5, 0.5)).astype(np.int64)   # astype truncates, as (int)
        xmins.append(xmin), counts.append(xmax - xmin), rows.append(K)
    table = np.zeros((n_out, max(counts)), dtype=np.int64)
    for i, K in enumerate(rows):
        table[i, :len(K)] = K
    return np.asarray(xmins), np.asarray(counts), table


def _resize_axis0(x, n_out):
    """One pass along dim 0 of an integer-valued float64 tensor [n_in, ...] -> [n_out, ...], clipped and rounded to 0..255.  The
    products are integers below 2^31, so the float64 matmul is exact in any summation order."""
    n_in = x.shape[0]
    xmin, cnt, K = resize_coefficients(n_in, n_out)
    M = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        M[i, xmin[i]:xmin[i] + cnt[i]] = K[i, :cnt[i]]
    acc = (torch.from_numpy(M).to(x.device) @ x.reshape(n_in, -1)).to(torch.int64)
    out = ((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS).clamp_(0, 255)
    return out.to(torch.float64).reshape((n_out,) + tuple(x.shape[1:]))


def pil_bicubic_reference(img_u8, size):
    """PIL.Image.resize(size, BICUBIC) of a uint8 image [H, W, C] (tensor or array, any device); size = (width, height) as in PIL.
    Horizontal pass first, into a clipped and rounded uint8 intermediate; a pass whose size does not change is skipped."""
    img = torch.as_tensor(img_u8)
    if img.dtype != torch.uint8 or img.dim() != 3:
        raise ValueError("img_u8 must be a uint8 image [H, W, C], got %s %s" % (img.dtype, tuple(img.shape)))
    w, h = int(size[0]), int(size[1])
    if w < 1 or h < 1 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("sizes must be >= 1")
    x = img.to(torch.float64)
    if w != img.shape[1]:
        x = _resize_axis0(x.transpose(0, 1).contiguous(), w).transpose(0, 1).contiguous()
    if h != img.shape[0]:
        x = _resize_axis0(x, h)
    return x.to(torch.uint8)


def feather_mask(w, h, feather, device=None):
    """The paste weight in 1/256ths [h, w] (int64): 256 without feather, else min(256, ((2 d + 1) * 256) // (2 feather)) with d the
    distance to the nearest box edge, min(x, w-1-x, y, h-1-y)."""
    x = torch.arange(w, device=device)
    y = torch.arange(h, device=device)
    d = torch.minimum(torch.minimum(x, w - 1 - x)[None, :], torch.minimum(y, h - 1 - y)[:, None])
    if feather == 0:
        return torch.full_like(d, 256)
    return torch.clamp(((2 * d + 1) * 256) // (2 * feather), max=256)


def quantize_reference(faces):
    """torchvision save_image's rule: clamp(floor(x * 255 + 0.5), 0, 255) in fp32, NaN -> 0; [B,3,R,R] -> uint8 [B,R,R,3]."""
    v = faces.to(torch.float32) * 255
    v = torch.floor(v + 0.5)
    v = torch.where(torch.isnan(v), torch.zeros_like(v), v).clamp(0, 255)
    return v.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ argument checks (as the C side)
def _check_common(photos, boxes, photo_index):
    if not torch.is_tensor(photos) or photos.dtype != torch.uint8 or photos.dim() != 4 or photos.shape[3] != 3 or photos.shape[0] < 1:
        raise ValueError("photos must be a uint8 tensor [N, H, W, 3]")
    N, H, W = int(photos.shape[0]), int(photos.shape[1]), int(photos.shape[2])
    b = np.asarray(boxes.cpu() if torch.is_tensor(boxes) else boxes, dtype=np.int64).reshape(-1, 4)
    B = b.shape[0]
    if B > MAX_BATCH:
        raise ValueError("at most %d boxes per call, got %d" % (MAX_BATCH, B))
    if photo_index is None:
        idx = np.zeros(B, dtype=np.int64)
    else:
        idx = np.asarray(photo_index.cpu() if torch.is_tensor(photo_index) else photo_index, dtype=np.int64).reshape(-1)
        if idx.shape[0] != B:
            raise ValueError("photo_index must hold one index per box, got %d for %d boxes" % (idx.shape[0], B))
    for i in range(B):
        l, t, w, h = (int(v) for v in b[i])
        if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
            raise ValueError("boxes[%d]: sides must be in [1, %d], got %d x %d" % (i, MAX_SIDE, w, h))
        if l < 0 or t < 0 or l + w > W or t + h > H:
            raise ValueError("boxes[%d] = (%d, %d, %d, %d) does not lie inside the %d x %d photo" % (i, l, t, w, h, W, H))
        if not 0 <= idx[i] < N:
            raise ValueError("photo_index[%d] = %d is outside [0, %d)" % (i, idx[i], N))
    return b.astype(np.int32), idx.astype(np.int32)


def _check_sizes(lr, res):
    if isinstance(lr, bool) or not isinstance(lr, int) or not (lr == 0 or 8 <= lr <= 64):
        raise ValueError("lr must be 0 or an integer in [8, 64], got %r" % (lr,))
    if isinstance(res, bool) or not isinstance(res, int) or res % 64 or not 64 <= res <= 512:
        raise ValueError("res must be a multiple of 64 in [64, 512], got %r" % (res,))


def _check_feather(feather):
    if isinstance(feather, bool) or not isinstance(feather, int) or not 0 <= feather <= MAX_FEATHER:
        raise ValueError("feather must be an integer in [0, %d], got %r" % (MAX_FEATHER, feather))


def boxes_overlap(boxes, photo_index):
    """The first pair (i, j) of boxes that share a pixel of one photo, or None.  Boxes that only touch do not overlap."""
    for i in range(len(boxes)):
        for j in range(i + 1, len(boxes)):
            if photo_index[i] != photo_index[j]:
                continue
            a, b = boxes[i], boxes[j]
            if a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]:
                return i, j
    return None


def _check_faces(faces, B):
    if not torch.is_tensor(faces) or faces.dim() != 4 or faces.shape[0] != B or faces.shape[1] != 3 or faces.shape[2] != faces.shape[3] \
            or faces.shape[2] % 64 or not 64 <= faces.shape[2] <= 512:
        raise ValueError("faces must be (B,3,R,R) with one face per box and R a multiple of 64 in [64, 512], got %s for %d boxes"
                         % (tuple(faces.shape) if torch.is_tensor(faces) else type(faces), B))


# ------------------------------------------------------------------------------------------------ references
def ingest_reference(photos, boxes, photo_index=None, lr=32, res=128, return_uint8=False):
    """`ingest` in plain torch on photos' device: fp32 [B,3,res,res] = uint8 / 255 (and the uint8 [B,res,res,3] with return_uint8)."""
    b, idx = _check_common(photos, boxes, photo_index)
    _check_sizes(lr, res)
    u8 = torch.empty((len(b), res, res, 3), dtype=torch.uint8, device=photos.device)
    for i, (l, t, w, h) in enumerate(b.tolist()):
        face = photos[int(idx[i]), t:t + h, l:l + w]
        if lr:
            face = pil_bicubic_reference(face, (lr, lr))
        u8[i] = pil_bicubic_reference(face, (res, res))
    # a tensor divisor: torch multiplies by the reciprocal of a Python-number divisor on the GPU, and to_tensor's result is a true division
    out = u8.permute(0, 3, 1, 2).to(torch.float32) / torch.full((), 255.0, device=u8.device)
    return (out, u8) if return_uint8 else out


def paste_reference(photos, faces, boxes, photo_index=None, feather=0):
    """`paste` in plain torch on photos' device; returns a new photo tensor."""
    b, idx = _check_common(photos, boxes, photo_index)
    _check_faces(faces, len(b))
    _check_feather(feather)
    if boxes_overlap(b, idx) is not None:
        raise ValueError("boxes %d and %d overlap in one photo" % boxes_overlap(b, idx))
    out = photos.clone()
    q8 = quantize_reference(faces.to(photos.device))
    for i, (l, t, w, h) in enumerate(b.tolist()):
        q = pil_bicubic_reference(q8[i], (w, h)).to(torch.int64)
        m = feather_mask(w, h, feather, device=photos.device)[:, :, None]
        p = out[int(idx[i]), t:t + h, l:l + w].to(torch.int64)
        out[int(idx[i]), t:t + h, l:l + w] = ((p * (256 - m) + q * m + 128) >> 8).to(torch.uint8)
    return out


# ------------------------------------------------------------------------------------------------ the GPU calls
def _host_i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def ingest(photos, boxes, photo_index=None, lr=32, res=128, return_uint8=False):
    """hd_face_ingest on the current stream of photos' device: photos uint8 [N,H,W,3], boxes [B,4] (left, top, width, height) and
    photo_index [B] on the host.  Returns fp32 [B,3,res,res] in [0, 1] (and the uint8 [B,res,res,3] with return_uint8)."""
    b, idx = _check_common(photos, boxes, photo_index)
    _check_sizes(lr, res)
    require_cuda(photos.device)
    dev, B = photos.device, len(b)
    out = torch.empty((B, 3, res, res), dtype=torch.float32, device=dev)
    u8 = torch.empty((B, res, res, 3), dtype=torch.uint8, device=dev) if return_uint8 else None
    if B:
        L = _lib.lib()
        p = photos.contiguous()
        need = _lib.check(L.hd_face_ingest_workspace(B, lr, res))
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
        (b, bp), (idx, ip) = _host_i32(b), _host_i32(idx)
        with torch.cuda.device(dev):
            _lib.check(L.hd_face_ingest(p.data_ptr(), int(p.shape[0]), int(p.shape[1]), int(p.shape[2]), bp, ip, B, lr, res, out.data_ptr(),
                                        u8.data_ptr() if u8 is not None else None, ws.data_ptr(), need, stream_ptr(dev)))
        ws.record_stream(torch.cuda.current_stream(dev))
    return (out, u8) if return_uint8 else out


def paste(photos, faces, boxes, photo_index=None, feather=0, inplace=False):
    """hd_face_paste on the current stream of photos' device: faces fp32 [B,3,R,R] in [0, 1] are quantised, resized to their boxes and
    blended into photos (uint8 [N,H,W,3]) with a feathered edge.  Returns the photos: a new tensor unless inplace."""
    b, idx = _check_common(photos, boxes, photo_index)
    _check_faces(faces, len(b))
    _check_feather(feather)
    pair = boxes_overlap(b, idx)
    if pair is not None:
        raise ValueError("boxes %d and %d overlap in one photo" % pair)
    require_cuda(photos.device)
    if inplace and not photos.is_contiguous():
        raise ValueError("inplace needs contiguous photos")
    dev, B = photos.device, len(b)
    out = photos if inplace else photos.clone(memory_format=torch.contiguous_format)
    if B:
        L = _lib.lib()
        f = faces.to(device=dev, dtype=torch.float32).contiguous()
        res = int(f.shape[2])
        need = _lib.check(L.hd_face_paste_workspace(B, res))
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        (b, bp), (idx, ip) = _host_i32(b), _host_i32(idx)
        with torch.cuda.device(dev):
            _lib.check(L.hd_face_paste(out.data_ptr(), int(out.shape[0]), int(out.shape[1]), int(out.shape[2]), f.data_ptr(), res, bp, ip, B,
                                       feather, ws.data_ptr(), need, stream_ptr(dev)))
        ws.record_stream(torch.cuda.current_stream(dev))
        f.record_stream(torch.cuda.current_stream(dev))
    return out
