"""What tests/test_photo_host.py and tests/test_photo.py share: tests/golden/photo_pil.npz (tools/photo_golden.py wrote it with Pillow)
decoded once, and the two golden photos on one canvas, as one call of hifidiff_amd.photo takes them."""
import functools

import numpy as np
import torch

from conftest import golden


def _decode(e):
    """tools/photo_golden.py's encode undone: planar differences along x (mod 256) -> uint8 [..., H, W, 3]."""
    return np.ascontiguousarray(np.moveaxis(np.cumsum(e, axis=-1, dtype=np.uint8), -3, -1))


@functools.lru_cache(maxsize=None)
def pil():
    z = golden("photo_pil.npz")
    return {k: (_decode(z[k]) if z[k].dtype == np.uint8 else z[k]) for k in z.files}


def boxes():
    """(photo_index [n], boxes [n,4] as left, top, width, height) of the golden box list."""
    b = pil()["boxes"]
    return b[:, 0].copy(), b[:, 1:].copy()


@functools.lru_cache(maxsize=None)
def canvas():
    """uint8 [2, H, W, 3]: both golden photos at the top left of a common canvas whose remaining bytes are 255.  The crop comes before
    the resize, so what surrounds a photo must not matter."""
    p0, p1 = pil()["photo0"], pil()["photo1"]
    H, W = max(p0.shape[0], p1.shape[0]), max(p0.shape[1], p1.shape[1])
    c = np.full((2, H, W, 3), 255, dtype=np.uint8)
    c[0, :p0.shape[0], :p0.shape[1]] = p0
    c[1, :p1.shape[0], :p1.shape[1]] = p1
    return torch.from_numpy(c)


def ingest_golden(lr, res=64):
    """(box numbers, uint8 [n,res,res,3]) of Pillow's results for that setting."""
    g = pil()
    if res == 128:
        return [int(g["box128"])], torch.from_numpy(g["ingest_lr32_res128"][None])
    which = [int(i) for i in g["boxes16"]] if lr == 16 else list(range(len(g["boxes"])))
    return which, torch.from_numpy(g["ingest_lr%d_res64" % lr])
