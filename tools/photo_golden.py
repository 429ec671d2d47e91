"""Writes tests/golden/photo_pil.npz: Pillow's own results for the photo ingest and paste-back resizes (hifidiff_amd.photo), so that the
tests can hold the library to byte equality with Pillow on machines that do not have it.  Needs Pillow; run from the repository root:
    python tools/photo_golden.py
Two synthetic photos of different sizes (synth.photo: a smooth field plus noise, from synth.rand), the box list of tests/test_photo.py, and per box
  ingest_lr{32,16,0}_res64   crop -> resize((lr, lr), BICUBIC) -> resize((64, 64), BICUBIC)      (lr 0: crop -> (64, 64)); lr 16 for BOXES16 only
  ingest_lr32_res128         the same at 128 for BOX128
  paste_<i>                  the lr 0 result of box i resized to the box's (width, height): the paste direction, for PASTE_BOXES
Image arrays are stored planar and as differences along x modulo 256 (`encode`; np.cumsum(..., dtype=uint8) undoes it): deflate gets the
file under 400 KB that way, and the bytes are still Pillow's.  No tool or test that runs on the GPU imports this file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hifidiff_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "photo_pil.npz")
SIZES = [(120, 144), (131, 113)]                                      # (height, width) of the two photos
#        photo, left, top, width, height
BOXES = [
    (0, 0, 0, 144, 120),       # 0  the whole photo
    (1, 0, 0, 113, 131),       # 1  the whole photo
    (0, 0, 0, 40, 45),         # 2  top left corner
    (0, 103, 0, 41, 40),       # 3  top right corner
    (1, 0, 92, 38, 39),        # 4  bottom left corner
    (1, 80, 94, 33, 37),       # 5  bottom right corner, 33 x 37: scale just above 1 at lr 32
    (0, 50, 40, 20, 24),       # 6  the first pass upscales
    (1, 30, 30, 32, 32),       # 7  both passes skipped at lr 32
    (0, 60, 10, 32, 90),       # 8  the horizontal pass skipped at lr 32
    (1, 20, 70, 64, 31),       # 9
    (0, 100, 100, 7, 3),       # 10
    (1, 112, 130, 1, 1),       # 11 one pixel, in the corner
    (0, 17, 11, 111, 97),      # 12 odd, non-integer scale
    (0, 3, 5, 64, 64),         # 13 the identity at lr 0, res 64
]
BOXES16 = [0, 5, 6, 8, 10, 11, 12]
BOX128 = 12
PASTE_BOXES = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]


def encode(a):
    """uint8 [..., H, W, 3] -> uint8 [..., 3, H, W] of differences along x (mod 256)."""
    p = np.moveaxis(a, -1, -3).astype(np.int16)
    return np.diff(p, axis=-1, prepend=0).astype(np.uint8)


def decode(e):
    return np.moveaxis(np.cumsum(e, axis=-1, dtype=np.uint8), -3, -1)


def main():
    import PIL
    from PIL import Image
    photos = [synth.photo("photo.%d" % k, h, w) for k, (h, w) in enumerate(SIZES)]

    def ingest(i, lr, res):
        p, l, t, w, h = BOXES[i]
        im = Image.fromarray(photos[p]).crop((l, t, l + w, t + h))
        if lr:
            im = im.resize((lr, lr), Image.BICUBIC)
        return np.asarray(im.resize((res, res), Image.BICUBIC))

    d = {"photo0": photos[0], "photo1": photos[1], "boxes": np.asarray(BOXES, dtype=np.int32), "boxes16": np.asarray(BOXES16, dtype=np.int32),
         "box128": np.asarray(BOX128, dtype=np.int32), "paste_boxes": np.asarray(PASTE_BOXES, dtype=np.int32),
         "pillow_version": np.asarray(PIL.__version__)}
    d["ingest_lr32_res64"] = np.stack([ingest(i, 32, 64) for i in range(len(BOXES))])
    d["ingest_lr0_res64"] = np.stack([ingest(i, 0, 64) for i in range(len(BOXES))])
    d["ingest_lr16_res64"] = np.stack([ingest(i, 16, 64) for i in BOXES16])
    d["ingest_lr32_res128"] = ingest(BOX128, 32, 128)
    for i in PASTE_BOXES:
        _, _, _, w, h = BOXES[i]
        d["paste_%d" % i] = np.asarray(Image.fromarray(d["ingest_lr0_res64"][i]).resize((w, h), Image.BICUBIC))
    for k in list(d):
        if d[k].dtype == np.uint8:
            assert np.array_equal(decode(encode(d[k])), d[k]), k
            d[k] = encode(d[k])
    np.savez_compressed(OUT, **d)
    print("%s: %d bytes, Pillow %s" % (OUT, os.path.getsize(OUT), PIL.__version__))


if __name__ == "__main__":
    main()
