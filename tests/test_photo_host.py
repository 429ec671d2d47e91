"""Host side of the photo ingest and paste-back (no GPU): hifidiff_amd.photo's references against Pillow's own results
(tests/golden/photo_pil.npz; against Pillow itself where it is installed), the exports, every HD_ERR_INVALID case of hd_face_ingest /
hd_face_paste (raised before any HIP call, so this machine needs no device), the overlap rule and the feather mask."""
import ctypes

import numpy as np
import pytest
import torch

import photo_cases as pc
from hifidiff_amd import _lib, photo

HD_ERR_INVALID = -1                                                   # include/hifidiff_hip.h


# ------------------------------------------------------------------------------------------------ the references against Pillow's bytes
@pytest.mark.parametrize("lr,res", [(32, 64), (16, 64), (0, 64), (32, 128)])
def test_ingest_reference_equals_the_goldens(lr, res):
    idx, boxes = pc.boxes()
    which, want = pc.ingest_golden(lr, res)
    out, u8 = photo.ingest_reference(pc.canvas(), boxes[which], idx[which], lr=lr, res=res, return_uint8=True)
    assert torch.equal(u8, want)
    assert out.dtype == torch.float32 and torch.equal(out, want.permute(0, 3, 1, 2).float().div(255))


def test_paste_direction_resize_equals_the_goldens():
    g = pc.pil()
    _, boxes = pc.boxes()
    for i in g["paste_boxes"]:
        w, h = int(boxes[i, 2]), int(boxes[i, 3])
        got = photo.pil_bicubic_reference(g["ingest_lr0_res64"][i], (w, h))
        assert np.array_equal(got.numpy(), g["paste_%d" % i]), (int(i), w, h)


def test_same_size_is_the_identity_and_the_goldens_name_their_pillow():
    g = pc.pil()
    assert str(g["pillow_version"])[0].isdigit()
    x = torch.from_numpy(g["photo0"])
    assert torch.equal(photo.pil_bicubic_reference(x, (x.shape[1], x.shape[0])), x)
    _, boxes = pc.boxes()
    assert tuple(boxes[13, 2:]) == (64, 64)                           # the identity case of the ingest: a 64 x 64 box at lr 0, res 64
    l, t = int(boxes[13, 0]), int(boxes[13, 1])
    assert np.array_equal(g["ingest_lr0_res64"][13], g["photo0"][t:t + 64, l:l + 64])


def test_references_equal_pillow_itself():
    Image = pytest.importorskip("PIL.Image")
    idx, boxes = pc.boxes()
    photos = pc.canvas()
    for i in range(len(boxes)):
        l, t, w, h = (int(v) for v in boxes[i])
        crop = Image.fromarray(photos[int(idx[i]), t:t + h, l:l + w].numpy())
        for lr, res in ((32, 64), (16, 128), (8, 64), (0, 64)):
            im = crop.resize((lr, lr), Image.BICUBIC) if lr else crop
            want = np.asarray(im.resize((res, res), Image.BICUBIC))
            _, got = photo.ingest_reference(photos, boxes[i:i + 1], idx[i:i + 1], lr=lr, res=res, return_uint8=True)
            assert np.array_equal(got[0].numpy(), want), (i, lr, res)
        face = torch.from_numpy(pc.pil()["ingest_lr0_res64"][i])
        want = np.asarray(Image.fromarray(face.numpy()).resize((w, h), Image.BICUBIC))
        assert np.array_equal(photo.pil_bicubic_reference(face, (w, h)).numpy(), want), i


def test_paste_reference_blends_with_the_mask():
    idx, boxes = pc.boxes()
    photos = pc.canvas()
    which = [2, 6, 9]
    faces = torch.from_numpy(pc.pil()["ingest_lr32_res64"][which]).permute(0, 3, 1, 2).float().div(255)
    for feather in (0, 3, 40):
        got = photo.paste_reference(photos, faces, boxes[which], idx[which], feather=feather)
        changed = torch.zeros(photos.shape[:3], dtype=torch.bool)
        for n, i in enumerate(which):
            l, t, w, h = (int(v) for v in boxes[i])
            q = photo.pil_bicubic_reference(photo.quantize_reference(faces[n:n + 1])[0], (w, h)).long()
            m = photo.feather_mask(w, h, feather)[:, :, None]
            p = photos[int(idx[i]), t:t + h, l:l + w].long()
            assert torch.equal(got[int(idx[i]), t:t + h, l:l + w].long(), (p * (256 - m) + q * m + 128) >> 8)
            changed[int(idx[i]), t:t + h, l:l + w] = True
        assert torch.equal(got[~changed], photos[~changed])
    assert torch.equal(photo.quantize_reference(faces), torch.from_numpy(pc.pil()["ingest_lr32_res64"][which]))     # u8 / 255 comes back as u8


@pytest.mark.parametrize("feather", [0, 1, 16, 256])
def test_mask_formula(feather):
    for w, h in ((1, 1), (7, 3), (40, 45), (600, 513)):
        m = photo.feather_mask(w, h, feather)
        assert tuple(m.shape) == (h, w)
        for x, y in ((0, 0), (w - 1, h - 1), (w // 2, h // 2), (w // 3, 0), (0, h // 3), (min(w - 1, feather), min(h - 1, feather))):
            d = min(x, w - 1 - x, y, h - 1 - y)
            want = 256 if feather == 0 else min(256, ((2 * d + 1) * 256) // (2 * feather))
            assert int(m[y, x]) == want, (w, h, x, y)
        assert int(m.min()) >= (256 if feather == 0 else 256 // (2 * feather)) and int(m.max()) <= 256
    if feather == 1:
        assert int(photo.feather_mask(5, 5, 1).min()) == 128 and int(photo.feather_mask(5, 5, 1)[1, 1]) == 256


# ------------------------------------------------------------------------------------------------ exports and argument checks
def test_the_entry_points_are_exported():
    with open(_lib.HEADER) as fh:
        header = fh.read()
    for name, decl in (("hd_face_ingest", "int hd_face_ingest("), ("hd_face_paste", "int hd_face_paste("),
                       ("hd_face_ingest_workspace", "int64_t hd_face_ingest_workspace("), ("hd_face_paste_workspace", "int64_t hd_face_paste_workspace(")):
        assert name in _lib.EXPORTS
        assert decl in header
        assert hasattr(_lib.lib(), name)
    import hifidiff_amd
    assert hifidiff_amd.photo is photo


PHO, OUT, U8, WS, FAC = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000     # made-up addresses: no check reads them
BIG = 1 << 40


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _ingest(photos=PHO, n=2, H=100, W=120, boxes=((0, 0, 50, 50),), index=None, lr=32, res=128, out=OUT, ws=WS, ws_bytes=BIG, pass_boxes=True):
    L = _lib.lib()
    b, bp = _i32(boxes)
    i, ip = _i32(index) if index is not None else (None, None)
    rc = L.hd_face_ingest(photos, n, H, W, bp if pass_boxes else None, ip, len(b), lr, res, out, U8, ws, ws_bytes, None)
    return rc, L.hd_last_error(None).decode()


def _paste(photos=PHO, n=2, H=100, W=120, faces=FAC, res=64, boxes=((0, 0, 50, 50),), index=None, feather=0, ws=WS, ws_bytes=BIG, pass_boxes=True):
    L = _lib.lib()
    b, bp = _i32(boxes)
    i, ip = _i32(index) if index is not None else (None, None)
    rc = L.hd_face_paste(photos, n, H, W, faces, res, bp if pass_boxes else None, ip, len(b), feather, ws, ws_bytes, None)
    return rc, L.hd_last_error(None).decode()


COMMON_BAD = [
    (dict(photos=None), "photos"),
    (dict(pass_boxes=False), "boxes is NULL"),
    (dict(n=0), "n_photos"),
    (dict(H=0), "height"),
    (dict(W=-4), "width"),
    (dict(boxes=np.zeros((0, 4))), "batch"),
    (dict(boxes=((0, 0, 0, 10),)), "boxes[0]: sides"),
    (dict(boxes=((0, 0, 10, 10), (0, 20, 10, 2049))), "boxes[1]: sides"),
    (dict(boxes=((0, 0, 10, -1),)), "boxes[0]: sides"),
    (dict(boxes=((-1, 0, 10, 10),)), "boxes[0] = (-1, 0, 10, 10) does not lie inside"),
    (dict(boxes=((0, -2, 10, 10),)), "does not lie inside"),
    (dict(boxes=((111, 0, 10, 10),)), "does not lie inside"),              # one column past the right edge
    (dict(boxes=((0, 91, 10, 10),)), "does not lie inside"),               # one row past the bottom edge
    (dict(boxes=((0, 0, 121, 10),)), "does not lie inside"),
    (dict(boxes=((0, 0, 10, 10), (30, 0, 10, 10)), index=(0, 2)), "photo_index[1] = 2"),
    (dict(boxes=((0, 0, 10, 10),), index=(-1,)), "photo_index[0] = -1"),
    (dict(ws=None), "workspace is NULL"),
]
INGEST_BAD = COMMON_BAD + [
    (dict(lr=7), " lr "), (dict(lr=65), " lr "), (dict(lr=-1), " lr "),
    (dict(res=0), " res "), (dict(res=96), " res "), (dict(res=576), " res "),
    (dict(out=None), "out is NULL"),
    (dict(out=OUT + 2), "out must be aligned"),
    (dict(ws_bytes=32 * 32 * 3 - 1), "workspace_bytes"),
]
PASTE_BAD = COMMON_BAD + [
    (dict(res=32), " res "), (dict(res=100), " res "), (dict(res=1024), " res "),
    (dict(feather=-1), "feather"), (dict(feather=257), "feather"),
    (dict(faces=None), "faces is NULL"),
    (dict(faces=FAC + 1), "faces must be aligned"),
    (dict(ws_bytes=64 * 64 * 3 - 1), "workspace_bytes"),
    (dict(boxes=((0, 0, 10, 10), (9, 9, 10, 10))), "boxes[0] and boxes[1] overlap"),
]


def _ids(cases):
    return ["%d-%s" % (i, n.strip().split(" ")[0].replace("[", "").replace("]", "").replace(":", "")) for i, (_, n) in enumerate(cases)]


@pytest.mark.parametrize("kw,names", INGEST_BAD, ids=_ids(INGEST_BAD))
def test_ingest_refuses_bad_arguments_before_any_device_work(kw, names):
    rc, msg = _ingest(**kw)
    assert rc == HD_ERR_INVALID, (rc, msg)
    assert msg.startswith("hd_face_ingest:") and names in msg, msg


@pytest.mark.parametrize("kw,names", PASTE_BAD, ids=_ids(PASTE_BAD))
def test_paste_refuses_bad_arguments_before_any_device_work(kw, names):
    rc, msg = _paste(**kw)
    assert rc == HD_ERR_INVALID, (rc, msg)
    assert msg.startswith("hd_face_paste:") and names in msg, msg


def test_workspace_queries():
    L = _lib.lib()
    assert L.hd_face_ingest_workspace(5, 32, 128) == 5 * 32 * 32 * 3
    assert L.hd_face_ingest_workspace(5, 0, 512) == 0                 # one resize: no intermediate image
    assert L.hd_face_paste_workspace(3, 128) == 3 * 128 * 128 * 3
    for args, name in (((0, 32, 128), "batch"), ((4097, 32, 128), "batch"), ((1, 4, 128), " lr "), ((1, 32, 100), " res ")):
        assert L.hd_face_ingest_workspace(*args) == HD_ERR_INVALID
        assert name in L.hd_last_error(None).decode()
    for args, name in (((0, 64), "batch"), ((1, 65), " res ")):
        assert L.hd_face_paste_workspace(*args) == HD_ERR_INVALID
        assert name in L.hd_last_error(None).decode()
    rc, msg = _ingest(lr=0, ws=None, ws_bytes=0, photos=None)         # lr 0 needs no workspace: the refusal names photos, not the workspace
    assert rc == HD_ERR_INVALID and "photos" in msg


def test_overlap_rule():
    """Touching boxes are allowed, one shared pixel is refused, equal boxes in different photos are allowed.  The C side gets past the
    overlap check in the allowed cases and refuses the (too small) workspace instead, still before any HIP call."""
    touching = ((0, 0, 10, 10), (10, 0, 10, 10), (0, 10, 10, 10), (10, 10, 5, 5))
    one_pixel = ((0, 0, 10, 10), (9, 9, 10, 10))
    assert photo.boxes_overlap(touching, (0, 0, 0, 0)) is None
    assert photo.boxes_overlap(one_pixel, (0, 0)) == (0, 1)
    assert photo.boxes_overlap(one_pixel, (0, 1)) is None
    assert photo.boxes_overlap(((0, 0, 10, 10), (20, 0, 5, 5), (3, 3, 1, 1)), (1, 1, 1)) == (0, 2)      # a box inside another
    for boxes, index in ((touching, (0, 0, 0, 0)), (one_pixel, (0, 1)), (one_pixel, (1, 0))):
        rc, msg = _paste(boxes=boxes, index=index, ws_bytes=1)
        assert rc == HD_ERR_INVALID and "workspace_bytes" in msg, msg
    for boxes, index in ((one_pixel, (0, 0)), (one_pixel, (1, 1)), (one_pixel, None)):
        rc, msg = _paste(boxes=boxes, index=index, ws_bytes=1)
        assert rc == HD_ERR_INVALID and "overlap" in msg, msg
    rc, msg = _ingest(boxes=one_pixel, ws_bytes=1)                    # the ingest only reads: overlapping boxes are fine there
    assert rc == HD_ERR_INVALID and "workspace_bytes" in msg, msg


def test_python_argument_checks():
    photos = pc.canvas()
    face = torch.zeros((1, 3, 64, 64))
    ok = [(0, 0, 10, 10)]
    for kw in (dict(lr=7), dict(lr=65), dict(lr=32.0), dict(res=96), dict(res=0), dict(res=576)):
        with pytest.raises(ValueError):
            photo.ingest(photos, ok, **kw)
    for boxes in ([(0, 0, 0, 10)], [(0, 0, 10, 2049)], [(-1, 0, 10, 10)], [(140, 0, 10, 10)], [(0, 125, 10, 10)]):
        with pytest.raises(ValueError):
            photo.ingest(photos, boxes)
        with pytest.raises(ValueError):
            photo.paste(photos, face, boxes)
    for index in ([2], [-1], [0, 0]):
        with pytest.raises(ValueError):
            photo.ingest(photos, ok, photo_index=index)
    for bad in (photos.float(), photos[0], photos[..., :2]):
        with pytest.raises(ValueError):
            photo.ingest(bad, ok)
    for kw in (dict(feather=-1), dict(feather=257), dict(feather=1.5)):
        with pytest.raises(ValueError):
            photo.paste(photos, face, ok, **kw)
    for f in (torch.zeros((2, 3, 64, 64)), torch.zeros((1, 3, 96, 96)), torch.zeros((1, 1, 64, 64)), torch.zeros((1, 3, 64, 128))):
        with pytest.raises(ValueError):
            photo.paste(photos, f, ok)
    with pytest.raises(ValueError):
        photo.paste(photos, torch.zeros((2, 3, 64, 64)), [(0, 0, 10, 10), (9, 9, 10, 10)])
    with pytest.raises(ValueError):
        photo.paste_reference(photos, torch.zeros((2, 3, 64, 64)), [(0, 0, 10, 10), (9, 9, 10, 10)])
    with pytest.raises(RuntimeError):                                 # well-formed, but no CPU path exists
        photo.ingest(photos, ok)
    with pytest.raises(RuntimeError):
        photo.paste(photos, face, ok)
    with pytest.raises(ValueError):
        photo.pil_bicubic_reference(photos[0].float(), (8, 8))
