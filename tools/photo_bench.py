#!/usr/bin/env python3
"""What the photo ends cost: ms per call of photo.ingest (lr 32 and 0, res 128 and 512) and photo.paste (feather 0 and 16, 128 px faces)
for 64 faces from eight 1920 x 1080 photos with boxes of about 400 px, against
  - the reference's way: a Python loop over PIL images on the CPU, ONE thread (crop, resize, resize, np.asarray; the host-to-device copy
    of the result is not included), where Pillow is installed;
  - a torch composition on the same GPU: per face F.interpolate(mode="bicubic", antialias=True).  It is not bit-equal to Pillow (fp32
    weights, no uint8 intermediate) and is there for its time only.
The library's bytes are compared with photo.ingest_reference / paste_reference on a few faces before anything is timed.  Device events
around `reps` back-to-back calls after a warm-up, library and torch windows alternating over `rounds` rounds; median (min .. max).
floor = (box bytes read + output bytes written; paste: faces read + box bytes read and written) at the HBM peak of 8.0 TB/s over the
library's time -- a share of the memory bound.
    python tools/photo_bench.py [--rounds 5] [--out profiles/r24_photo.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                                                      # bytes / s, the spec figure
N, H, W, PER = 8, 1080, 1920, 8                                        # photos, their size, faces per photo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_photo.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from hifidiff_amd import photo
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/photo_bench.py measures on the GPU; none is present (nothing is recorded)")
    try:
        from PIL import Image
    except ImportError:
        Image = None
    g = torch.Generator().manual_seed(24)
    photos_cpu = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    photos = photos_cpu.cuda()
    boxes, idx = [], []
    for p in range(N):                                                 # eight heads a photo on a 4 x 2 grid of 480 x 540 cells: no overlap
        for k in range(PER):
            w, h = (int(v) for v in torch.randint(380, 421, (2,), generator=g))
            cx, cy = (k % 4) * 480, (k // 4) * 540
            boxes.append((cx + int(torch.randint(0, 480 - w + 1, (1,), generator=g)), cy + int(torch.randint(0, 540 - h + 1, (1,), generator=g)), w, h))
            idx.append(p)
    boxes, idx = np.asarray(boxes, dtype=np.int32), np.asarray(idx, dtype=np.int32)
    B = len(boxes)
    box_bytes = int((boxes[:, 2] * boxes[:, 3]).sum()) * 3

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def timed(hfn, tfn):
        for _ in range(3):
            hfn(); tfn()
        torch.cuda.synchronize()
        hreps = max(5, min(200, int(250.0 / max(window(hfn, 3), 1e-3)) + 1))
        treps = max(2, min(50, int(250.0 / max(window(tfn, 2), 1e-3)) + 1))
        hd, th = [], []
        for _ in range(max(3, a.rounds)):
            hd.append(window(hfn, hreps)); th.append(window(tfn, treps))
        hd.sort(); th.sort()
        return hd, th

    def fmt(v):
        return "%.4f (%.4f .. %.4f)" % (v[len(v) // 2], v[0], v[-1])

    def torch_ingest(lr, res):
        out = []
        for (l, t, w, h), p in zip(boxes.tolist(), idx.tolist()):
            x = photos[p, t:t + h, l:l + w].permute(2, 0, 1)[None].float()
            if lr:
                x = F.interpolate(x, size=(lr, lr), mode="bicubic", antialias=True)
            out.append(F.interpolate(x, size=(res, res), mode="bicubic", antialias=True))
        return torch.cat(out).div_(255)

    def pil_ingest(lr, res):
        out = []
        for (l, t, w, h), p in zip(boxes.tolist(), idx.tolist()):
            im = Image.fromarray(photos_cpu[p].numpy()).crop((l, t, l + w, t + h))
            if lr:
                im = im.resize((lr, lr), Image.BICUBIC)
            out.append(np.asarray(im.resize((res, res), Image.BICUBIC)))
        return out

    def cpu_ms(fn):
        t = []
        for _ in range(3):
            t0 = time.perf_counter(); fn(); t.append(1e3 * (time.perf_counter() - t0))
        return "%.1f" % sorted(t)[1]

    lines = ["tools/photo_bench.py (MI355X): ms per call for %d faces from %d photos of %d x %d, boxes of 380 .. 420 px.  hd = hifidiff_amd.photo" % (B, N, W, H),
             "(output allocation and the ctypes call included), torch = F.interpolate(antialias=True) per face on the same GPU (not bit-equal, time",
             "only), PIL = the reference's loop over PIL images on the CPU, one thread, median of 3 (%s).  Device events, %d alternating rounds," % (
                 "Pillow " + __import__("PIL").__version__ if Image else "Pillow is not installed here: not measured", max(3, a.rounds)),
             "median (min .. max).  floor = the bytes the call must move at 8.0 TB/s over the hd time.", "",
             "%-22s  %-26s  %-28s  %8s  %8s  %7s" % ("call", "hd ms", "torch ms", "torch/hd", "PIL ms", "floor")]
    few = [0, 9, 63]
    for lr, res in ((32, 128), (0, 128), (32, 512), (0, 512)):
        _, got = photo.ingest(photos, boxes[few], idx[few], lr=lr, res=res, return_uint8=True)
        _, want = photo.ingest_reference(photos_cpu, boxes[few], idx[few], lr=lr, res=res, return_uint8=True)
        if not torch.equal(got.cpu(), want):
            raise SystemExit("ingest lr %d res %d differs from the reference; nothing is timed" % (lr, res))
        hd, th = timed(lambda: photo.ingest(photos, boxes, idx, lr=lr, res=res), lambda: torch_ingest(lr, res))
        floor_ms = 1e3 * (box_bytes + B * 3 * res * res * 4) / HBM_PEAK
        lines.append("%-22s  %-26s  %-28s  %7.1fx  %8s  %6.2f%%" % ("ingest lr %d res %d" % (lr, res), fmt(hd), fmt(th), th[len(th) // 2] / hd[len(hd) // 2],
                                                                cpu_ms(lambda: pil_ingest(lr, res)) if Image else "-", 100 * floor_ms / hd[len(hd) // 2]))
    res = 128
    faces = torch.rand((B, 3, res, res), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    work = photos.clone()
    for feather in (0, 16):
        got = photo.paste(photos[:1], faces[:2], boxes[:2], idx[:2], feather=feather)
        want = photo.paste_reference(photos_cpu[:1], faces[:2].cpu(), boxes[:2], idx[:2], feather=feather)
        if not torch.equal(got.cpu(), want):
            raise SystemExit("paste feather %d differs from the reference; nothing is timed" % feather)
        masks = [photo.feather_mask(int(w), int(h), feather, device="cuda").float().div(256)[None] for _, _, w, h in boxes.tolist()]

        def torch_paste():
            for f, ((l, t, w, h), p) in enumerate(zip(boxes.tolist(), idx.tolist())):
                q = F.interpolate(faces[f:f + 1], size=(h, w), mode="bicubic", antialias=True)[0].clamp(0, 1) * 255
                reg = work[p, t:t + h, l:l + w].permute(2, 0, 1)
                reg.copy_((reg.float() * (1 - masks[f]) + q * masks[f] + 0.5).to(torch.uint8))

        def pil_paste():
            fc = (faces.cpu().clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).numpy()
            for f, (l, t, w, h) in enumerate(boxes.tolist()):
                np.asarray(Image.fromarray(fc[f]).resize((w, h), Image.BICUBIC))

        hd, th = timed(lambda: photo.paste(work, faces, boxes, idx, feather=feather, inplace=True), torch_paste)
        floor_ms = 1e3 * (2 * box_bytes + B * 3 * res * res * 4) / HBM_PEAK
        lines.append("%-22s  %-26s  %-28s  %7.1fx  %8s  %6.2f%%" % ("paste feather %d (128)" % feather, fmt(hd), fmt(th), th[len(th) // 2] / hd[len(hd) // 2],
                                                                cpu_ms(pil_paste) if Image else "-", 100 * floor_ms / hd[len(hd) // 2]))
    lines += ["", "PIL ms of the paste rows is the resize loop alone (no blend, no copies); its ingest rows do not include the host-to-device copy."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
