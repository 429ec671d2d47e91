#!/usr/bin/env python3
"""End-to-end latent-space pipeline of `ddim_sample` (test_refiner.py:58-95) on an MI355X, with synthetic weights:

    cr_face   = CoarseRestoration()(ln_face)                 # hifidiff_amd.cr          (test_refiner.py:77)
    cr_latent = vae.encode(bicubic(cr_face)).latent_dist.sample() * 0.18215   # hifidiff_amd.vae (test_refiner.py:78-83)
    latent    = 50-step DDIM with FacialRefiner              # hifidiff_amd.refiner + sampling (test_refiner.py:85-91)
                (or --scheduler dpmpp2m: DPM-Solver++ 2M, the usual diffusers swap for fewer evaluations, e.g. --steps 20)
    images    = vae.decode(latent / 0.18215).sample          # hifidiff_amd.vae         (test_refiner.py:93)

    python examples/pipeline.py [--batch 8] [--scheduler ddim|dpmpp2m] [--steps 50] [--strength 0.6]
    python examples/pipeline.py --stream 200 [--refill-every 5] [--batch 64]    # continuous batching of 200 requests, mixed strengths
    python examples/pipeline.py --stream 200 --steps-mix 10,20,50    # the requests cycle through schedules of 10, 20 and 50 steps in one batch
    python examples/pipeline.py --preview-every 10          # decode every 10th row's denoised estimate: how the image forms
    python examples/pipeline.py --stream 200 --preview-every 1      # one progress line per step() of the serving loop
    python examples/pipeline.py --mask-box 32,40,96,72 --mask-box 48,84,80,108 [--strength 0.8]   # inpainting: resample the boxes (pixels of
                                                          # the 128 x 128 face), keep the coarse restoration everywhere else
    python examples/pipeline.py --fidelity 0.5 [--fidelity-scale 4] [--fidelity-rows 0,30]   # low-pass guidance towards the coarse restoration:
                                                          # its structure and colour stay, the diffusion adds the detail
    python examples/pipeline.py --color-fix wavelet [--color-weight 0.8]    # after the decode: the image keeps its detail and takes the
                                                          # coarse restoration's colour (hd_color_fix; also with --stream)
    python examples/pipeline.py --metrics [--preview-every 10]    # the reference loop's scores: PSNR / SSIM of the final image against
                                                          # cr_face, and of every preview against the final image (hd_image_metrics)
    python examples/pipeline.py --metrics --lpips-weights alexnet.pth,lin.pth    # also LPIPS (hd_lpips) with a local AlexNet file and the lin
                                                          # layers' file; --lpips-synthetic: synthetic weights, to see the call run
    python examples/pipeline.py --from-photos 8 [--feather 8]     # photo in, photo out: head boxes of synthetic photos become ln_face
                                                          # (photo.ingest: Pillow's crop -> 32 -> 128 bicubic, on the GPU), the restored faces
                                                          # are pasted back into the photos (photo.paste)
    python examples/pipeline.py --photo group.jpg --box 410,120,380,400 [--box ...] [--save out.png]    # the same for a real file (PIL reads
                                                          # and writes the file; the resampling runs on the GPU)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hifidiff_amd import color, metrics, photo, sampling, schedulers, synth        # noqa: E402
from hifidiff_amd.cr import CoarseRestoration                            # noqa: E402
from hifidiff_amd.refiner import FacialRefiner                           # noqa: E402
from hifidiff_amd.vae import AutoencoderKL                               # noqa: E402


def decode(a, vae, latents, cr_face):
    """images = vae.decode(latents / 0.18215).sample; with --color-fix the colour-corrected images (hd_color_fix on the decode's stream,
    the reference resampled inside the call when the sizes differ) and a line with the colour distance to cr_face before and after."""
    if a.color_fix is None:
        return vae.decode(latents / 0.18215).sample                    # the reference's call form; decode_scaled(latents) is the fused one
    images = vae.decode_scaled(latents)
    # one call does both: vae.decode_scaled(latents, color_ref=cr_face, color_mode=..., color_weight=...); here the plain images are wanted too
    fixed = color.color_fix(images, cr_face, mode=a.color_fix, weight=a.color_weight)
    ref = cr_face if cr_face.shape[-1] == images.shape[-1] else F.interpolate(cr_face, images.shape[-1], mode="bicubic", align_corners=False)
    dist = lambda x: float((x.mean(dim=(-2, -1)) - ref.mean(dim=(-2, -1))).abs().mean())   # noqa: E731
    print(f"colour fix {a.color_fix}, weight {1.0 if a.color_weight is None else a.color_weight}: mean |channel mean - cr_face's| "
          f"{dist(images):.4f} before, {dist(fixed):.4f} after")
    return fixed


def scores(result, target, lpips=None):
    """Mean PSNR / SSIM (and LPIPS, given a loaded model) over the faces, scored as the reference's evaluation loop does
    (metrics.evaluate: resampled to the target's size, both min-max normalised over the batch; two hd_image_metrics calls and one
    hd_lpips call on the current stream)."""
    ev = metrics.evaluate(result, target, lpips=lpips)
    text = f"PSNR {float(ev.psnr.mean()):.2f} dB, SSIM {float(ev.ssim.mean()):.4f}"
    return text if ev.lpips is None else text + f", LPIPS {float(ev.lpips.mean()):.4f}"


def lpips_model(a, dev):
    """--lpips-weights A,B: a torchvision AlexNet state dict and the lin layers' state dict, two local files.  --lpips-synthetic:
    synthetic weights."""
    if a.lpips_weights is None and not a.lpips_synthetic:
        return None
    if a.lpips_weights is not None:
        m = metrics.LPIPS.from_files(*a.lpips_weights.split(","))
    else:
        m = metrics.LPIPS()
        m.load_state_dict(synth.lpips_state_dict())
        print("LPIPS: the weights are synthetic; the number is not comparable to published LPIPS")
    return m.to(dev)


def load_photos(a, dev):
    """--from-photos N: ceil(N / 4) synthetic 720 x 540 photos with four head boxes each; --photo FILE --box l,t,w,h: a real file.
    Returns uint8 photos [n,H,W,3] on the GPU and the host's boxes [B,4] and photo indices [B]."""
    if a.photo is not None:
        from PIL import Image                                          # file I/O only
        img = torch.from_numpy(np.asarray(Image.open(a.photo).convert("RGB")).copy())[None]
        boxes = np.asarray([[int(v) for v in b.split(",")] for b in a.box], dtype=np.int32)
        return img.to(dev), boxes, np.zeros(len(boxes), dtype=np.int32)
    n = (a.from_photos + 3) // 4
    img = torch.from_numpy(np.stack([synth.photo(f"photo/{k}", 540, 720) for k in range(n)]))
    g = torch.Generator().manual_seed(11)
    boxes = []
    for f in range(a.from_photos):                                     # one box per 360 x 270 quarter: no two overlap
        w, h = (int(v) for v in torch.randint(150, 251, (2,), generator=g))
        cx, cy = (f % 2) * 360, (f // 2 % 2) * 270
        boxes.append((cx + int(torch.randint(0, 360 - w + 1, (1,), generator=g)), cy + int(torch.randint(0, 270 - h + 1, (1,), generator=g)), w, h))
    return img.to(dev), np.asarray(boxes, dtype=np.int32), np.arange(a.from_photos, dtype=np.int32) // 4


def paste_back(a, photos, boxes, pidx, ln_face, images):
    """The restored faces go back into the photos (photo.paste: quantise, Pillow's bicubic to the box, feathered blend).  Prints that no
    byte outside the boxes moved and the PSNR inside the boxes against the original photo, for the degraded input and for the result."""
    inside = torch.zeros(photos.shape[:3], dtype=torch.bool, device=photos.device)
    for (l, t, w, h), p in zip(boxes.tolist(), pidx.tolist()):
        inside[p, t:t + h, l:l + w] = True
    before = photo.paste(photos, ln_face, boxes, pidx, feather=a.feather)
    after = photo.paste(photos, (images.clamp(-1, 1) + 1) / 2, boxes, pidx, feather=a.feather)

    def psnr(x):
        mse = float(((x[inside].float() - photos[inside].float()) ** 2).mean())
        return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))
    moved = int((after[~inside] != photos[~inside]).sum())
    print(f"paste-back of {len(boxes)} faces into {photos.shape[0]} photos of {photos.shape[2]} x {photos.shape[1]}, feather {a.feather}: "
          f"{moved} bytes outside the boxes changed; PSNR inside the boxes against the photo: {psnr(before):.2f} dB with the degraded "
          f"input pasted, {psnr(after):.2f} dB with the result" + (" (synthetic weights: the result is not a face)" if a.photo is None else ""))
    if a.save is not None:
        from PIL import Image
        Image.fromarray(after[0].cpu().numpy()).save(a.save)
        print(f"wrote {a.save}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scheduler", choices=("ddim", "dpmpp2m"), default="ddim")
    ap.add_argument("--steps", type=int, default=None, help="denoiser evaluations per face (default: 50 for ddim, 20 for dpmpp2m)")
    ap.add_argument("--strength", type=float, default=None,
                    help="img2img: start from cr_latent noised to this strength (diffusers' convention; default: off, pure-noise start)")
    ap.add_argument("--stream", type=int, default=None, metavar="N",
                    help="continuous batching: N synthetic requests with strengths in [0.2, 1.0] through sampling.ContinuousSampler "
                         "(--batch slots), then VAE decode")
    ap.add_argument("--refill-every", type=int, default=5, metavar="K", help="--stream: iterations per call between refills")
    ap.add_argument("--prefetch", type=int, default=0, metavar="P",
                    help="--stream: prepare the conditioning of up to P queued requests ahead, in one call, and refill slots by copy "
                         "(sampling.ContinuousSampler(prefetch=P), hd_pool_prepare / hd_pool_commit; 0: prepare at every refill)")
    ap.add_argument("--steps-mix", default=None, metavar="N1,N2,..",
                    help="--stream: per-request schedules -- the requests cycle through these step counts of --scheduler, all in the same "
                         "slots (sampling.ScheduleSet, hd_sample_spans)")
    ap.add_argument("--mask-box", action="append", default=None, metavar="x0,y0,x1,y1",
                    help="inpainting: resample this pixel box of the 128 x 128 face and keep cr_latent elsewhere (repeatable; composes with "
                         "--strength, --scheduler and --stream)")
    ap.add_argument("--preview-every", type=int, default=None, metavar="N",
                    help="progress previews: decode the denoised estimate of every N-th row through the VAE and print its mean absolute "
                         "difference to the final image; with --stream: one progress line per step()")
    ap.add_argument("--fidelity", type=float, default=None, metavar="W",
                    help="low-pass guidance towards cr_latent with weight W in (0, 1]: x0 <- x0 + W (LP_N(cr_latent) - LP_N(x0)) on every "
                         "guided row (composes with --strength, --mask-box, --scheduler and --stream)")
    ap.add_argument("--fidelity-scale", type=int, default=4, metavar="N",
                    help="--fidelity: block size N of the low-pass filter, a divisor of 16 (1: every element, 16: only each channel's mean)")
    ap.add_argument("--fidelity-rows", default=None, metavar="A,B", help="--fidelity: guide rows A <= j < B of each face's own schedule (default: all)")
    ap.add_argument("--color-fix", choices=tuple(color.MODES), default=None,
                    help="colour-correct the decoded images against cr_face: wavelet (five a-trous levels: the image's detail on the "
                         "reference's low frequencies) or adain (the reference's per-channel mean and deviation); composes with everything")
    ap.add_argument("--color-weight", type=float, default=None, metavar="W", help="--color-fix: weight of the correction in [0, 1] (default 1)")
    ap.add_argument("--metrics", action="store_true",
                    help="score the final images against cr_face (mean PSNR / SSIM over the faces, the reference loop's scoring) and, with "
                         "--preview-every, every decoded preview against the final images; also with --stream")
    ap.add_argument("--lpips-weights", default=None, metavar="A,B",
                    help="--metrics: also LPIPS-AlexNet, with a torchvision AlexNet state dict A and the lin layers' state dict B (local files)")
    ap.add_argument("--lpips-synthetic", action="store_true",
                    help="--metrics: also LPIPS with synthetic weights (the number is not comparable to published LPIPS)")
    ap.add_argument("--from-photos", type=int, default=None, metavar="N",
                    help="photo in, photo out: N head boxes of synthetic photos are ingested as ln_face (photo.ingest), run through the "
                         "pipeline and pasted back (photo.paste); replaces --batch")
    ap.add_argument("--photo", default=None, metavar="FILE", help="as --from-photos for an image file (needs PIL for the file I/O) and --box")
    ap.add_argument("--box", action="append", default=None, metavar="l,t,w,h", help="--photo: a head box (repeatable; boxes must not overlap)")
    ap.add_argument("--feather", type=int, default=8, metavar="PX", help="--from-photos / --photo: width of the blended edge of the paste, 0..256")
    ap.add_argument("--save", default=None, metavar="FILE", help="--from-photos / --photo: write the first photo with the faces pasted back (needs PIL)")
    a = ap.parse_args()
    if a.photo is not None and not a.box:
        ap.error("--photo needs at least one --box l,t,w,h")
    if (a.photo is not None or a.from_photos is not None) and a.stream is not None:
        ap.error("--from-photos / --photo run the batch pipeline, not --stream")
    if (a.lpips_weights is not None or a.lpips_synthetic) and not a.metrics:
        ap.error("--lpips-weights / --lpips-synthetic need --metrics")
    if a.lpips_weights is not None and len(a.lpips_weights.split(",")) != 2:
        ap.error("--lpips-weights takes two files: A,B")
    if a.color_weight is not None and (a.color_fix is None or not 0.0 <= a.color_weight <= 1.0):
        ap.error("--color-weight needs --color-fix and a value in [0, 1]")
    if a.preview_every is not None and a.preview_every < 1:
        ap.error("--preview-every must be >= 1")
    if a.fidelity is None and (a.fidelity_rows is not None or a.fidelity_scale != 4):
        ap.error("--fidelity-scale / --fidelity-rows need --fidelity")
    a.fid_rows = None if a.fidelity_rows is None else tuple(int(v) for v in a.fidelity_rows.split(","))
    a.mask = None
    if a.mask_box:
        a.mask = sampling.region_mask([tuple(int(v) for v in b.split(",")) for b in a.mask_box], 16)
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)

    cr = CoarseRestoration()
    cr.load_state_dict(synth.cr_state_dict())            # real use: torch.load(cr_ckpt)["model_state_dict"]
    cr.to(dev)
    vae = AutoencoderKL()
    vae.load_state_dict(synth.vae_state_dict())          # real use: AutoencoderKL.from_pretrained(<local sd-2-1-base dir>, subfolder="vae")
    vae.to(dev)
    model = FacialRefiner(latent_res=16)
    model.load_state_dict(synth.refiner_state_dict(16))  # real use: safetensors.torch.load_file(refiner_ckpt)
    model.to(dev)
    a.lpips = lpips_model(a, dev)
    if a.scheduler == "ddim":
        sch = schedulers.DDIMScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear", prediction_type="epsilon",
                                       clip_sample_range=3.0)
    else:                                                # same network, same ODE, second-order multistep solver
        sch = schedulers.DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_schedule="scaled_linear",
                                                     prediction_type="epsilon", solver_order=2, algorithm_type="dpmsolver++")
    steps = a.steps or (50 if a.scheduler == "ddim" else 20)

    if a.steps_mix and a.stream is None:
        ap.error("--steps-mix needs --stream")
    if a.prefetch and a.stream is None:
        ap.error("--prefetch needs --stream")
    if a.prefetch < 0:
        ap.error("--prefetch must be >= 0")
    if a.stream is not None:
        return stream(a, cr, vae, model, sch, steps, dev)

    B = a.batch
    photos = None
    if a.from_photos is not None or a.photo is not None:               # ln_face as every dataset class of the reference builds it, on the GPU
        photos, boxes, pidx = load_photos(a, dev)
        B = len(boxes)
        ln_face = photo.ingest(photos, boxes, pidx, lr=32, res=128)
    else:
        ln_face = torch.from_numpy(np.stack([synth.rand(f"ln_face/{f}", (3, 128, 128)) for f in range(B)])).to(dev)
    latent = torch.randn(B, 4, 16, 16, device=dev)

    torch.cuda.synchronize(); t0 = time.time()
    cr_face = cr(ln_face)
    torch.cuda.synchronize(); t1 = time.time()
    cr_latent = vae.encode_scaled(cr_face, 128, seed=7)                # bicubic (identity at 128) + encode + sample + x 0.18215
    torch.cuda.synchronize(); t2 = time.time()
    sch.set_timesteps(steps)
    pv = {} if a.preview_every is None else {"previews": a.preview_every}
    if a.fidelity is not None:                                         # the coarse restoration's low frequencies stay (set_guidance checks the values)
        pv.update(guide=cr_latent, guide_weight=a.fidelity, guide_scale=a.fidelity_scale, guide_rows=a.fid_rows)
    if a.mask is not None:                                             # inpainting: the boxes are resampled, the rest stays cr_latent
        latent, start, nz = sampling.inpaint_start(sch, cr_latent, 1.0 if a.strength is None else a.strength, noise=latent)
        out = sampling.sample(model, latent, cr_face, cr_latent, sch, start_steps=start, mask=a.mask[None].expand(B, 16, 16),
                              known=cr_latent, known_noise=nz, **pv)
    elif a.strength is None:
        out = sampling.sample(model, latent, cr_face, cr_latent, sch, **pv)   # conditioning once + graph-replayed loop
    else:                                                              # img2img: noise cr_latent to timesteps[start], run the remaining rows
        latent, start = sampling.img2img_start(sch, cr_latent, a.strength, noise=latent)
        out = sampling.sample(model, latent, cr_face, cr_latent, sch, start_steps=start, **pv)
    snaps = None
    if a.preview_every is not None:
        out, snaps, snap_rows = out
    if a.fidelity is not None:
        lp = lambda t: sampling.low_pass(t, a.fidelity_scale)         # noqa: E731
        print(f"fidelity {a.fidelity} at N = {a.fidelity_scale}: mean |LP(latent) - LP(cr_latent)| {float((lp(out) - lp(cr_latent)).abs().mean()):.4f}")
    torch.cuda.synchronize(); t3 = time.time()
    images = decode(a, vae, out, cr_face)
    torch.cuda.synchronize(); t4 = time.time()
    for s in range(0 if snaps is None else snaps.shape[0]):            # the estimate of every N-th row as an image (hd_vae_decode)
        ran = snap_rows[s] >= 0                                        # img2img: a face that started later has not run this row
        if bool(ran.any()):
            img = vae.decode(snaps[s][ran] / 0.18215).sample
            print(f"preview {s}: row {int(snap_rows[s][ran].max())} of {steps}, {int(ran.sum())} faces, mean |image - final| "
                  f"{float((img - images[ran]).abs().mean()):.4f}" + (f", {scores(img, images[ran], a.lpips)}" if a.metrics else ""))
    if a.metrics:
        print(f"final images against cr_face: {scores(images, cr_face, a.lpips)}")
    if photos is not None:
        paste_back(a, photos, boxes, pidx, ln_face, images)
    print(f"batch {B}: coarse restoration {1e3 * (t1 - t0):.1f} ms, VAE encode {1e3 * (t2 - t1):.1f} ms, {steps}-step {a.scheduler} "
          f"{1e3 * (t3 - t2):.1f} ms, VAE decode {1e3 * (t4 - t3):.1f} ms; latent range [{float(out.min()):.2f}, {float(out.max()):.2f}], "
          f"images {tuple(images.shape)} finite {bool(torch.isfinite(images).all())}")


def stream(a, cr, vae, model, sch, steps, dev):
    """N requests, each with its own seed and strength, through the serving loop: a finished face leaves its slot and the next request
    takes it (FacialRefiner.prepare_slots; with --prefetch its conditioning was prepared ahead, together with that of the requests queued
    behind it, and FacialRefiner.pool_commit copies it in), so no slot waits for the slowest face of a batch."""
    N = a.stream
    g = torch.Generator().manual_seed(3)
    strength = (0.2 + 0.8 * torch.rand(N, generator=g)).tolist()
    torch.cuda.synchronize(); t0 = time.time()
    reqs = []
    for b in range(0, N, 64):                                          # coarse restoration + VAE encode of the requests, 64 at a time
        n = min(64, N - b)
        ln_face = torch.from_numpy(np.stack([synth.rand(f"ln_face/{f}", (3, 128, 128)) for f in range(b, b + n)])).to(dev)
        cr_face = cr(ln_face)
        cr_latent = vae.encode_scaled(cr_face, 128, seed=7 + b)
        reqs += [(cr_face[i], cr_latent[i]) for i in range(n)]
    sch.set_timesteps(steps)
    pick = [None] * N
    if a.steps_mix:                                                    # one schedule per step count, every request on its own
        import copy
        counts = [int(v) for v in a.steps_mix.split(",")]
        members = {n: copy.deepcopy(sch) for n in counts}
        for n, s in members.items():
            s.set_timesteps(n)
        sch, steps = sampling.ScheduleSet(members), a.steps_mix
        pick = [counts[i % len(counts)] for i in range(N)]
    cs = sampling.ContinuousSampler(model, sch, batch=a.batch, refill_every=a.refill_every, previews=a.preview_every is not None,
                                    prefetch=a.prefetch)
    torch.cuda.synchronize(); t1 = time.time()
    fid = {} if a.fidelity is None else dict(fidelity=a.fidelity, fidelity_scale=a.fidelity_scale, fidelity_rows=a.fid_rows)
    ids = [cs.submit(f, l, seed=1000 + i, strength=strength[i], mask=a.mask, **fid, **({"schedule": pick[i]} if a.steps_mix else {}))
           for i, (f, l) in enumerate(reqs)]
    out = {}
    while cs.busy():
        cs.step()
        out.update(cs.poll())
        if a.preview_every is not None:                                # what a front end would show: every running request's x0
            pr = cs.previews()
            if pr:
                done = sum(d for d, _, _ in pr.values()) / sum(t for _, t, _ in pr.values())
                spread = torch.stack([x0 for _, _, x0 in pr.values()]).std()
                print(f"call {cs.calls}: {len(pr)} requests running, {100 * done:.0f}% of their rows done, {len(out)} finished, "
                      f"x0 std {float(spread):.3f}")
    torch.cuda.synchronize(); t2 = time.time()
    lat = torch.stack([out[i] for i in ids])
    cr_faces = torch.stack([f for f, _ in reqs])
    images = decode(a, vae, lat, cr_faces)
    torch.cuda.synchronize(); t3 = time.time()
    if a.metrics:
        print(f"final images against cr_face: {scores(images, cr_faces, a.lpips)}")
    print(f"stream of {N} requests (strength 0.2..1.0), {a.batch} slots, refill every {a.refill_every}: coarse restoration + VAE encode "
          f"{1e3 * (t1 - t0):.1f} ms, {steps}-step {a.scheduler} {1e3 * (t2 - t1):.1f} ms ({N / (t2 - t1):.1f} faces/s, {cs.calls} calls, "
          f"{cs.refilled} slots refilled{f', {cs.pool_prepared} of them prepared ahead in {cs.pool_calls} calls' if a.prefetch else ''}), VAE decode {1e3 * (t3 - t2):.1f} ms; images {tuple(images.shape)} finite "
          f"{bool(torch.isfinite(images).all())}")


if __name__ == "__main__":
    main()
