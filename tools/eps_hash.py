"""sha256 of eps (batch 7 with per-face timesteps, batch 64 shared timestep), of 12 DDPM steps at batch 64 and of one call of every
entry point beside the sampling loop (CoarseRestoration, the VAE boundary, colour fix, PSNR / SSIM, LPIPS, photo ingest and paste) on
synthetic weights and fixed inputs: two builds of the library that claim the same arithmetic must print the same lines.
usage: python tools/eps_hash.py [repo root of the build]"""
import hashlib
import os
import sys

root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch  # noqa: E402
from hifidiff_amd import color, metrics, photo, sampling, schedulers, synth  # noqa: E402
from hifidiff_amd.cr import CoarseRestoration  # noqa: E402
from hifidiff_amd.refiner import FacialRefiner  # noqa: E402
from hifidiff_amd.vae import AutoencoderKL  # noqa: E402

torch.set_grad_enabled(False)
m = FacialRefiner(16); m.load_state_dict(synth.refiner_state_dict(16)); m.to("cuda:0")
h = lambda *ts: hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in ts)).hexdigest()[:16]  # noqa: E731
x, crl, crf = [t.cuda() for t in synth.sample_inputs(7, 16)]
print("eps B=7 per-face ", h(m(x, torch.tensor([980., 500., 0., 37., 861., 250., 999.]), crf, crl).sample))
x, crl, crf = [t.cuda() for t in synth.sample_inputs(64, 16)]
print("eps B=64 t=500   ", h(m(x, 500, crf, crl).sample))
sch = schedulers.DDPMScheduler(clip_sample_range=3.0); sch.timesteps = sch.timesteps[:12]
print("ddpm12 B=64      ", h(sampling.sample(m, x, crf, crl, sch, seed=3)))
del m

G = lambda a: torch.from_numpy(a).cuda()  # noqa: E731

cr = CoarseRestoration(); cr.load_state_dict(synth.cr_state_dict()); cr.to("cuda:0")
print("cr B=2           ", h(cr(G(synth.rand("hash.cr", (2, 3, 128, 128))))))
vae = AutoencoderKL(); vae.load_state_dict(synth.vae_state_dict()); vae.to("cuda:0")
img128, img64 = G(synth.rand("hash.img128", (2, 3, 128, 128))), G(synth.rand("hash.img64", (2, 3, 64, 64)))
print("vae encode 128>64", h(vae.encode_scaled(img128, 64, noise=G(synth.randn("hash.noise", (2, 4, 8, 8))))))
print("vae decode L=8   ", h(vae.decode_scaled(G(synth.randn("hash.lat", (2, 4, 8, 8))))))
print("color wavelet    ", h(color.color_fix(img64, img128, mode="wavelet")))
print("color adain      ", h(color.color_fix(img64, img128, mode="adain")))
for ch in ("y", "rgb"):
    r = metrics.image_metrics(img128, img64, channels=ch, normalize="face", ssim_map=True)
    print("metrics %-9s" % ch, h(r.mse, r.ssim, r.ssim_map, metrics.image_range(img128, 64), metrics.image_range(img64)))
lp = metrics.LPIPS(); lp.load_state_dict(synth.lpips_state_dict()); lp.to("cuda:0")
print("lpips B=2        ", h(*lp(img64, G(synth.rand("hash.ref64", (2, 3, 64, 64))), per_layer=True)))
import photo_cases  # noqa: E402  (tests/: the golden photos and their box list)
idx, boxes = [a[:2] for a in photo_cases.boxes()]
photos = photo_cases.canvas().cuda()
faces, u8 = photo.ingest(photos, boxes, idx, lr=32, res=128, return_uint8=True)
print("photo ingest     ", h(faces, u8))
print("photo paste      ", h(photo.paste(photos, faces.flip(-1), boxes, idx, feather=4)))
