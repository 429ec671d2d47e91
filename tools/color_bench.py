#!/usr/bin/env python3
"""What the colour correction costs: ms per call of hd_color_fix (wavelet with n = 5 levels, AdaIN) at batch 64 and 128 / 256 / 512 px,
against the same formula composed from torch ops on the same GPU (wavelet: c + B_5(s - c) as five F.pad + five grouped conv2d;
AdaIN: mean / var / elementwise), in fp32.  The two outputs are compared before anything is timed.  Device events around `reps`
back-to-back calls, after a warm-up of every shape; library and torch windows alternate over `rounds` rounds in one process and the
median is reported with the spread.  The last column is the traffic floor over the measured time: 12 bytes per pixel (read c, read s,
write out) at the HBM peak of 8.0 TB/s -- a share of the memory bound, not of anything else.
    python tools/color_bench.py [--batch 64] [--rounds 5] [--out profiles/r20_color_fix.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                                                      # bytes / s, the spec figure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_color_fix.txt"))
    a = ap.parse_args()
    import torch
    from hifidiff_amd import color
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/color_bench.py measures on the GPU; none is present (nothing is recorded)")
    B = a.batch

    def torch_wavelet(c, s):
        d = s - c
        for i in range(5):
            d = color.wavelet_blur(d, 2 ** i)
        return c + d

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    lines = ["tools/color_bench.py (MI355X): ms per call at batch %d, fp32 NCHW; hd = hd_color_fix (one launch), torch = the same formula from" % B,
             "torch ops on the same GPU.  Device events around back-to-back calls, %d alternating rounds, median (min .. max).  floor = 12 B per" % max(3, a.rounds),
             "pixel at 8.0 TB/s over the hd time.  max|hd - torch| is taken before timing.", "",
             "%-8s %5s  %-26s  %-26s  %7s  %7s  %s" % ("mode", "px", "hd ms", "torch ms", "torch/hd", "floor", "max|hd - torch|")]
    g = torch.Generator(device="cuda").manual_seed(20)
    for R in [int(v) for v in a.sizes.split(",")]:
        c = torch.rand((B, 3, R, R), device="cuda", generator=g) * 2 - 1
        s = torch.rand((B, 3, R, R), device="cuda", generator=g) * 2 - 1
        for mode, tfn in (("wavelet", lambda: torch_wavelet(c, s)), ("adain", lambda: color.adain_color_fix_reference(c, s))):
            hfn = lambda: color.color_fix(c, s, mode=mode)             # noqa: E731
            diff = float((hfn() - tfn()).abs().max())
            if not diff <= 1e-4:
                raise SystemExit("%s at %d px: hd_color_fix and the torch composition differ by %.3e; nothing is timed" % (mode, R, diff))
            for _ in range(3):                                         # warm-up of this shape, both sides
                hfn(); tfn()
            torch.cuda.synchronize()
            hreps = max(10, min(200, int(250.0 / max(window(hfn, 5), 1e-3)) + 1))           # windows of about a quarter second
            treps = max(3, min(50, int(250.0 / max(window(tfn, 2), 1e-3)) + 1))
            hd, th = [], []
            for _ in range(max(3, a.rounds)):
                hd.append(window(hfn, hreps)); th.append(window(tfn, treps))
            hd.sort(); th.sort()
            hm, tm = hd[len(hd) // 2], th[len(th) // 2]
            floor_ms = 1e3 * 12.0 * B * 3 * R * R / HBM_PEAK
            lines.append("%-8s %5d  %-26s  %-26s  %7.1fx  %6.1f%%  %.2e" % (
                mode, R, "%.4f (%.4f .. %.4f)" % (hm, hd[0], hd[-1]), "%.4f (%.4f .. %.4f)" % (tm, th[0], th[-1]), tm / hm, 100 * floor_ms / hm, diff))
        del c, s
    lines += ["", "hd ms includes color_fix's output allocation (torch's caching allocator) and the ctypes call; both sides run on torch's current stream."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
