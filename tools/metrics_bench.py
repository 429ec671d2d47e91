#!/usr/bin/env python3
"""What the image metrics cost, and how exact they are.  First the measured errors of hd_image_metrics / hd_image_range against the
float64 formulas with their torch-fp32 yardsticks (tools/metrics_cases.py, the figures tests/test_metrics.py asserts on).  Then ms per
call at batch 64 and 128 / 256 / 512 px of hd_image_metrics in the y and rgb modes and of hd_image_range, each against the same formula
composed from torch ops on the same GPU in fp32 (metrics.image_metrics_reference: five grouped 11 x 11 separable convolutions on five
moment maps, about 25 ops; range: amin + amax).  The composition is the comparison, not the code under test; the two results are compared
before anything is timed.  Device events around `reps` back-to-back calls, after a warm-up of every shape; library and torch windows
alternate over `rounds` rounds in one process and the median is reported with the spread.  floor = the traffic floor over the measured
time: 24 bytes per pixel position (both images read once, three fp32 channels each; 12 for the range) at the HBM peak of 8.0 TB/s.
    python tools/metrics_bench.py [--batch 64] [--rounds 5] [--out profiles/r22_metrics.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8.0e12                                                      # bytes / s, the spec figure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_metrics.txt"))
    a = ap.parse_args()
    import torch
    from hifidiff_amd import metrics
    import metrics_cases
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/metrics_bench.py measures on the GPU; none is present (nothing is recorded)")
    B = a.batch

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    lines = ["tools/metrics_bench.py (MI355X).", ""] + metrics_cases.report() + [
        "", "ms per call at batch %d, fp32 NCHW, images and reference of one size; hd = the library call (hd_image_metrics: two launches;" % B,
        "hd_image_range: one), torch = the same formula from torch ops on the same GPU in fp32.  Device events around back-to-back calls,",
        "%d alternating rounds, median (min .. max).  floor = 24 B per pixel position (range: 12 B) at 8.0 TB/s over the hd time." % max(3, a.rounds),
        "max|hd - torch| (SSIM per face; range: both ends) is taken before timing.", "",
        "%-8s %5s  %-26s  %-26s  %8s  %7s  %s" % ("call", "px", "hd ms", "torch ms", "torch/hd", "floor", "max|hd - torch|")]
    g = torch.Generator(device="cuda").manual_seed(22)
    lost = []
    for R in [int(v) for v in a.sizes.split(",")]:
        ref = torch.rand((B, 3, R, R), device="cuda", generator=g)
        img = (ref + 0.05 * torch.randn((B, 3, R, R), device="cuda", generator=g)).clamp(0, 1)
        for call in ("y", "rgb", "range"):
            if call == "range":
                hfn = lambda: metrics.image_range(img)                 # noqa: E731
                tfn = lambda: metrics.range_reference(img)             # noqa: E731
                diff = float((hfn() - tfn()).abs().max())
                floor_b = 12.0
            else:
                hfn = lambda: metrics.image_metrics(img, ref, channels=call)             # noqa: E731
                tfn = lambda: metrics.image_metrics_reference(img, ref, channels=call)   # noqa: E731
                diff = float((hfn().ssim - tfn().ssim.double()).abs().max())
                floor_b = 24.0
            if not diff <= 1e-4:
                raise SystemExit("%s at %d px: the library and the torch composition differ by %.3e; nothing is timed" % (call, R, diff))
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
            floor_ms = 1e3 * floor_b * B * R * R / HBM_PEAK
            if not hm < tm:
                lost.append("%s at %d px" % (call, R))
            lines.append("%-8s %5d  %-26s  %-26s  %7.1fx  %6.1f%%  %.2e" % (
                call, R, "%.4f (%.4f .. %.4f)" % (hm, hd[0], hd[-1]), "%.4f (%.4f .. %.4f)" % (tm, th[0], th[-1]), tm / hm, 100 * floor_ms / hm, diff))
        del img, ref
    lines += ["", "hd ms includes the wrapper's allocations (torch's caching allocator: the result, the workspace) and the ctypes calls; both sides run on",
              "torch's current stream.  " + ("The library call is faster than the composition in every row." if not lost else
                                            "The library call does NOT beat the composition for: " + ", ".join(lost) + ".")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
