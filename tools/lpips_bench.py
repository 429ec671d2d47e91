#!/usr/bin/env python3
"""What hd_lpips costs, and how exact it is.  First the measured errors against `metrics.lpips_reference` in float64 with their bf16
emulation yardsticks (tools/lpips_cases.py, the figures tests/test_lpips.py asserts on).  Then ms per call at batch 64 and 128 / 256 /
512 px against the same formula composed from torch ops on the same GPU in fp32 (metrics.lpips_reference: ten convolutions, four
max-pools and the distance, about 80 ops for the pair).  The composition is the comparison, not the code under test; the two results
are compared before anything is timed.  Device events around `reps` back-to-back calls, after a warm-up of every shape; library and
torch windows alternate over `rounds` rounds in one process and the median is reported with the spread.  Last, the distance kernel on
its own: the program timed with and without its last two launches (hd_debug_limit_ops), and the difference against the kernel's floor,
the bytes of the ten feature maps (bf16, read once) at the HBM peak of 8.0 TB/s.
    python tools/lpips_bench.py [--batch 64] [--rounds 5] [--out profiles/r23_lpips.txt]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_lpips.txt"))
    a = ap.parse_args()
    import torch
    from hifidiff_amd import _lib, arch, metrics
    import lpips_cases
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        raise SystemExit("tools/lpips_bench.py measures on the GPU; none is present (nothing is recorded)")
    B, rounds = a.batch, max(3, a.rounds)

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def median(fn, reps):
        v = sorted(window(fn, reps) for _ in range(rounds))
        return v[len(v) // 2], v[0], v[-1]

    lines = ["tools/lpips_bench.py (MI355X).  Synthetic weights (synth.lpips_state_dict): the scores are not comparable to published LPIPS.", ""]
    lines += lpips_cases.report()
    print("\n".join(lines), flush=True)
    model, L = lpips_cases.model(), _lib.lib()
    state = {k: v.cuda() for k, v in lpips_cases.state().items()}
    head = ["", "ms per call at batch %d, fp32 NCHW, images and reference of one size, inputs in [0, 1]; hd = the library call (ten launches)," % B,
            "torch = the same formula from torch ops on the same GPU in fp32.  Device events around back-to-back calls, %d alternating rounds," % rounds,
            "median (min .. max).  max|hd - torch| over the faces is taken before timing (bf16 storage against fp32).", "",
            "%5s  %-26s  %-26s  %8s  %s" % ("px", "hd ms", "torch ms", "torch/hd", "max|hd - torch|  (mean score)")]
    tail = ["", "the distance kernel alone: the program with and without its last two launches (distance + combine), median of %d rounds each;" % rounds,
            "floor = the bytes of the ten feature maps (2 B x sum_k 2 P_k C_k per face pair) at 8.0 TB/s.", "",
            "%5s  %-12s  %-12s  %-12s  %-10s  %s" % ("px", "all ms", "convs ms", "distance ms", "floor ms", "floor / distance")]
    print("\n".join(head), flush=True)
    g = torch.Generator(device="cuda").manual_seed(23)
    lost = []
    for R in [int(v) for v in a.sizes.split(",")]:
        ref = torch.rand((B, 3, R, R), device="cuda", generator=g)
        img = (ref + 0.05 * torch.randn((B, 3, R, R), device="cuda", generator=g)).clamp(0, 1)
        hfn = lambda: model(img, ref)                                  # noqa: E731
        tfn = lambda: metrics.lpips_reference(state, img, ref)         # noqa: E731
        h, t = hfn(), tfn()
        diff, mean = float((h - t.double()).abs().max()), float(h.mean())
        if not diff <= 0.05 * mean:
            raise SystemExit("%d px: the library and the torch composition differ by %.3e at a mean score of %.3e; nothing is timed" % (R, diff, mean))
        for _ in range(3):                                             # warm-up of this shape, both sides
            hfn(); tfn()
        torch.cuda.synchronize()
        hreps = max(5, min(100, int(250.0 / max(window(hfn, 3), 1e-3)) + 1))            # windows of about a quarter second
        treps = max(3, min(50, int(250.0 / max(window(tfn, 2), 1e-3)) + 1))
        hd, th = [], []
        for _ in range(rounds):
            hd.append(window(hfn, hreps)); th.append(window(tfn, treps))
        hd.sort(); th.sort()
        hm, tm = hd[len(hd) // 2], th[len(th) // 2]
        if not hm < tm:
            lost.append("%d px" % R)
        head.append("%5d  %-26s  %-26s  %7.1fx  %.2e  (%.3e)" % (R, "%.4f (%.4f .. %.4f)" % (hm, hd[0], hd[-1]), "%.4f (%.4f .. %.4f)" % (tm, th[0], th[-1]),
                                                                  tm / hm, diff, mean))
        print(head[-1], flush=True)
        n_ops = L.hd_num_ops(model._ctx, 0)
        try:
            _lib.check(L.hd_debug_limit_ops(model._ctx, 0, n_ops - 2), model._ctx)
            convs = median(hfn, hreps)[0]
        finally:
            L.hd_debug_limit_ops(model._ctx, 0, -1)
        full = median(hfn, hreps)[0]
        s = arch.lpips_sides(R)
        fbytes = 2.0 * B * sum(2 * p * c for p, c in zip((s[0] ** 2, s[1] ** 2, s[2] ** 2, s[2] ** 2, s[2] ** 2), (64, 192, 384, 256, 256)))
        floor_ms, dist = 1e3 * fbytes / HBM_PEAK, full - convs
        tail.append("%5d  %-12.4f  %-12.4f  %-12.4f  %-10.5f  %s" % (R, full, convs, dist, floor_ms, "%.1f%%" % (100 * floor_ms / dist) if dist > 0 else "n/a"))
        print(tail[-1], flush=True)
        del img, ref
    lines += head + tail
    lines += ["", "hd ms includes the wrapper's allocations (torch's caching allocator), two ctypes calls and the rebuild of the launch program for the new",
              "output pointers; both sides run on torch's current stream.  " + ("The library call is faster than the composition in every row." if not lost else
                                                                                "The library call does NOT beat the composition for: " + ", ".join(lost) + ".")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))
    print("written:", a.out)


if __name__ == "__main__":
    main()
