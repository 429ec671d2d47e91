"""ms per step of the per-face-row loop (hd_sample_rows) against hd_sample: batch 64, latent 16, DDIM-50 on synthetic weights.

Runs alternate between the forms (median of --runs each): hd_sample; hd_sample_rows with start rows spread over the schedule (every face
evaluated every iteration, faces past their last row held); and both with the persistent stages off ("face" / "xcd" 0: the per-GEMM
program) for contrast.  Writes the table to profiles/r07_rows_bench.txt (or --out)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_rows_bench.txt"))
    a = ap.parse_args()
    from hifidiff_amd import _lib, schedulers, synth
    from hifidiff_amd.refiner import FacialRefiner
    torch.set_grad_enabled(False)
    m = FacialRefiner(16)
    m.load_state_dict(synth.refiner_state_dict(16))
    m.to("cuda:0")
    x, crl, crf = synth.sample_inputs(64, 16)
    m.prepare(crf.cuda(), crl.cuda())
    L, ctx = _lib.lib(), m.engine.ctx
    s = schedulers.DDIMScheduler(clip_sample_range=3.0)
    s.set_timesteps(50)
    ts, coef = [t.float().contiguous() for t in s.coefficient_table()]
    sch = _lib.Schedule()
    sch.n_steps = 50
    sch.timesteps = ctypes.cast(ts.data_ptr(), ctypes.POINTER(ctypes.c_float))
    sch.coef = ctypes.cast(coef.data_ptr(), ctypes.POINTER(ctypes.c_float))
    rows = torch.tensor([f * 49 // 63 for f in range(64)], dtype=torch.int32)
    rp = ctypes.cast(rows.data_ptr(), ctypes.POINTER(ctypes.c_int32))
    xd = x.cuda().contiguous()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(fn(), ctx)
        torch.cuda.synchronize()
        _lib.check(L.hd_check(ctx), ctx)
        return (time.perf_counter() - t0) * 1e3 / 50

    forms = {
        "hd_sample": lambda: L.hd_sample(ctx, xd.data_ptr(), ctypes.byref(sch), None, 0, stream),
        "hd_sample_rows": lambda: L.hd_sample_rows(ctx, xd.data_ptr(), ctypes.byref(sch), rp, 50, None, 0, stream),
    }
    res = {}
    for stages in (1, 0):
        for k in ("face", "xcd"):
            _lib.check(L.hd_set_option(ctx, k.encode(), stages), ctx)
        for f in forms.values():                         # capture + warm
            timed(f)
        t = {k: [] for k in forms}
        for _ in range(a.runs):
            for k, f in forms.items():
                t[k].append(timed(f))
        for k in forms:
            res[(k, stages)] = t[k]
        if stages:
            st = {k: L.hd_get_option(ctx, k.encode()) for k in ("sample_stage_launches", "sample_face_stage_launches", "rows_stage_launches")}
    lines = ["# tools/rows_bench.py: batch 64, latent 16, DDIM-50, synthetic weights; ms per step (whole call / 50), alternating runs",
             f"# hd_sample_rows start rows f * 49 // 63 (f = 0..63), n_iters 50; persistent-stage launches per step: {st}",
             "form                      stages  median   runs"]
    for (k, stages), v in res.items():
        lines.append(f"{k:<25} {'on' if stages else 'off':<6}  {statistics.median(v):7.3f}  " + " ".join(f"{u:.3f}" for u in v))
    on = statistics.median(res[("hd_sample_rows", 1)]) / statistics.median(res[("hd_sample", 1)]) - 1
    off = statistics.median(res[("hd_sample_rows", 0)]) / statistics.median(res[("hd_sample", 1)]) - 1
    lines.append(f"hd_sample_rows vs hd_sample (stages on): {100 * on:+.1f} %;  per-GEMM per-face form vs hd_sample: {100 * off:+.1f} %")
    txt = "\n".join(lines) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)


if __name__ == "__main__":
    main()
