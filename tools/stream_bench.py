"""Continuous batching against static batching: batch 64, latent 16, synthetic weights (writes profiles/r08_stream_bench.txt, or --out).

Scenarios (requests all queued at t = 0; each request has its own seed and img2img strength):
  (a) 512 requests at strength 1.0, DDIM-50;   (b) 512 requests with strengths uniform in [0.2, 1.0], DDIM-50;   (c) (b) with DPM-Solver++ 2M, 20 steps.
Forms: static batching -- 64 requests at a time through sample(start_steps=...), the batch runs until its slowest face is done -- and
sampling.ContinuousSampler at refill_every K = 1, 5, 10.  Each configuration is timed end to end (queue to last result, device
synchronised), in alternating runs; reported: median and spread of faces/s, and the mean request latency (finish time - 0).
Also: hd_prepare_slots for n = 1, 8, 32, 64 against hd_prepare at 64, hd_sample_faces ms/step against hd_sample_rows, and where the time
of a continuous run goes (refills against sampling calls; an instrumented run with a synchronisation around each part).
--mixed-steps 10,20,50 runs one scenario instead (and appends to --out): the requests cycle through DDIM schedules of these step counts,
strengths uniform in [0.2, 1.0]; one ContinuousSampler over a sampling.ScheduleSet (hd_sample_spans: all step counts share the 64 slots)
against one ContinuousSampler per step count, run one after the other, shortest schedule first (what a single-schedule batch allows).
--prefetch P measures the conditioning pool instead (writes profiles/r15_pool_bench.txt, or --out): scenarios (a), (b), (c) at K = 1, 5, 10
with ContinuousSampler(prefetch=0) and (prefetch=P), and with --parent DIR (a checkout of the parent commit with its library built) the
parent's sampler in a second process, all in alternating runs: faces/s median [min, max] and the instrumented refill share of each; then
hd_pool_prepare and hd_pool_commit for n = 1, 8, 64 next to hd_prepare_slots.
    python tools/stream_bench.py --prefetch 64 [--parent DIR] [--runs 3]"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sync():
    torch.cuda.synchronize()


def requests(n, mixed, seed=8):
    from hifidiff_amd import synth
    _, crl, crf = synth.sample_inputs(64, 16, seed=seed)
    g = torch.Generator().manual_seed(seed)
    strength = (0.2 + 0.8 * torch.rand(n, generator=g)).tolist() if mixed else [1.0] * n
    # 64 distinct conditioning inputs, reused round robin (their content does not change the cost)
    return [(crf[i % 64].cuda(), crl[i % 64].cuda(), 1000 + i, strength[i]) for i in range(n)]


def run_static(m, sch, reqs):
    from hifidiff_amd import sampling
    sync()
    t0 = time.perf_counter()
    lat = []
    probe = sampling.ContinuousSampler(m, sch, batch=64)                  # only for the per-request initial latents (CPU generator)
    for b in range(0, len(reqs), 64):
        chunk = reqs[b:b + 64]
        starts = [probe._start(crl, seed, st) for _, crl, seed, st in chunk]
        x = torch.stack([s[0] for s in starts]).cuda()
        rows = torch.tensor([s[1] for s in starts])
        crf = torch.stack([r[0] for r in chunk])
        crl = torch.stack([r[1] for r in chunk])
        sampling.sample(m, x, crf, crl, sch, start_steps=rows, seed=chunk[0][2])      # hd_sample_rows*
        lat += [time.perf_counter() - t0] * len(chunk)                    # sample() synchronises (check=True)
    return time.perf_counter() - t0, statistics.mean(lat)


def run_continuous(m, sch, reqs, K, instrument=False, prefetch=0):
    from hifidiff_amd import sampling
    cs = sampling.ContinuousSampler(m, sch, batch=64, refill_every=K, **({"prefetch": prefetch} if prefetch else {}))
    t_refill = [0.0]
    if instrument:
        inner = cs._refill

        def timed_refill(dev):
            sync()
            t = time.perf_counter()
            inner(dev)
            sync()
            t_refill[0] += time.perf_counter() - t
        cs._refill = timed_refill
    sync()
    t0 = time.perf_counter()
    for r in reqs:
        cs.submit(*r)
    lat = []
    while cs.busy():
        cs.step()                                                         # sample() synchronises after each call
        done = cs.poll()
        lat += [time.perf_counter() - t0] * len(done)
    total = time.perf_counter() - t0
    return total, statistics.mean(lat), t_refill[0], cs.calls


def run_set(m, sset, reqs, keys, K):
    """One ContinuousSampler over the set: every request on its own member."""
    from hifidiff_amd import sampling
    cs = sampling.ContinuousSampler(m, sset, batch=64, refill_every=K)
    sync()
    t0 = time.perf_counter()
    for r, k in zip(reqs, keys):
        cs.submit(*r, schedule=k)
    lat = []
    while cs.busy():
        cs.step()
        lat += [time.perf_counter() - t0] * len(cs.poll())
    return time.perf_counter() - t0, statistics.mean(lat)


def run_one_by_one(m, sset, reqs, keys, K):
    """One ContinuousSampler per member, one after the other (shortest schedule first); latencies count from the common t = 0."""
    from hifidiff_amd import sampling
    sync()
    t0 = time.perf_counter()
    lat = []
    for key in sorted(sset.keys):
        cs = sampling.ContinuousSampler(m, sset.member(key), batch=64, refill_every=K)
        for r, k in zip(reqs, keys):
            if k == key:
                cs.submit(*r)
        while cs.busy():
            cs.step()
            lat += [time.perf_counter() - t0] * len(cs.poll())
    return time.perf_counter() - t0, statistics.mean(lat)


def mixed_steps(m, a):
    from hifidiff_amd import sampling, schedulers
    counts = [int(v) for v in a.mixed_steps.split(",")]
    members = {}
    for n in counts:
        members[n] = schedulers.DDIMScheduler(clip_sample_range=3.0)
        members[n].set_timesteps(n)
    sset = sampling.ScheduleSet(members)
    reqs = requests(a.requests, True)
    keys = [counts[i % len(counts)] for i in range(len(reqs))]
    n = len(reqs)
    out = [f"\n# tools/stream_bench.py --mixed-steps {a.mixed_steps}: {n} requests queued at t = 0, DDIM, step counts cycling over the requests, "
           f"strength U[0.2, 1.0], batch 64, latent 16; {a.runs} alternating runs (median [min, max])",
           "form                              faces/s median [min, max]        mean latency s   vs one by one"]
    forms = [(f"{name} K={K}", fn, K) for K in (5, 10) for name, fn in (("one sampler per count", run_one_by_one), ("one sampler, set", run_set))]
    for _, fn, K in forms:                                                # warm: captures, FiLM tables, staging chain
        fn(m, sset, reqs[:96], keys[:96], K)
    res = {f: [] for f, _, _ in forms}
    for _ in range(a.runs):
        for f, fn, K in forms:
            res[f].append(fn(m, sset, reqs, keys, K))
    for f, _, K in forms:
        base = statistics.median(n / t for t, _ in res[f"one sampler per count K={K}"])
        fps = [n / t for t, _ in res[f]]
        lat = statistics.median(l for _, l in res[f])
        out.append(f"{f:<33} {statistics.median(fps):8.1f} [{min(fps):7.1f}, {max(fps):7.1f}]   {lat:10.3f}      {statistics.median(fps) / base:5.2f}x")
    txt = "\n".join(out) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(txt)


def scenarios():
    from hifidiff_amd import schedulers

    def ddim():
        s = schedulers.DDIMScheduler(clip_sample_range=3.0)
        s.set_timesteps(50)
        return s

    def dpm():
        s = schedulers.DPMSolverMultistepScheduler()
        s.set_timesteps(20)
        return s
    return [("a", "512 requests, strength 1.0, DDIM-50", ddim, False), ("b", "512 requests, strength U[0.2, 1.0], DDIM-50", ddim, True),
            ("c", "512 requests, strength U[0.2, 1.0], DPM-Solver++ 2M 20 steps", dpm, True)]


def t_ms(fn, reps=10):
    fn()
    sync()
    v = []
    for _ in range(reps):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        v.append((time.perf_counter() - t) * 1e3)
    return statistics.median(v), min(v), max(v)


def worker(root, n_req):
    """--prefetch: one process per tree (this one, the parent's).  Commands on stdin: `run <scenario> <K> <prefetch> <instrument>` ->
    `<seconds> <mean latency> <refill seconds> <calls>`; `cond` -> the pool call timings, one line each, then `end`."""
    sys.path.insert(0, root)
    from hifidiff_amd import synth
    from hifidiff_amd.refiner import FacialRefiner
    torch.set_grad_enabled(False)
    m = FacialRefiner(16)
    m.load_state_dict(synth.refiner_state_dict(16))
    m.to("cuda:0")
    scen = {key: (mk(), requests(n_req, mixed)) for key, _, mk, mixed in scenarios()}
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if cmd[0] == "quit":
            break
        if cmd[0] == "run":
            sch, reqs = scen[cmd[1]]
            total, lat, t_ref, calls = run_continuous(m, sch, reqs, int(cmd[2]), instrument=cmd[4] == "1", prefetch=int(cmd[3]))
            if int(cmd[3]):
                m.disable_pool()
            print(f"{total:.6f} {lat:.6f} {t_ref:.6f} {calls}", flush=True)
        elif cmd[0] == "cond":
            _, crl, crf = synth.sample_inputs(64, 16)
            crl, crf = crl.cuda(), crf.cuda()
            e = m.engine
            e.prepare(crl, cr_face=crf)
            e.enable_pool(64)
            for nn in (1, 8, 64):
                idx = list(range(0, 64, 64 // nn))[:nn]
                for name, fn in (("hd_prepare_slots", lambda: e.prepare_slots(idx, crl[:nn], cr_face=crf[:nn])),
                                 ("hd_pool_prepare ", lambda: e.pool_prepare(idx, crl[:nn], cr_face=crf[:nn])),
                                 ("hd_pool_commit  ", lambda: e.pool_commit(idx, idx))):
                    t = t_ms(fn)
                    print(f"{name}  n = {nn:2d}: {t[0]:7.3f} [{t[1]:.3f}, {t[2]:.3f}]", flush=True)
            e.disable_pool()
            print("end", flush=True)


class Child:
    def __init__(self, root, n_req):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, "--requests", str(n_req)],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        line = self.p.stdout.readline()
        while line and not line.startswith("ready"):
            line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("the worker of %s ended before it was ready" % root)

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("the worker ended")
        return line.rstrip("\n")

    def run(self, key, K, prefetch, instrument=False):
        v = self.ask(f"run {key} {K} {prefetch} {int(instrument)}").split()
        return float(v[0]), float(v[1]), float(v[2]), int(v[3])

    def close(self):
        self.p.stdin.write("quit\n")
        self.p.stdin.flush()
        self.p.wait()


def pool_bench(a):
    P, n = a.prefetch, a.requests
    this = Child(ROOT, n)
    parent = Child(os.path.abspath(a.parent), n) if a.parent else None
    forms = ([("parent", parent, 0)] if parent else []) + [("prefetch 0", this, 0), (f"prefetch {P}", this, P)]
    out = [f"# tools/stream_bench.py --prefetch {P}: batch 64, latent 16, synthetic weights, one MI355X; {n} requests queued at t = 0; "
           f"{a.runs} alternating runs per configuration (median [min, max]); parent: the parent commit's build in a process of its own"
           + ("" if parent else " (not run: no --parent)")]
    for key, title, _, _ in scenarios():
        out.append(f"\n({key}) {title}")
        out.append("form                         faces/s median [min, max]        mean latency s   vs " + forms[0][0] + "   instrumented: refills of the run")
        for K in (1, 5, 10):
            for _, ch, pf in forms:                                        # warm: captures, FiLM table, staging chain, pool
                ch.run(key, K, pf)
            res = {f: [] for f, _, _ in forms}
            for _ in range(a.runs):
                for f, ch, pf in forms:
                    res[f].append(ch.run(key, K, pf))
            base = statistics.median(n / r[0] for r in res[forms[0][0]])
            for f, ch, pf in forms:
                fps = [n / r[0] for r in res[f]]
                lat = statistics.median(r[1] for r in res[f])
                total, _, t_ref, calls = ch.run(key, K, pf, instrument=True)
                out.append(f"K={K:<2d} {f:<22} {statistics.median(fps):8.1f} [{min(fps):7.1f}, {max(fps):7.1f}]   {lat:10.3f}      "
                           f"{statistics.median(fps) / base:5.2f}x      {t_ref:.3f} of {total:.3f} s ({100 * t_ref / total:.1f} %), {calls} calls")
            print("\n".join(out[-len(forms):]), flush=True)
    out.append("\nconditioning calls (ms, host-timed with synchronisation, median [min, max] of 10)")
    this.p.stdin.write("cond\n")
    this.p.stdin.flush()
    for line in iter(this.p.stdout.readline, ""):
        if line.startswith("end"):
            break
        out.append(line.rstrip("\n"))
    this.close()
    if parent:
        parent.close()
    txt = "\n".join(out) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--requests", type=int, default=512)
    ap.add_argument("--out", default=None, help="default: profiles/r08_stream_bench.txt (--prefetch: profiles/r15_pool_bench.txt)")
    ap.add_argument("--mixed-steps", help="comma-separated step counts: run the mixed-schedule scenario only, appended to --out")
    ap.add_argument("--prefetch", type=int, default=0, metavar="P", help="measure the conditioning pool: prefetch 0 and P (and --parent) at K = 1, 5, 10")
    ap.add_argument("--parent", help="--prefetch: checkout of the parent commit (library built): its sampler is alternated with this tree's")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.requests)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r15_pool_bench.txt" if a.prefetch else "r08_stream_bench.txt")
    if a.prefetch:
        return pool_bench(a)
    from hifidiff_amd import _lib, synth
    from hifidiff_amd.refiner import FacialRefiner
    torch.set_grad_enabled(False)
    m = FacialRefiner(16)
    m.load_state_dict(synth.refiner_state_dict(16))
    m.to("cuda:0")
    if a.mixed_steps:
        return mixed_steps(m, a)
    L = _lib.lib()
    out = ["# tools/stream_bench.py: batch 64, latent 16, synthetic weights, one MI355X; requests queued at t = 0; "
           f"{a.runs} alternating runs per configuration (median [min, max])"]

    scen = scenarios()
    ddim = scen[0][2]
    forms = ["static"] + [f"continuous K={k}" for k in (1, 5, 10)]
    for key, title, mk, mixed in scen:
        reqs = requests(a.requests, mixed)
        sch = mk()
        n = len(reqs)

        def one(form):
            if form == "static":
                return run_static(m, sch, reqs)
            return run_continuous(m, sch, reqs, int(form.split("=")[1]))[:2]
        for f in forms:                                                   # warm: captures, FiLM table, staging chain
            one(f) if f == "static" else run_continuous(m, sch, reqs[:96], int(f.split("=")[1]))
        res = {f: [] for f in forms}
        for _ in range(a.runs):
            for f in forms:
                res[f].append(one(f))
        out.append(f"\n({key}) {title}")
        out.append("form                 faces/s median [min, max]        mean latency s   vs static")
        base = statistics.median(n / t for t, _ in res["static"])
        for f in forms:
            fps = [n / t for t, _ in res[f]]
            lat = statistics.median(l for _, l in res[f])
            out.append(f"{f:<20} {statistics.median(fps):8.1f} [{min(fps):7.1f}, {max(fps):7.1f}]   {lat:10.3f}      "
                       f"{statistics.median(fps) / base:5.2f}x")
        for k in (1, 5, 10):
            total, _, t_ref, calls = run_continuous(m, sch, reqs, k, instrument=True)
            out.append(f"  instrumented continuous K={k}: {total:.3f} s, of which refills {t_ref:.3f} s ({100 * t_ref / total:.1f} %), "
                       f"{calls} sampling calls")
        print("\n".join(out[-(len(forms) + 5):]), flush=True)

    # hd_prepare_slots against hd_prepare
    _, crl, crf = synth.sample_inputs(64, 16)
    crl, crf = crl.cuda(), crf.cuda()
    m.engine.prepare(crl, cr_face=crf)

    out.append("\nconditioning (ms, host-timed with synchronisation, median [min, max] of 10)")
    t = t_ms(lambda: m.engine.prepare(crl, cr_face=crf))
    out.append(f"hd_prepare        B = 64: {t[0]:7.3f} [{t[1]:.3f}, {t[2]:.3f}]")
    for nn in (1, 8, 32, 64):
        sl = list(range(0, 64, 64 // nn))[:nn]
        t = t_ms(lambda: m.engine.prepare_slots(sl, crl[:nn], cr_face=crf[:nn]))
        out.append(f"hd_prepare_slots  n = {nn:2d}: {t[0]:7.3f} [{t[1]:.3f}, {t[2]:.3f}]")

    # hd_sample_faces against hd_sample_rows (DDIM-50, start rows spread over the schedule, as tools/rows_bench.py)
    s = ddim()
    ts, coef = [u.float().contiguous() for u in s.coefficient_table()]
    sc = _lib.Schedule()
    sc.n_steps = 50
    sc.timesteps = ctypes.cast(ts.data_ptr(), ctypes.POINTER(ctypes.c_float))
    sc.coef = ctypes.cast(coef.data_ptr(), ctypes.POINTER(ctypes.c_float))
    rows = torch.tensor([f * 49 // 63 for f in range(64)], dtype=torch.int32)
    rp = ctypes.cast(rows.data_ptr(), ctypes.POINTER(ctypes.c_int32))
    seeds = (ctypes.c_uint64 * 64)(*range(64))
    xd = synth.sample_inputs(64, 16)[0].cuda().contiguous()
    ctx, stream = m.engine.ctx, torch.cuda.current_stream().cuda_stream
    fns = {"hd_sample_rows": lambda: L.hd_sample_rows(ctx, xd.data_ptr(), ctypes.byref(sc), rp, 50, None, 0, stream),
           "hd_sample_faces": lambda: L.hd_sample_faces(ctx, xd.data_ptr(), ctypes.byref(sc), rp, 50, seeds, None, 0, stream)}
    res = {k: [] for k in fns}
    for f in fns.values():
        _lib.check(f(), ctx)
    for _ in range(5):
        for k, f in fns.items():
            sync()
            t = time.perf_counter()
            _lib.check(f(), ctx)
            sync()
            res[k].append((time.perf_counter() - t) * 1e3 / 50)
    _lib.check(L.hd_check(ctx), ctx)
    out.append("\nms per step, DDIM-50, start rows f * 49 // 63, median [min, max] of 5 alternating runs")
    for k, v in res.items():
        out.append(f"{k:<16} {statistics.median(v):.3f} [{min(v):.3f}, {max(v):.3f}]")
    txt = "\n".join(out) + "\n"
    print(txt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(txt)


if __name__ == "__main__":
    main()
