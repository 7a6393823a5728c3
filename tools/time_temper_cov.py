"""Time one stage of the tempered SMC sampler under both proposals (genjax.inference.smc.TemperedSMC: proposal="diagonal" ->
gjx_temper_move with torch's float64 scales read back; proposal="covariance" -> gjx_temper_moments + gjx_temper_move_cov,
include/gjx_temper_cov.h) on a GPU box:

    python tools/time_temper_cov.py [philox|threefry] [--model regression gauss10] [--n 1000000] [--K 2] [--calls 9] [--warmup 2]
                                    [--limit 240]

Each model runs in a CHILD process of its own (`--child MODEL`) under `--limit` seconds; the parent stops at the first child
that fails or runs out of time and starts nothing after it.  Per model (the README's regression with m = 20 points and noise
0.1; a 10-latent Gaussian with ten observations: the models of tools/time_temper.py) the child prints one JSON line per
measurement:

  * `run`: per proposal, wall time of whole `TemperedSMC.run` calls (host reads included), stages, time per stage, the
    acceptance rates;
  * `moments`: HIP-event times of one gjx_temper_moments launch (ops.temper_moments, the output allocation included), and the
    bytes it must move, 4 (L + 1) per particle plus the pass over the weights, as a fraction of what 8 TB/s would carry;
  * `scales`: the float64 weighted-deviation proposal scales in torch, read back (TemperedSMC.population_scales: what the
    diagonal route pays per stage) — wall time, since its cost is a host read;
  * `scales_device`: the same without the read, HIP events;
  * `move` / `move_cov`: HIP-event times of the two move launches (K sweeps through a permuted ancestors column).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("impl", nargs="?", default="philox", choices=["philox", "threefry"])
ap.add_argument("--model", nargs="+", default=["regression", "gauss10"], choices=["regression", "gauss10"])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--K", type=int, default=2)
ap.add_argument("--calls", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--child", default=None)
args = ap.parse_args()

if args.child is None:
    for model in args.model:
        cmd = [sys.executable, os.path.abspath(__file__), args.impl, "--child", model, "--n", str(args.n), "--K", str(args.K),
               "--calls", str(args.calls), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(tool="time_temper_cov", model=model, error=f"no result within {args.limit} s")), flush=True)
            sys.exit(124)
        if rc != 0:
            print(json.dumps(dict(tool="time_temper_cov", model=model, error=f"exit status {rc}")), flush=True)
            sys.exit(rc if rc > 0 else 1)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax import ChoiceMap, Target, gen, normal  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402
from genjax.inference.smc import TemperedSMC  # noqa: E402


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=statistics.median(ms), q1_ms=ms[len(ms) // 4], q3_ms=ms[(3 * len(ms)) // 4], calls=calls)


def walled(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return dict(median_ms=statistics.median(ms), q1_ms=ms[len(ms) // 4], q3_ms=ms[(3 * len(ms)) // 4], calls=calls)


def make(model):
    rng = np.random.default_rng(0)
    if model == "regression":
        @gen
        def regression(xs, s):
            w = normal(0.0, 2.0) @ "w"
            b = normal(0.0, 2.0) @ "b"
            for i, x in enumerate(xs):
                normal(w * x + b, s) @ ("y", i)

        xs = np.linspace(-1.0, 1.0, 20)
        ys = 0.7 * xs - 0.3 + 0.1 * rng.standard_normal(20)
        return Target(regression, ([float(x) for x in xs], 0.1), ChoiceMap.d({("y", i): float(y) for i, y in enumerate(ys)}))

    @gen
    def gauss10():
        zs = [normal(0.0, 1.0) @ f"z{i}" for i in range(10)]
        for i, z in enumerate(zs):
            normal(z, 0.1) @ f"y{i}"

    return Target(gauss10, (), ChoiceMap.d({f"y{i}": float(v) for i, v in enumerate(rng.standard_normal(10))}))


ops = load_hip_ops()
with use_ops(ops):
    n, K = args.n, args.K
    key = genjax.random.key(1, args.impl)
    base = dict(tool="time_temper_cov", impl=args.impl, model=args.child, n=n, K=K)
    algs = {p: TemperedSMC(make(args.child), n, n_moves=K, proposal=p) for p in ("diagonal", "covariance")}
    res = {}
    for p, alg in algs.items():
        res[p] = alg.run(key)  # (compiles)
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[p] = alg.run(key)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        stages = len(res[p].betas) - 1
        run_ms = statistics.median(walls)
        print(json.dumps(dict(base, what="run", proposal=p, median_ms=run_ms, stages=stages, ms_per_stage=run_ms / stages,
                              accept_rate=res[p].accept_rate, log_z=res[p].log_marginal_likelihood,
                              n_degenerate=res[p].n_degenerate)), flush=True)
    st = algs["covariance"]._state()
    plan, L = st["tplan"], len(st["latents"])
    r = res["covariance"]
    x, lp, ll = r.columns, r.lp, r.ll
    anc = torch.randperm(n, device=lp.device).to(torch.int32)
    lw = (ll * 0.5).contiguous()
    ws = ops.temper_moments_workspace(n, L)
    mo = timed(lambda: ops.temper_moments(x, lw, ws), args.calls, args.warmup)
    nbytes = 4 * (L + 2) * n  # every column once, the weights twice (the block maximum, then the tile)
    mo.update(what="moments", L=L, bytes=nbytes, of_8TBs=nbytes / 8e12 / (mo["median_ms"] * 1e-3))
    print(json.dumps(dict(base, **mo)), flush=True)
    sc = walled(lambda: TemperedSMC.population_scales(x, lw).cpu(), args.calls, args.warmup)
    print(json.dumps(dict(base, what="scales", **sc)), flush=True)
    sd = timed(lambda: TemperedSMC.population_scales(x, lw), args.calls, args.warmup)
    print(json.dumps(dict(base, what="scales_device", **sd)), flush=True)
    _, factor, scales_dev, _ = ops.temper_moments(x, lw, ws)
    scales = scales_dev.cpu().numpy()
    k2 = genjax.random.key(2, args.impl)
    for what, fn in (("move", lambda: ops.temper_move(plan, k2, x, lp, ll, 1.0, K, scales, ancestors=anc)),
                     ("move_cov", lambda: ops.temper_move_cov(plan, k2, x, lp, ll, 1.0, K, factor, ancestors=anc))):
        m = timed(fn, args.calls, args.warmup)
        m.update(what=what, L=L, ns_per_particle_sweep=m["median_ms"] * 1e6 / (float(n) * max(K, 1)))
        print(json.dumps(dict(base, **m)), flush=True)
