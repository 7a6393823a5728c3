"""Time the tempered SMC sampler (genjax.inference.smc.TemperedSMC -> gjx_temper_move, gjx_temper_ess_ladder) on a GPU box:

    python tools/time_temper.py [philox|threefry] [--model regression gauss10] [--n 1000000] [--K 2] [--calls 9] [--warmup 2]
                                [--limit 240]

Each model runs in a CHILD process of its own (`--child MODEL`) under `--limit` seconds; the parent stops at the first child
that fails or runs out of time and starts nothing after it.  Per model (the README's regression with m = 20 points and noise
0.1; a 10-latent Gaussian with ten observations) the child prints one JSON line per measurement:

  * `run`: wall time of whole `TemperedSMC.run` calls (host reads included), stages, time per stage;
  * `move`: HIP-event times of the move launch alone (ops.temper_move: K sweeps through a permuted ancestors column, the
    output allocation included) -> median, ns per particle-sweep, and the bytes the launch must move, (L + 2) * 8 + 4 per
    particle, as a fraction of what 8 TB/s would carry in that time;
  * `move_K0`: the same launch with K = 0, recompute = 1 (the stage-0 fill: load, assess, store);
  * `ladder`: one gjx_temper_ess_ladder launch over 32 temperatures;
  * `resample`: one gjx_resample_systematic call over the stage's log-weights;
  * `scales`: the float64 weighted-deviation proposal scales on the device, read back;
  * `share`: the move launch's share of a stage (move / (run per stage)).
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
            print(json.dumps(dict(tool="time_temper", model=model, error=f"no result within {args.limit} s")), flush=True)
            sys.exit(124)
        if rc != 0:
            print(json.dumps(dict(tool="time_temper", model=model, error=f"exit status {rc}")), flush=True)
            sys.exit(rc if rc > 0 else 1)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax import ChoiceMap, Target, gen, normal  # noqa: E402
from genjax._amd import temper  # noqa: E402
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
    alg = TemperedSMC(make(args.child), n, n_moves=K)
    key = genjax.random.key(1, args.impl)
    res = alg.run(key)  # (compiles)
    base = dict(tool="time_temper", impl=args.impl, model=args.child, n=n, K=K)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = alg.run(key)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    stages = len(res.betas) - 1
    run_ms = statistics.median(walls)
    print(json.dumps(dict(base, what="run", median_ms=run_ms, stages=stages, ms_per_stage=run_ms / stages, betas=res.betas,
                          accept_rate=res.accept_rate, log_z=res.log_marginal_likelihood)), flush=True)
    st = alg._state()
    plan, L = st["tplan"], len(st["latents"])
    x, lp, ll = res.columns, res.lp, res.ll
    anc = torch.randperm(n, device=lp.device).to(torch.int32)
    lw = (ll * 0.5).contiguous()
    scales = TemperedSMC.population_scales(x, lw).cpu().numpy()
    k2 = genjax.random.key(2, args.impl)
    m = timed(lambda: ops.temper_move(plan, k2, x, lp, ll, 1.0, K, scales, ancestors=anc), args.calls, args.warmup)
    nbytes = ((L + 2) * 8 + 4) * n
    m.update(what="move", L=L, ns_per_particle_sweep=m["median_ms"] * 1e6 / (float(n) * max(K, 1)), bytes=nbytes,
             of_8TBs=nbytes / 8e12 / (m["median_ms"] * 1e-3), share_of_stage=m["median_ms"] / (run_ms / stages))
    print(json.dumps(dict(base, **m)), flush=True)
    m0 = timed(lambda: ops.temper_move(plan, k2, x, None, None, 0.0, 0, None, recompute=True, want_accept=False), args.calls, args.warmup)
    print(json.dumps(dict(base, what="move_K0", **m0)), flush=True)
    ws = ops.temper_ladder_workspace(n)
    deltas = temper.ladder_deltas(0.0)
    out = ops.empty(2 * len(deltas) + 1, torch.float64)
    ld = timed(lambda: ops.temper_ess_ladder(ll, deltas, ws, out), args.calls, args.warmup)
    print(json.dumps(dict(base, what="ladder", G=len(deltas), **ld)), flush=True)
    rs = timed(lambda: ops.resample("systematic", k2.literal(), lw), args.calls, args.warmup)
    print(json.dumps(dict(base, what="resample", **rs)), flush=True)
    sc = timed(lambda: TemperedSMC.population_scales(x, lw).cpu(), args.calls, args.warmup)
    print(json.dumps(dict(base, what="scales", **sc)), flush=True)
