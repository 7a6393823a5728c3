"""Time the generated kernels of a plated COUNT site (include/gjx_counts.h) on a GPU box, next to the Normal regression of
tools/time_plate.py on the same box in the same process:

    python tools/time_counts.py [philox|threefry] [--D 1000] [--n 1000000] [--K 2] [--calls 5] [--warmup 1] [--limit 420]

The models are y_d ~ Poisson(exp(w x_d + b)) and y_d ~ N(w x_d + b, 0.1), each ONE plated site over D rows.  The work runs in
a CHILD process (`--child`) under `--limit` seconds; the parent starts nothing after a child that fails or runs out of time.
Per model and call the child prints one JSON line of HIP-event times (median, quartiles): `move` (ops.temper_move, K sweeps
through a permuted ancestors column), `pointwise` (ops.temper_pointwise), `loo` (ops.temper_psis at the package's tail length)
and `predictive` (ops.temper_predictive, no draws kept), with ps per (particle, datum) — per sweep for the move.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("impl", nargs="?", default="philox", choices=["philox", "threefry"])
ap.add_argument("--D", type=int, default=1000)
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--K", type=int, default=2)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--limit", type=int, default=420)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()

if not args.child:
    cmd = [sys.executable, os.path.abspath(__file__), args.impl, "--child", "--D", str(args.D), "--n", str(args.n), "--K", str(args.K),
           "--calls", str(args.calls), "--warmup", str(args.warmup)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(tool="time_counts", error=f"no result within {args.limit} s")), flush=True)
        sys.exit(124)
    if rc != 0:
        print(json.dumps(dict(tool="time_counts", error=f"exit status {rc}")), flush=True)
    sys.exit(rc if rc >= 0 else 1)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax import ChoiceMap, Target, gen, normal, poisson  # noqa: E402
from genjax._amd import temper  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402


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


@gen
def poisson_regression(xs):
    w = normal(0.0, 2.0) @ "w"
    b = normal(0.0, 2.0) @ "b"
    poisson(log_rate=w * xs + b) @ "y"


@gen
def normal_regression(xs, s):
    w = normal(0.0, 2.0) @ "w"
    b = normal(0.0, 2.0) @ "b"
    normal(w * xs + b, s) @ "y"


D, n, K = args.D, args.n, args.K
rng = np.random.default_rng(0)
xs = np.linspace(-1.0, 1.0, D).astype(np.float32)
counts = rng.poisson(np.exp(0.7 * xs + 1.0)).astype(np.float32)
ys = (0.7 * xs - 0.3 + 0.1 * rng.standard_normal(D)).astype(np.float32)
ops = load_hip_ops()
with use_ops(ops):
    key = genjax.random.key(2, args.impl)
    dev = ops.device()
    anc = torch.randperm(n, device=dev).to(torch.int32)
    scales = np.array([0.01, 0.01], dtype=np.float32)
    M = int(ops.lib.call("gjx_psis_tail_len", n, 1.0))
    cases = [("poisson", Target(poisson_regression, (torch.from_numpy(xs),), ChoiceMap.d({"y": torch.from_numpy(counts)})), (0.7, 1.0)),
             ("normal", Target(normal_regression, (torch.from_numpy(xs), 0.1), ChoiceMap.d({"y": torch.from_numpy(ys)})), (0.7, -0.3))]
    for model, target, centre in cases:
        # a population around the posterior (a tenth of a unit wide): rates, densities and tails of ordinary size
        x = [(c + 0.1 * torch.randn(n, device=dev)).contiguous() for c in centre]
        tr = temper.lower(target, n)
        plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
        if tr.params:
            plan.set_params(tr.params)
        plan.set_data(tr.data_columns(dev))
        _, lp, ll, _ = ops.temper_move(plan, key, x, None, None, 0.0, 0, None, recompute=True, want_accept=False)  # (compiles)
        calls = {
            "move": (lambda: ops.temper_move(plan, key, x, lp, ll, 1.0, K, scales, ancestors=anc), max(K, 1)),
            "pointwise": (lambda: ops.temper_pointwise(plan, x), 1),
            "loo": (lambda: ops.temper_psis(plan, x, M), 1),
            "predictive": (lambda: ops.temper_predictive(plan, key, x, 0), 1),
        }
        for what, (fn, per) in calls.items():
            fn()  # (compiles)
            m = timed(fn, args.calls, args.warmup)
            m.update(tool="time_counts", impl=args.impl, model=model, what=what, D=D, n=n, K=K, tail_len=M,
                     ps_per_particle_datum=m["median_ms"] * 1e9 / (float(n) * D * per))
            print(json.dumps(m), flush=True)
