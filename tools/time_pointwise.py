"""Time the pointwise launch pair over a PLATED tempered plan (include/gjx_pointwise.h) on a GPU box:

    python tools/time_pointwise.py [--models regression logistic] [--D 64 1000 10000] [--n 1000000] [--calls 20] [--warmup 3]
                                   [--limit 300]

Each (model, D) runs in a CHILD process of its own (`--child MODEL D`) under `--limit` seconds; the parent stops at the first
child that fails or runs out of time and starts nothing after it.  Per (model, D) the child prints two JSON lines:

  * `pointwise`: HIP-event times of ops.temper_pointwise (both launches, the workspace and output allocations included) ->
    median, quartiles, and ps per (particle, row);
  * `torch`: the SAME four quantities per row (log-sum-exp, sum, sum of squares, count) written in torch over the latent
    columns, in row chunks of at most 2^26 [rows, n] elements per temporary — what a user has without the call, timed in the
    same process on the same box (the only fair baseline: no earlier version has the call; a figure from another box is
    none), and the largest difference between the two results.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--models", nargs="+", default=["regression", "logistic"], choices=["regression", "logistic"])
ap.add_argument("--D", nargs="+", type=int, default=[64, 1000, 10000])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--child", nargs=2, default=None)
args = ap.parse_args()
if args.calls < 20:
    ap.error("--calls: the median of at least 20 timed calls")

if args.child is None:
    for model in args.models:
        for D in args.D:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", model, str(D), "--n", str(args.n), "--calls", str(args.calls),
                   "--warmup", str(args.warmup)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(tool="time_pointwise", model=model, D=D, error=f"no result within {args.limit} s")), flush=True)
                sys.exit(124)
            if rc != 0:
                print(json.dumps(dict(tool="time_pointwise", model=model, D=D, error=f"exit status {rc}")), flush=True)
                sys.exit(rc if rc > 0 else 1)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from genjax import ChoiceMap, Target, flip, gen, normal  # noqa: E402
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
def regression(xs, s):
    w = normal(0.0, 2.0) @ "w"
    b = normal(0.0, 2.0) @ "b"
    normal(w * xs + b, s) @ "y"


@gen
def logistic(x1, x2):
    w1 = normal(0.0, 2.0) @ "w1"
    w2 = normal(0.0, 2.0) @ "w2"
    b = normal(0.0, 2.0) @ "b"
    flip(torch.sigmoid(w1 * x1 + w2 * x2 + b)) @ "y"


model, D, n = args.child[0], int(args.child[1]), args.n
rng = np.random.default_rng(0)
f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
x1 = rng.uniform(-1.0, 1.0, D)
ops = load_hip_ops()
with use_ops(ops):
    dev = ops.device()
    if model == "regression":
        ys = 0.7 * x1 - 0.3 + 0.1 * rng.standard_normal(D)
        target = Target(regression, (f(x1), 0.1), ChoiceMap.d({"y": f(ys)}))
        x = [(c + 0.02 * torch.randn(n, device=dev)).contiguous() for c in (0.7, -0.3)]  # a posterior-like population
        dx, dy = f(x1).to(dev), f(ys).to(dev)

        def row_terms(lo, hi):  # [rows, n] float32
            z = (dy[lo:hi, None] - (x[0][None, :] * dx[lo:hi, None] + x[1][None, :])) / 0.1
            return -0.5 * z * z - (0.5 * math.log(2 * math.pi) + math.log(0.1))
    else:
        x2 = rng.uniform(-1.0, 1.0, D)
        p = 1.0 / (1.0 + np.exp(-(1.5 * x1 - 1.0 * x2 + 0.2)))
        yb = rng.random(D) < p
        target = Target(logistic, (f(x1), f(x2)), ChoiceMap.d({"y": torch.from_numpy(yb)}))
        x = [(c + 0.1 * torch.randn(n, device=dev)).contiguous() for c in (1.5, -1.0, 0.2)]
        d1, d2, dy = f(x1).to(dev), f(x2).to(dev), torch.from_numpy(yb).to(dev)

        def row_terms(lo, hi):
            z = x[0][None, :] * d1[lo:hi, None] + x[1][None, :] * d2[lo:hi, None] + x[2][None, :]
            return torch.where(dy[lo:hi, None], torch.nn.functional.logsigmoid(z), torch.nn.functional.logsigmoid(-z))

    rows = max(1, (1 << 26) // n)

    def in_torch():
        out = torch.empty((4, D), dtype=torch.float64, device=dev)
        for lo in range(0, D, rows):
            hi = min(D, lo + rows)
            t = row_terms(lo, hi)
            t64 = t.double()
            out[0, lo:hi] = torch.logsumexp(t64, dim=1)
            out[1, lo:hi] = t64.sum(dim=1)
            out[2, lo:hi] = (t64 * t64).sum(dim=1)
            out[3, lo:hi] = (t > -math.inf).sum(dim=1)
        return out

    tr = temper.lower(target, n)
    plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
    if tr.params:
        plan.set_params(tr.params)
    plan.set_data([t.to(device=dev, dtype=torch.float32).contiguous() for t in tr.data])
    got = ops.temper_pointwise(plan, x)  # (compiles)
    common = dict(tool="time_pointwise", model=model, D=D, n=n, chunks=int(ops.lib.call("gjx_pointwise_chunks", n, D)),
                  workspace_mb=int(ops.lib.call("gjx_pointwise_workspace_bytes", n, D)) / 1e6)
    m = timed(lambda: ops.temper_pointwise(plan, x), args.calls, args.warmup)
    m.update(common, what="pointwise", ps_per_particle_row=m["median_ms"] * 1e9 / (float(n) * D))
    print(json.dumps(m), flush=True)
    ref = in_torch()
    b = timed(in_torch, args.calls, args.warmup)
    b.update(common, what="torch", ps_per_particle_row=b["median_ms"] * 1e9 / (float(n) * D), speedup=b["median_ms"] / m["median_ms"],
             max_abs_lse_diff=float((got[0] - ref[0]).abs().max()), max_rel_s1_diff=float(((got[1] - ref[1]) / ref[1]).abs().max()),
             counts_equal=bool(torch.equal(got[3], ref[3])))
    print(json.dumps(b), flush=True)
