"""Time gjx_plate_loglik (include/gjx_plate_loglik.h) against its two baselines on a GPU box:

    python tools/time_plate_loglik.py [philox|threefry] [--D 1000 100000] [--n 4096 65536 1000000] [--calls 15] [--warmup 3] [--limit 240]

The model is the regression y_d ~ N(w x_d + b, 0.1) as ONE plated site over D rows.  Each (D, n) runs in a CHILD process of
its own (`--child D n`) under `--limit` seconds; the parent stops at the first child that fails or runs out of time and starts
nothing after it.  Per (D, n) the child prints one JSON line with the HIP-event times (median, quartiles) of three calls on
the same plan, data and prior draws, taken in ALTERNATION — round r times each of them once — so that a drift of the box
falls on all three:

  * `split`:     ops.plate_loglik at the library's rows per chunk (two launches);
  * `one_chunk`: the same call with rows_per_chunk >= D (C = 1: the move kernel's split of the work, two launches);
  * `recompute`: ops.temper_move(n_moves = 0, recompute = 1), the one launch that computed ll before this header existed.

All three include their output allocation.  A figure from another box is none: the pool's boxes differ by 3-8 %."""
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
ap.add_argument("--D", nargs="+", type=int, default=[1000, 100_000])
ap.add_argument("--n", nargs="+", type=int, default=[4096, 65_536, 1_000_000])
ap.add_argument("--calls", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--child", nargs=2, type=int, default=None)
args = ap.parse_args()

if args.child is None:
    for D in args.D:
        for n in args.n:
            cmd = [sys.executable, os.path.abspath(__file__), args.impl, "--child", str(D), str(n), "--calls", str(args.calls),
                   "--warmup", str(args.warmup)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(tool="time_plate_loglik", D=D, n=n, error=f"no result within {args.limit} s")), flush=True)
                sys.exit(124)
            if rc != 0:
                print(json.dumps(dict(tool="time_plate_loglik", D=D, n=n, error=f"exit status {rc}")), flush=True)
                sys.exit(rc if rc > 0 else 1)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax import ChoiceMap, Target, gen, normal  # noqa: E402
from genjax._amd import temper  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402


@gen
def plated(xs, s):
    w = normal(0.0, 2.0) @ "w"
    b = normal(0.0, 2.0) @ "b"
    normal(w * xs + b, s) @ "y"


D, n = args.child
rng = np.random.default_rng(0)
xs = np.linspace(-1.0, 1.0, D).astype(np.float32)
ys = (0.7 * xs - 0.3 + 0.1 * rng.standard_normal(D)).astype(np.float32)
ops = load_hip_ops()
with use_ops(ops):
    key = genjax.random.key(2, args.impl)
    dev = ops.device()
    x = [(2.0 * torch.randn(n, device=dev)).contiguous() for _ in range(2)]  # prior draws
    tr = temper.lower(Target(plated, (torch.from_numpy(xs), 0.1), ChoiceMap.d({"y": torch.from_numpy(ys)})), n)
    plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
    plan.set_params(tr.params)
    plan.set_data(tr.data_columns(dev))
    one = (D + 3) // 4 * 4
    calls = dict(split=lambda: ops.plate_loglik(plan, x, impl=key.impl),
                 one_chunk=lambda: ops.plate_loglik(plan, x, impl=key.impl, rows_per_chunk=one),
                 recompute=lambda: ops.temper_move(plan, key, x, None, None, 0.0, 0, None, recompute=True, want_accept=False))
    for _ in range(args.warmup):  # (the first round compiles)
        outs = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["split"][0].isnan(), outs["recompute"][2].isnan())
                and torch.equal(outs["one_chunk"][0].nan_to_num(), outs["recompute"][2].nan_to_num()))
    ms = {k: [] for k in calls}
    for _ in range(args.calls):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = dict(tool="time_plate_loglik", impl=args.impl, D=D, n=n, calls=args.calls, one_chunk_equals_recompute=same,
               chunks=int(ops.lib.call("gjx_plate_loglik_chunks", n, D, 0)))
    for k, v in ms.items():
        v.sort()
        out[k] = dict(median_ms=statistics.median(v), q1_ms=v[len(v) // 4], q3_ms=v[(3 * len(v)) // 4])
    out["split_over_one_chunk"] = out["split"]["median_ms"] / out["one_chunk"]["median_ms"]
    out["split_over_recompute"] = out["split"]["median_ms"] / out["recompute"]["median_ms"]
    print(json.dumps(out), flush=True)
