"""Time the move launch of a PLATED tempered plan (include/gjx_plate.h) on a GPU box:

    python tools/time_plate.py [philox|threefry] [--D 20 1000 10000] [--n 1000000] [--K 2] [--calls 9] [--warmup 2] [--limit 240]

The model is the regression y_d ~ N(w x_d + b, 0.1) as ONE plated site over D rows.  Each D runs in a CHILD process of its
own (`--child D`) under `--limit` seconds; the parent stops at the first child that fails or runs out of time and starts
nothing after it.  Per D the child prints one JSON line:

  * `move`: HIP-event times of ops.temper_move alone (K sweeps through a permuted ancestors column from prior draws, the
    output allocation included) -> median, quartiles, and ps per (particle, datum, sweep);
  * at D = 20 also `move_unrolled`: the SAME data as the unrolled plan (twenty observed sites, every number a launch
    parameter), timed in the same process on the same box — the baseline of the plated form.  A figure from another box is
    none: the pool's boxes differ by 3-8 %.
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
ap.add_argument("--D", nargs="+", type=int, default=[20, 1000, 10000])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--K", type=int, default=2)
ap.add_argument("--calls", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--child", type=int, default=None)
args = ap.parse_args()

if args.child is None:
    for D in args.D:
        cmd = [sys.executable, os.path.abspath(__file__), args.impl, "--child", str(D), "--n", str(args.n), "--K", str(args.K),
               "--calls", str(args.calls), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(tool="time_plate", D=D, error=f"no result within {args.limit} s")), flush=True)
            sys.exit(124)
        if rc != 0:
            print(json.dumps(dict(tool="time_plate", D=D, error=f"exit status {rc}")), flush=True)
            sys.exit(rc if rc > 0 else 1)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax import ChoiceMap, Target, gen, normal  # noqa: E402
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
def plated(xs, s):
    w = normal(0.0, 2.0) @ "w"
    b = normal(0.0, 2.0) @ "b"
    normal(w * xs + b, s) @ "y"


@gen
def unrolled(xs, s):
    w = normal(0.0, 2.0) @ "w"
    b = normal(0.0, 2.0) @ "b"
    for i, x in enumerate(xs):
        normal(w * x + b, s) @ ("y", i)


D, n, K = args.child, args.n, args.K
rng = np.random.default_rng(0)
xs = np.linspace(-1.0, 1.0, D).astype(np.float32)
ys = (0.7 * xs - 0.3 + 0.1 * rng.standard_normal(D)).astype(np.float32)
ops = load_hip_ops()
with use_ops(ops):
    key = genjax.random.key(2, args.impl)
    dev = ops.device()
    x = [(2.0 * torch.randn(n, device=dev)).contiguous() for _ in range(2)]  # prior draws
    anc = torch.randperm(n, device=dev).to(torch.int32)
    scales = np.array([0.05, 0.05], dtype=np.float32)
    targets = [("move", Target(plated, (torch.from_numpy(xs), 0.1), ChoiceMap.d({"y": torch.from_numpy(ys)})))]
    if D == 20:
        targets.append(("move_unrolled", Target(unrolled, ([float(v) for v in xs], 0.1),
                                                ChoiceMap.d({("y", i): float(v) for i, v in enumerate(ys)}))))
    for what, target in targets:
        tr = temper.lower(target, n)
        plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
        plan.set_params(tr.params)
        if tr.data:
            plan.set_data([t.to(device=dev, dtype=torch.float32).contiguous() for t in tr.data])
        _, lp, ll, _ = ops.temper_move(plan, key, x, None, None, 0.0, 0, None, recompute=True, want_accept=False)  # (compiles)
        m = timed(lambda: ops.temper_move(plan, key, x, lp, ll, 1.0, K, scales, ancestors=anc), args.calls, args.warmup)
        m.update(tool="time_plate", impl=args.impl, what=what, D=D, n=n, K=K, sites=len(tr.sites), params=len(tr.params),
                 ps_per_particle_datum_sweep=m["median_ms"] * 1e9 / (float(n) * D * max(K, 1)))
        print(json.dumps(m), flush=True)
