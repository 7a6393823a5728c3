"""Time pointwise, loo (the PSIS call) and predictive over a plan with GROUPED latents (include/gjx_group_checks.h) on a GPU
box, next to the flat plated regression of the same D on the same box in the same process:

    python tools/time_group_checks.py [philox|threefry] [--D 1000] [--G 10 100 1000] [--n 1000000] [--calls 15] [--warmup 1] [--limit 540]

The grouped model is the random-intercept regression mu, b ~ N(0, 2), a_g ~ N(mu, 0.7), y_d ~ N(a[g_d] + b x_d, 0.5) over D
rows in G groups of equal size; the flat one y_d ~ N(w x_d + b, 0.5), ONE plated site over the same D rows.  The work runs in a
CHILD process (`--child`) under `--limit` seconds; the parent starts nothing after a child that fails or runs out of time.
Per G and call the child times the flat and the grouped call ALTERNATELY (HIP events around one call each, median and
quartiles) and prints one JSON line with both and their ratio.  The events bracket the whole `Ops` call — its launches and
the allocation of its workspace and outputs from the caching allocator, on both sides alike; `loo` is the PSIS call alone
(nine launches), without the pointwise call `TemperedSMC.loo` adds.  There is no gate: the flat call is the yardstick.  The extra
traffic of the grouped call is the [G, n] column: every (row, particle) term reads one more f32 — from a line the lanes of a
group share (pointwise, predictive: rows on lanes) or from consecutive addresses (PSIS: particles on lanes).
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
ap.add_argument("--G", type=int, nargs="+", default=[10, 100, 1000])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--calls", type=int, default=15)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--limit", type=int, default=540)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()

if not args.child:
    cmd = [sys.executable, os.path.abspath(__file__), args.impl, "--child", "--D", str(args.D), "--G", *[str(g) for g in args.G], "--n", str(args.n),
           "--calls", str(args.calls), "--warmup", str(args.warmup)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(tool="time_group_checks", error=f"no result within {args.limit} s")), flush=True)
        sys.exit(124)
    if rc != 0:
        print(json.dumps(dict(tool="time_group_checks", error=f"exit status {rc}")), flush=True)
    sys.exit(rc if rc >= 0 else 1)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax import ChoiceMap, Target, gen, normal  # noqa: E402
from genjax._amd import temper  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternately(flat, grouped, calls, warmup):
    """-> (flat, grouped) summaries of `calls` timed calls each, taken in turns after `warmup` untimed ones of each."""
    for _ in range(warmup):
        flat()
        grouped()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(calls):
        ms[0].append(once(flat))
        ms[1].append(once(grouped))
    out = []
    for v in ms:
        v.sort()
        out.append(dict(median_ms=statistics.median(v), q1_ms=v[len(v) // 4], q3_ms=v[(3 * len(v)) // 4]))
    return out


@gen
def flat_regression(xs):
    w = normal(0.0, 2.0) @ "w"
    b = normal(0.0, 2.0) @ "b"
    normal(w * xs + b, 0.5) @ "y"


def intercepts(G):
    @gen
    def model(xs, g):
        mu = normal(0.0, 2.0) @ "mu"
        b = normal(0.0, 2.0) @ "b"
        a = normal(mu, 0.7).repeat(n=G) @ "a"
        normal(a[g] + b * xs, 0.5) @ "y"

    return model


D, n = args.D, args.n
rng = np.random.default_rng(0)
xs = np.linspace(-1.0, 1.0, D).astype(np.float32)
ops = load_hip_ops()
with use_ops(ops):
    key = genjax.random.key(2, args.impl)
    dev = ops.device()
    M = int(ops.lib.call("gjx_psis_tail_len", n, 1.0))
    ys = (0.6 * xs + 0.4 + 0.5 * rng.standard_normal(D)).astype(np.float32)
    tr = temper.lower(Target(flat_regression, (torch.from_numpy(xs),), ChoiceMap.d({"y": torch.from_numpy(ys)})), n)
    fplan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
    fplan.set_data(tr.data_columns(dev))
    fx = [(c + 0.05 * torch.randn(n, device=dev)).contiguous() for c in (0.6, 0.4)]
    flat_calls = dict(pointwise=lambda: ops.temper_pointwise(fplan, fx), loo=lambda: ops.temper_psis(fplan, fx, M),
                      predictive=lambda: ops.temper_predictive(fplan, key, fx, 0))
    for G in args.G:
        g = np.sort(np.arange(D) % G).astype(np.int64)  # G groups of D / G rows (the first D % G one longer)
        a_true = 0.4 + 0.7 * rng.standard_normal(G)
        ys = (a_true[g] + 0.6 * xs + 0.5 * rng.standard_normal(D)).astype(np.float32)
        tr = temper.lower(Target(intercepts(G), (torch.from_numpy(xs), torch.from_numpy(g)), ChoiceMap.d({"y": torch.from_numpy(ys)})), n)
        plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
        plan.set_data(tr.data_columns(dev))
        plan.set_groups(tr.group_offsets().to(dev))
        # a population around the posterior (a twentieth of a unit wide)
        x = [(c + 0.05 * torch.randn(n, device=dev)).contiguous() for c in (0.4, 0.6)]
        z = [(torch.from_numpy(a_true.astype(np.float32)).to(dev)[:, None] + 0.05 * torch.randn(G, n, device=dev)).contiguous()]
        calls = dict(pointwise=lambda: ops.temper_pointwise(plan, x, z=z), loo=lambda: ops.temper_psis(plan, x, M, z=z),
                     predictive=lambda: ops.temper_predictive(plan, key, x, 0, z=z))
        for what in ("pointwise", "loo", "predictive"):
            f, gq = alternately(flat_calls[what], calls[what], args.calls, args.warmup)  # (the warm-up compiles)
            print(json.dumps(dict(tool="time_group_checks", impl=args.impl, call=what, D=D, G=G, n=n, tail_len=M, calls=args.calls, flat=f, grouped=gq,
                                  ratio=gq["median_ms"] / f["median_ms"], z_bytes=4 * G * n)), flush=True)
        del plan, z, calls
