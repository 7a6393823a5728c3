"""Time the generated move kernel of a plan with GROUPED latents (include/gjx_group.h) on a GPU box, next to the flat plated
regression of the same D on the same box in the same process:

    python tools/time_group.py [philox|threefry] [--D 1000] [--G 10 100 1000] [--n 1000000] [--K 2] [--calls 5] [--warmup 1] [--limit 420]

The grouped model is the random-intercept regression mu, b ~ N(0, 2), a_g ~ N(mu, 0.7), y_d ~ N(a[g_d] + b x_d, 0.5) over D
rows in G groups of equal size; the flat one y_d ~ N(w x_d + b, 0.5), ONE plated site over the same D rows.  The work runs in a
CHILD process (`--child`) under `--limit` seconds; the parent starts nothing after a child that fails or runs out of time.
Per model the child prints one JSON line of HIP-event times (median, quartiles) of one move call (K sweeps through a
permuted ancestors column), with ps per (particle, datum, sweep) and, for the grouped plans, the time left per (particle,
group, sweep) after three row-term evaluations at the flat plan's price — the expectation from the code is three row terms
per (particle, row, sweep) plus two per-lane cipher calls per (particle, group, sweep).
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
ap.add_argument("--K", type=int, default=2)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--limit", type=int, default=420)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()

if not args.child:
    cmd = [sys.executable, os.path.abspath(__file__), args.impl, "--child", "--D", str(args.D), "--G", *[str(g) for g in args.G], "--n", str(args.n),
           "--K", str(args.K), "--calls", str(args.calls), "--warmup", str(args.warmup)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(tool="time_group", error=f"no result within {args.limit} s")), flush=True)
        sys.exit(124)
    if rc != 0:
        print(json.dumps(dict(tool="time_group", error=f"exit status {rc}")), flush=True)
    sys.exit(rc if rc >= 0 else 1)

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


D, n, K = args.D, args.n, args.K
rng = np.random.default_rng(0)
xs = np.linspace(-1.0, 1.0, D).astype(np.float32)
ops = load_hip_ops()
with use_ops(ops):
    key = genjax.random.key(2, args.impl)
    dev = ops.device()
    anc = torch.randperm(n, device=dev).to(torch.int32)
    scales = np.array([0.01, 0.01], dtype=np.float32)
    # the flat plan first: its time per (particle, datum, sweep) is ONE row term
    ys = (0.6 * xs + 0.4 + 0.5 * rng.standard_normal(D)).astype(np.float32)
    tr = temper.lower(Target(flat_regression, (torch.from_numpy(xs),), ChoiceMap.d({"y": torch.from_numpy(ys)})), n)
    plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
    plan.set_data(tr.data_columns(dev))
    x = [(c + 0.05 * torch.randn(n, device=dev)).contiguous() for c in (0.6, 0.4)]
    _, lp, ll, _ = ops.temper_move(plan, key, x, None, None, 0.0, 0, None, recompute=True, want_accept=False)  # (compiles)
    m = timed(lambda: ops.temper_move(plan, key, x, lp, ll, 1.0, K, scales, ancestors=anc), args.calls, args.warmup)
    flat_ps = m["median_ms"] * 1e9 / (float(n) * D * max(K, 1))
    m.update(tool="time_group", impl=args.impl, model="flat", D=D, n=n, K=K, ps_per_particle_datum_sweep=flat_ps)
    print(json.dumps(m), flush=True)
    del plan, lp, ll
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
        zsc = torch.full((1, G), 0.05, dtype=torch.float32, device=dev)
        _, _, lp, ll, _, _ = ops.temper_move_grouped(plan, key, x, z, None, None, 0.0, 0, recompute=True, want_accept=False)  # (compiles)
        m = timed(lambda: ops.temper_move_grouped(plan, key, x, z, lp, ll, 1.0, K, scales, zsc, ancestors=anc), args.calls, args.warmup)
        per_sweep_ps = m["median_ms"] * 1e9 / (float(n) * max(K, 1))  # per (particle, sweep)
        m.update(tool="time_group", impl=args.impl, model="grouped", D=D, G=G, n=n, K=K,
                 ps_per_particle_datum_sweep=per_sweep_ps / D, row_terms_at_the_flat_price=per_sweep_ps / D / flat_ps,
                 ps_per_particle_group_sweep_beyond_three_row_terms=(per_sweep_ps - 3.0 * D * flat_ps) / G)
        print(json.dumps(m), flush=True)
        del plan, lp, ll, z
