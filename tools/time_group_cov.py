"""Time the per-group moments launch and the block move of include/gjx_group_cov.h on a GPU box, each next to the route it
stands beside, in alternate turns in the same process:

    python tools/time_group_cov.py [philox|threefry] [--D 1000] [--G 10 100 1000] [--S 1 2] [--n 1000000] [--K 2] [--calls 5] [--warmup 1] [--limit 420]

S = 1 is the random-intercept regression of tools/time_group.py, S = 2 adds a random slope c_g ~ N(b, 0.5).  Per (S, G) the
CHILD process (`--child`, under `--limit` seconds; the parent starts nothing after a child that fails or runs out of time)
prints one JSON line: HIP-event medians of gjx_group_moments next to TemperedSMC.group_scales (the share of 4 S G n bytes at
8 TB/s the launch achieves), and of gjx_temper_move_grouped_cov at the DIAGONAL factor next to gjx_temper_move_grouped with
the same scales.
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
ap.add_argument("--S", type=int, nargs="+", default=[1, 2], choices=[1, 2])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--K", type=int, default=2)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--limit", type=int, default=420)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()

if not args.child:
    cmd = [sys.executable, os.path.abspath(__file__), args.impl, "--child", "--D", str(args.D), "--G", *[str(g) for g in args.G], "--S",
           *[str(s) for s in args.S], "--n", str(args.n), "--K", str(args.K), "--calls", str(args.calls), "--warmup", str(args.warmup)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(tool="time_group_cov", error=f"no result within {args.limit} s")), flush=True)
        sys.exit(124)
    if rc != 0:
        print(json.dumps(dict(tool="time_group_cov", error=f"exit status {rc}")), flush=True)
    sys.exit(rc if rc >= 0 else 1)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax import ChoiceMap, Target, gen, normal  # noqa: E402
from genjax._amd import temper  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402
from genjax.inference.smc import TemperedSMC  # noqa: E402


def alternate(fa, fb, calls, warmup):
    """Median HIP-event ms of fa and fb, called in alternate turns."""
    ms = ([], [])
    for turn in range(warmup + calls):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if turn >= warmup:
                ms[k].append(a.elapsed_time(b))
    return statistics.median(ms[0]), statistics.median(ms[1])


def model_of(G, S):
    @gen
    def intercepts(xs, g):
        mu = normal(0.0, 2.0) @ "mu"
        b = normal(0.0, 2.0) @ "b"
        a = normal(mu, 0.7).repeat(n=G) @ "a"
        normal(a[g] + b * xs, 0.5) @ "y"

    @gen
    def slopes(xs, g):
        mu = normal(0.0, 2.0) @ "mu"
        b = normal(0.0, 2.0) @ "b"
        a = normal(mu, 0.7).repeat(n=G) @ "a"
        c = normal(b, 0.5).repeat(n=G) @ "c"
        normal(a[g] + c[g] * xs, 0.5) @ "y"

    return intercepts if S == 1 else slopes


D, n, K = args.D, args.n, args.K
rng = np.random.default_rng(0)
xs = np.linspace(2.0, 3.0, D).astype(np.float32)
ops = load_hip_ops()
with use_ops(ops):
    key = genjax.random.key(2, args.impl)
    dev = ops.device()
    anc = torch.randperm(n, device=dev).to(torch.int32)
    lw = (-torch.rand(n, device=dev) * 4.0).contiguous()
    scales = np.array([0.01, 0.01], dtype=np.float32)
    for S in args.S:
        for G in args.G:
            g = np.sort(np.arange(D) % G).astype(np.int64)
            ys = (0.4 + 0.6 * xs + 0.5 * rng.standard_normal(D)).astype(np.float32)
            tr = temper.lower(Target(model_of(G, S), (torch.from_numpy(xs), torch.from_numpy(g)), ChoiceMap.d({"y": torch.from_numpy(ys)})), n)
            plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
            plan.set_data(tr.data_columns(dev))
            plan.set_groups(tr.group_offsets().to(dev))
            x = [(c + 0.05 * torch.randn(n, device=dev)).contiguous() for c in (0.4, 0.6)]
            z = [(c + 0.05 * torch.randn(G, n, device=dev)).contiguous() for c in (0.4, 0.6)[:S]]
            ws = ops.temper_group_moments_workspace(n, G, S)
            mom_ms, torch_ms = alternate(lambda: ops.temper_group_moments(z, lw, ws), lambda: TemperedSMC.group_scales(z, lw), args.calls, args.warmup)
            zsc = torch.full((S, G), 0.05, dtype=torch.float32, device=dev)
            fz = torch.zeros(G, S * (S + 1) // 2, dtype=torch.float32, device=dev)
            for s in range(S):
                fz[:, s * (s + 1) // 2 + s] = 0.05
            _, _, lp, ll, _, _ = ops.temper_move_grouped(plan, key, x, z, None, None, 0.0, 0, recompute=True, want_accept=False)  # (compiles)
            ops.temper_move_grouped_cov(plan, key, x, z, lp, ll, 1.0, 0, None, want_accept=False)  # (compiles)
            block_ms, diag_ms = alternate(lambda: ops.temper_move_grouped_cov(plan, key, x, z, lp, ll, 1.0, K, fz, None, scales, ancestors=anc),
                                          lambda: ops.temper_move_grouped(plan, key, x, z, lp, ll, 1.0, K, scales, zsc, ancestors=anc),
                                          args.calls, args.warmup)
            print(json.dumps(dict(tool="time_group_cov", impl=args.impl, S=S, G=G, D=D, n=n, K=K, calls=args.calls, moments_ms=mom_ms,
                                  group_scales_torch_ms=torch_ms, share_of_8_TBps=4.0 * S * G * n / (mom_ms * 1e-3) / 8e12,
                                  block_move_ms=block_ms, grouped_move_ms=diag_ms, block_over_grouped=block_ms / diag_ms)), flush=True)
            del plan, lp, ll, z, ws
