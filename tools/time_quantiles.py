"""Time TemperedSMC.summary (include/gjx_quantiles.h) on a GPU box next to a torch route to the same outputs, in alternate
turns in the same process:

    python tools/time_quantiles.py [--D 1000] [--G 10 100 1000] [--n 1000000] [--calls 5] [--warmup 1] [--limit 420]

The model is the random-intercept regression of tools/time_group.py: two scalar latents and one grouped latent [G, n], C = 2 + G
columns.  Per G the CHILD process (`--child`, under `--limit` seconds; the parent starts nothing after a child that fails or
runs out of time) prints one JSON line: HIP-event medians of one `summary` call and of the torch route (per-column
torch.sort, the two order statistics gathered and interpolated, mean and var; in chunks of columns of at most 2^26 entries so
that the sort's indices fit), their ratio, and the share the call achieves of the byte floor of three sweeps over 4 C n bytes
at 8 TB/s.
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
ap.add_argument("--D", type=int, default=1000)
ap.add_argument("--G", type=int, nargs="+", default=[10, 100, 1000])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--limit", type=int, default=420)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()

if not args.child:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--D", str(args.D), "--G", *[str(g) for g in args.G], "--n", str(args.n),
           "--calls", str(args.calls), "--warmup", str(args.warmup)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(tool="time_quantiles", error=f"no result within {args.limit} s")), flush=True)
        sys.exit(124)
    if rc != 0:
        print(json.dumps(dict(tool="time_quantiles", error=f"exit status {rc}")), flush=True)
    sys.exit(rc if rc >= 0 else 1)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from genjax import ChoiceMap, Target, gen, normal  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402
from genjax.inference.smc import TemperedSMC  # noqa: E402

PROBS = (0.05, 0.5, 0.95)


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


def torch_route(cols, probs):
    """The same outputs through torch, a chunk of columns at a time: -> (quantiles [C, Q], mean [C], var [C]), float64."""
    n = cols[0].shape[-1]
    p = torch.tensor(probs, dtype=torch.float64, device=cols[0].device)
    h = (n - 1) * p
    lo = h.floor().long()
    hi = (lo + 1).clamp(max=n - 1)
    rows = max(1, (1 << 26) // n)
    out = []
    for c in cols:
        c = c.reshape(-1, n)
        for r0 in range(0, c.shape[0], rows):
            blk = c[r0:r0 + rows]
            s = torch.sort(blk, dim=1).values
            xl, xh = s[:, lo].double(), s[:, hi].double()
            d = blk.double()
            out.append((xl + (h - lo) * (xh - xl), d.mean(dim=1), d.var(dim=1)))
    return tuple(torch.cat(t) for t in zip(*out))


def model_of(G):
    @gen
    def intercepts(xs, g):
        mu = normal(0.0, 2.0) @ "mu"
        b = normal(0.0, 2.0) @ "b"
        a = normal(mu, 0.7).repeat(n=G) @ "a"
        normal(a[g] + b * xs, 0.5) @ "y"

    return intercepts


D, n = args.D, args.n
rng = np.random.default_rng(0)
xs = np.linspace(2.0, 3.0, D).astype(np.float32)
ops = load_hip_ops()
with use_ops(ops):
    dev = ops.device()
    for G in args.G:
        g = np.sort(np.arange(D) % G).astype(np.int64)
        ys = (0.4 + 0.6 * xs + 0.5 * rng.standard_normal(D)).astype(np.float32)
        alg = TemperedSMC(Target(model_of(G), (torch.from_numpy(xs), torch.from_numpy(g)), ChoiceMap.d({"y": torch.from_numpy(ys)})), n)
        cols = [(0.4 + 0.05 * torch.randn(n, device=dev)).contiguous(), (0.6 + 0.05 * torch.randn(n, device=dev)).contiguous(),
                (0.4 + 0.05 * torch.randn(G, n, device=dev)).contiguous()]
        got, (q, mean, var) = alg.summary(cols, PROBS), torch_route(cols, PROBS)
        mine = torch.cat([got.quantiles[a].reshape(-1, len(PROBS)) for a in ("mu", "b", "a")])
        err = float((mine - q).abs().max())  # (the two routes agree: last bits of the interpolation)
        hip_ms, torch_ms = alternate(lambda: alg.summary(cols, PROBS), lambda: torch_route(cols, PROBS), args.calls, args.warmup)
        floor_ms = 3 * 4.0 * (2 + G) * n / 8e12 * 1e3
        print(json.dumps(dict(tool="time_quantiles", G=G, n=n, columns=2 + G, calls=args.calls, summary_ms=hip_ms, torch_ms=torch_ms,
                              torch_over_summary=torch_ms / hip_ms, byte_floor_ms=floor_ms, share_of_byte_floor=floor_ms / hip_ms,
                              max_abs_quantile_difference=err)), flush=True)
        del cols, got, q, mean, var, mine
