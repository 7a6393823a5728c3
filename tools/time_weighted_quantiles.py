"""Time Ops.weighted_column_quantiles (include/gjx_quantiles.h, GJX_QUANTILES_WEIGHTED) on a GPU box next to the unweighted
call on the same columns and next to a torch route to the same quantiles, the three in alternate turns in the same process:

    python tools/time_weighted_quantiles.py [--T 100] [--G 10 100 1000] [--n 1000000] [--calls 15] [--warmup 2] [--limit 420]

Cases: "history" — one carry component's filtering history, T columns against T weight columns (V = T), what
SMCResult.summary calls; "paths" — G columns against one weight vector (V = 1), what Trajectories.summary calls.  Columns
are `0.4 + 0.05 randn` (concentrated, as filter populations are), log-weights `randn`.  Per case the CHILD process
(`--child`, under `--limit` seconds; the parent starts nothing after a child that fails or runs out of time) prints one
JSON line: HIP-event medians of the weighted call, of gjx_column_quantiles, and of the torch route (per row torch.sort, the
cumulative sum of the sorted softmax weights, searchsorted; chunks of at most 2^26 entries), and their ratios.
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
ap.add_argument("--T", type=int, default=100)
ap.add_argument("--G", type=int, nargs="*", default=[10, 100, 1000])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--calls", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--limit", type=int, default=420)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()

if not args.child:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--T", str(args.T), "--G", *[str(g) for g in args.G], "--n", str(args.n),
           "--calls", str(args.calls), "--warmup", str(args.warmup)]
    try:
        rc = subprocess.run(cmd, timeout=args.limit).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps(dict(tool="time_weighted_quantiles", error=f"no result within {args.limit} s")), flush=True)
        sys.exit(124)
    if rc != 0:
        print(json.dumps(dict(tool="time_weighted_quantiles", error=f"exit status {rc}")), flush=True)
    sys.exit(rc if rc >= 0 else 1)

import torch  # noqa: E402

from genjax._amd.runtime import load_hip_ops  # noqa: E402

PROBS = (0.05, 0.5, 0.95)


def alternate(fns, calls, warmup):
    """Median HIP-event ms of each of fns, called in alternate turns."""
    ms = [[] for _ in fns]
    for turn in range(warmup + calls):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if turn >= warmup:
                ms[k].append(a.elapsed_time(b))
    return [statistics.median(m) for m in ms]


def torch_route(x, lw, probs):
    """The inverted-CDF quantiles through torch: x [C, n], lw [V, n] (row c % V) -> [C, Q] (float weights: close, not exact)."""
    C, n = x.shape
    p = torch.tensor(probs, dtype=torch.float64, device=x.device)
    rows = max(1, (1 << 26) // n)
    out = []
    for r0 in range(0, C, rows):
        blk = x[r0:r0 + rows]
        w = torch.softmax(lw[torch.arange(r0, r0 + blk.shape[0], device=x.device) % lw.shape[0]].double(), dim=1)
        s, order = torch.sort(blk, dim=1)
        cum = torch.cumsum(torch.gather(w, 1, order), dim=1)
        at = torch.searchsorted(cum, (p * cum[:, -1:]).contiguous()).clamp(max=n - 1)
        out.append(torch.gather(s, 1, at))
    return torch.cat(out)


ops = load_hip_ops()
dev, n = ops.device(), args.n
for case, C, V in [("history", args.T, args.T)] + [("paths", G, 1) for G in args.G]:
    x = (0.4 + 0.05 * torch.randn(C, n, device=dev)).contiguous()
    lw = torch.randn(V, n, device=dev).contiguous()
    quant, _ = ops.weighted_column_quantiles([x], lw, PROBS)
    frac = float((quant != torch_route(x, lw, PROBS)).double().mean())  # (float cumulative sums: a neighbour now and then)
    w_ms, u_ms, t_ms = alternate([lambda: ops.weighted_column_quantiles([x], lw, PROBS), lambda: ops.column_quantiles([x], PROBS),
                                  lambda: torch_route(x, lw, PROBS)], args.calls, args.warmup)
    print(json.dumps(dict(tool="time_weighted_quantiles", case=case, columns=C, weight_columns=V, n=n, calls=args.calls, weighted_ms=w_ms,
                          unweighted_ms=u_ms, torch_ms=t_ms, weighted_over_unweighted=w_ms / u_ms, torch_over_weighted=t_ms / w_ms,
                          quantiles_differing_from_torch=frac)), flush=True)
    del x, lw, quant
