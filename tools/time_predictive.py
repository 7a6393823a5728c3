#!/usr/bin/env python3
"""Times gjx_temper_predictive (Ops.temper_predictive) next to the same quantities computed in chunked eager torch.

The model is the plated Normal regression of tests/plate_ref.py (y_d ~ N(w x_d + b, s)); populations of n particles, data of
D rows: D = 64 / 1000 / 10 000 at n = 1e6 by default.  The torch side restates the likelihood by hand, draws with torch's own
generator (other numbers: only the work is compared) and walks the particle axis in chunks so that its [chunk, D] temporaries
stay near 256 MB: per chunk one randn, the location, the value, its float64 sum and sum of squares, the count below the
observed value and the count equal to it.

Call times are device-event times around `--reps` calls after `--warmup` warm-up calls (the first call compiles); a GPU is
required — there is no fallback.  One line of JSON per (D, generator) goes to stdout; profiles/predictive_summary.md records
a run."""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "genjax-chi_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def torch_predictive(w, b, xs, ys, s, chunk):
    """The five per-row summaries in eager torch, float64 accumulators, the particle axis in chunks of `chunk`."""
    D = xs.numel()
    s1 = torch.zeros(D, dtype=torch.float64, device=xs.device)
    s2, below, equal = torch.zeros_like(s1), torch.zeros_like(s1), torch.zeros_like(s1)
    for lo in range(0, w.numel(), chunk):
        wc, bc = w[lo:lo + chunk, None], b[lo:lo + chunk, None]
        y = (wc * xs[None, :] + bc) + s * torch.randn(wc.shape[0], D, device=xs.device)
        yd = y.double()
        s1 += yd.sum(dim=0)
        s2 += (yd * yd).sum(dim=0)
        below += (y < ys[None, :]).sum(dim=0)
        equal += (y == ys[None, :]).sum(dim=0)
    return s1, s2, below, equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10 ** 6)
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1000, 10000])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-temp-mb", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_predictive: no GPU — nothing is measured without one")

    import genjax
    import plate_ref as P
    from genjax._amd import temper
    from genjax._amd.runtime import load_hip_ops, use_ops

    ops = load_hip_ops()
    rng = np.random.default_rng(0)
    n = args.n
    cols = [torch.from_numpy((c + 0.1 * rng.standard_normal(n)).astype(np.float32)).cuda() for c in (0.7, -0.3)]
    for D in args.rows:
        with use_ops(ops):
            target, data = P.target("normal", D, seed=1)
            tracer = temper.lower(target, 64)
            plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
        plan.set_params(tracer.params)
        dev = [t.to(torch.float32).cuda() for t in data]
        plan.set_data(dev)
        chunk = max(1, (args.torch_temp_mb << 20) // (4 * D))
        t_torch = event_ms(lambda: torch_predictive(cols[0], cols[1], dev[0], dev[1], 0.1, chunk), 1, max(1, args.reps // 2))
        for impl in ("philox", "threefry"):
            key = genjax.random.key(1, impl)
            t_sum = event_ms(lambda: ops.temper_predictive(plan, key, cols, 0), args.warmup, args.reps)
            t_64 = event_ms(lambda: ops.temper_predictive(plan, key, cols, -(-n // 64)), args.warmup, args.reps)
            print(json.dumps(dict(n=n, rows=D, generator=impl, chunks=int(ops.lib.call("gjx_predictive_chunks", n, D)),
                                  predictive_ms=round(t_sum, 3), predictive_64_draws_ms=round(t_64, 3), torch_chunked_ms=round(t_torch, 3),
                                  torch_chunk=chunk, draws_per_s=round(n * D / (t_sum * 1e-3), 0))), flush=True)


if __name__ == "__main__":
    main()
