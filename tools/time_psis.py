#!/usr/bin/env python3
"""Times gjx_temper_psis (Ops.temper_psis) next to gjx_temper_pointwise on the same plan and next to the selection and the body
sum computed in chunked eager torch.

The models are the plated Normal regression and the logistic regression of tests/plate_ref.py; populations of n particles
around the values the data was generated from, data of D rows: D = 64 / 1000 / 10 000 at n = 1e6 by default.  The torch side
restates the likelihood by hand and walks the ROW axis in chunks so that its [chunk, n] temporaries stay near 256 MB: per chunk
the table, one `topk` of tail_len + 1 per row and the sum of exp(tT - t) over the row.  It leaves the fit out (the GPU call
includes it), and is timed on at most `--torch-rows` rows: its time per row does not depend on D.

Call times are device-event times around `--reps` calls after `--warmup` warm-up calls (the first call compiles); a GPU is
required — there is no fallback.  One line of JSON per (model, D) goes to stdout; profiles/psis_summary.md records a run."""

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


def torch_terms(name, cols, data, lo, hi):
    """t[d, i] of rows lo .. hi in eager torch, f32 [hi - lo, n]."""
    if name == "normal":
        xs, ys = data
        r = (ys[lo:hi, None] - (cols[0][None, :] * xs[lo:hi, None] + cols[1][None, :])) / 0.1
        return -0.5 * r * r - (0.5 * np.log(2 * np.pi) + np.log(0.1))
    x1, x2, ys = data
    z = cols[0][None, :] * x1[lo:hi, None] + cols[1][None, :] * x2[lo:hi, None] + cols[2][None, :]
    return -torch.nn.functional.softplus(torch.where(ys[lo:hi, None] > 0.5, -z, z))


def torch_select(name, cols, data, rows, M, chunk):
    """The tail (topk) and the body sum per row, the row axis in chunks of `chunk`."""
    tails, body = [], []
    for lo in range(0, rows, chunk):
        t = torch_terms(name, cols, data, lo, min(lo + chunk, rows))
        tail = -torch.topk(-t, M + 1, dim=1).values
        tails.append(tail)
        body.append(torch.exp(tail[:, M:] - t).double().sum(dim=1))
    return torch.cat(tails), torch.cat(body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10 ** 6)
    ap.add_argument("--rows", type=int, nargs="+", default=[64, 1000, 10000])
    ap.add_argument("--models", nargs="+", default=["normal", "logistic"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-temp-mb", type=int, default=256)
    ap.add_argument("--torch-rows", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_psis: no GPU — nothing is measured without one")

    import plate_ref as P
    import pointwise_ref as W
    from genjax._amd import temper
    from genjax._amd.runtime import load_hip_ops, use_ops

    ops = load_hip_ops()
    rng = np.random.default_rng(0)
    n = args.n
    M = int(ops.lib.call("gjx_psis_tail_len", n, 1.0))
    for name in args.models:
        cols = [torch.from_numpy(c).cuda() for c in W.centred_columns(name, n, rng)]
        for D in args.rows:
            with use_ops(ops):
                target, data = P.target(name, D, seed=1)
                tracer = temper.lower(target, 64)
                plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            if tracer.params:
                plan.set_params(tracer.params)
            dev = [t.to(torch.float32).cuda() for t in data]
            plan.set_data(dev)
            t_psis = event_ms(lambda: ops.temper_psis(plan, cols, M), args.warmup, args.reps)
            t_tail = event_ms(lambda: ops.temper_psis(plan, cols, M, want_tail=True), 1, args.reps)
            t_pw = event_ms(lambda: ops.temper_pointwise(plan, cols), args.warmup, args.reps)
            rows = min(D, args.torch_rows)
            chunk = max(1, (args.torch_temp_mb << 20) // (4 * n))
            t_torch = event_ms(lambda: torch_select(name, cols, dev, rows, M, chunk), 1, 1)
            out, _ = ops.temper_psis(plan, cols, M)
            khat = out[1].cpu().numpy()
            print(json.dumps(dict(model=name, n=n, rows=D, tail_len=M,
                                  chunks=min(-(-n // 256), max(1, -(-2048 // -(-D // 4)))), psis_ms=round(t_psis, 3),
                                  psis_with_tail_ms=round(t_tail, 3), pointwise_ms=round(t_pw, 3), psis_over_pointwise=round(t_psis / t_pw, 2),
                                  terms_per_s=round(4.0 * n * D / (t_psis * 1e-3), 0), torch_rows=rows, torch_chunk_rows=chunk,
                                  torch_select_ms_per_row=round(t_torch / rows, 3), torch_select_ms_scaled=round(t_torch / rows * D, 1),
                                  khat_min=round(float(np.nanmin(khat)), 3), khat_max=round(float(np.max(khat)), 3))), flush=True)


if __name__ == "__main__":
    main()
