#!/usr/bin/env python3
"""Times gjx_temper_psis_units (Ops.temper_psis_units, what TemperedSMC.logo calls) in turns with gjx_temper_psis_grouped
(`loo`) of the same plan, and next to the same quantity in chunked eager torch.

The model is the random-intercept regression of tests/group_ref.py (`intercept`: L = 2 scalars, one grouped latent) over D rows
in U equal groups, the units being the plan's groups: D = 1000 and 10 000, U = 10 / 100 / 1000 at n = 1e6 by default, populations
around the generating values; no draw is made, so the generator does not matter.  The torch side restates the likelihood by
hand: per chunk of units (its [chunk, n] float64 table near `--torch-temp-mb`) the rows' terms are summed into the units'
entries (segment sums: rows are sorted by unit), then one `topk` of tail_len + 1 per unit and the body sum.  It leaves the fit out
and is timed on at most `--torch-units` units.

`logo` and `loo` are timed in TURNS in one process — one call of each per turn, device events around each call — and the
medians over `--reps` turns after `--warmup` turns are reported (the first call compiles); a GPU is required, there is no
fallback.  One line of JSON per (D, U) goes to stdout; profiles/logo_summary.md records a run."""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "genjax-chi_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def call_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def turns_ms(fns, warmup, reps):
    """The median call time of every function, the functions called in turns."""
    times = [[] for _ in fns]
    for r in range(warmup + reps):
        for k, fn in enumerate(fns):
            t = call_ms(fn)
            if r >= warmup:
                times[k].append(t)
    return [float(np.median(t)) for t in times]


def torch_logo(b, a, xs, ys, per, units, M, chunk):
    """Tail and body sum of the first `units` units (`per` rows each) in eager torch, `chunk` units at a time."""
    tails, body = [], []
    for u0 in range(0, units, chunk):
        u1 = min(u0 + chunk, units)
        T = torch.zeros((u1 - u0, b.numel()), dtype=torch.float64, device=b.device)
        for j in range(per):  # (row j of every unit of the chunk: a [chunk, n] block of terms)
            d = torch.arange(u0, u1, device=b.device) * per + j
            r = (ys[d, None] - (a[u0:u1] + b[None, :] * xs[d, None])) / 0.5
            T += (-0.5 * r * r - (0.5 * np.log(2 * np.pi) + np.log(0.5))).double()
        T = T.float()
        tail = -torch.topk(-T, M + 1, dim=1).values
        tails.append(tail)
        body.append(torch.exp(tail[:, M:] - T).double().sum(dim=1))
    return torch.cat(tails), torch.cat(body)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10 ** 6)
    ap.add_argument("--rows", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--units", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-temp-mb", type=int, default=256)
    ap.add_argument("--torch-units", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_logo: no GPU — nothing is measured without one")

    import group_checks_ref as GC
    import group_ref as GR
    from genjax._amd import temper
    from genjax._amd.runtime import load_hip_ops, use_ops

    ops = load_hip_ops()
    n = args.n
    M = int(ops.lib.call("gjx_psis_tail_len", n, 1.0))
    for D in args.rows:
        for U in args.units:
            per = D // U
            sizes = [per] * U
            with use_ops(ops):
                target, _, off = GR.target("intercept", sizes, 0)
                tracer = temper.lower(target, 64)
                plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            if tracer.params:
                plan.set_params(tracer.params)
            dev = [t.to(torch.float32).cuda() for t in tracer.data_columns("cpu")]
            plan.set_data(dev)
            doff = torch.from_numpy(off).cuda()
            plan.set_groups(doff)
            # the population of tests/group_checks_ref.centred_columns, drawn on the device (z is [U, n]: 4 GB at U = 1000)
            xs0, zs0 = GC.generating("intercept", sizes, 0)
            g = torch.Generator(device="cuda").manual_seed(D + U)
            x = [float(c) + 0.1 * torch.randn(n, device="cuda", generator=g) for c in xs0]
            z = [torch.from_numpy(zs0[0].astype(np.float32)).cuda()[:, None] + 0.1 * torch.randn((U, n), device="cuda", generator=g)]
            logo = lambda: ops.temper_psis_units(plan, x, doff, M, z=z)
            loo = lambda: ops.temper_psis(plan, x, M, z=z)
            pw = lambda: ops.temper_pointwise(plan, x, z=z)
            t_logo, t_loo, t_pw = turns_ms([logo, loo, pw], args.warmup, args.reps)
            units = min(U, args.torch_units)
            chunk = max(1, (args.torch_temp_mb << 20) // (8 * n))
            xs_d, ys_d = dev[0], dev[-1]  # (the plan's data columns: the regressor, then the observed value)
            t_torch = float(np.median([call_ms(lambda: torch_logo(x[1], z[0], xs_d, ys_d, per, units, M, chunk)) for _ in range(3)]))
            out, _ = logo()
            khat = out[1].cpu().numpy()
            print(json.dumps(dict(model="intercept", n=n, rows=D, units=U, rows_per_unit=per, tail_len=M, logo_ms=round(t_logo, 3),
                                  loo_ms=round(t_loo, 3), pointwise_ms=round(t_pw, 3), logo_over_loo=round(t_logo / t_loo, 3),
                                  table_mb=round(4.0 * U * n / 2 ** 20, 1), torch_units=units, torch_chunk_units=chunk,
                                  torch_ms_per_unit=round(t_torch / units, 3), torch_ms_scaled=round(t_torch / units * U, 1),
                                  khat_min=round(float(np.nanmin(khat)), 3), khat_max=round(float(np.max(khat)), 3))), flush=True)


if __name__ == "__main__":
    main()
