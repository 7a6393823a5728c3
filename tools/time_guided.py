"""Time the guided particle filter next to the bootstrap filter of the same user-written model, whole runs of one filter,
back to back in one process (GPU box):

    python tools/time_guided.py [philox|threefry] [--n 1000000] [--T 100] [--blocks 24] [--runs 3] [--only bootstrap|guided]

The model is the LGSSM (a = 0.9, q = 1) with sharp observations (r = 0.05); the guided filter proposes from the locally
optimal p(x_t | x_{t-1}, y_t).  After a warm-up of both (compilation, code objects, allocator), `--blocks` timed blocks
per filter ALTERNATE between the two; a block is `--runs` whole runs ending in one device synchronise.  Prints the median
and the quartiles of the per-run time and the ratio guided / bootstrap, and one JSON line.  `--only`: one filter alone — under
`rocprofv3 --kernel-trace --stats` / `--pmc` (both filters' step kernels have the same name: one run each), and, as
`--only bootstrap` with GJX_HIP_LIB=<another build of libgjx_hip.so>, how the parent commit's figure is taken on the same
box (a library without include/gjx_guided.h cannot run the guided filter).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax import ChoiceMapBuilder as C, gen, normal  # noqa: E402
from genjax._amd import workloads as W  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402
from genjax._amd.smc_fused import BootstrapSMC, StateSpaceModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("impl", nargs="?", default="philox", choices=["philox", "threefry"])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--T", type=int, default=100)
ap.add_argument("--blocks", type=int, default=24)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--only", choices=["bootstrap", "guided"])
args = ap.parse_args()

A, Q, R = 0.9, 1.0, 0.05
old_r, W.LGSSM["r"] = W.LGSSM["r"], R
y = W.lgssm_data(args.T)
exact = W.lgssm_exact_log_z(y)
W.LGSSM["r"] = old_r


@gen
def init():
    x = normal(0.0, 1.0) @ "x"
    normal(x, R) @ "y"
    return x


@gen
def step(x):
    x2 = normal(A * x, Q) @ "x"
    normal(x2, R) @ "y"
    return x2


s2 = 1.0 / (1.0 / Q ** 2 + 1.0 / R ** 2)
c1, c2, s = s2 * A / Q ** 2, s2 / R ** 2, math.sqrt(s2)
p0 = 1.0 / (1.0 + 1.0 / R ** 2)
k0, s0 = p0 / R ** 2, math.sqrt(p0)


@gen
def track_q(carry, y_t):
    normal(c1 * carry + c2 * y_t, s) @ "x"


@gen
def start_q(y_t):
    normal(k0 * y_t, s0) @ "x"


ops = load_hip_ops()  # raises without a GPU: there is no other way to take these numbers
obs = C["y"].set(torch.tensor(y))
key = genjax.random.key(1, args.impl)
model = StateSpaceModel(init, step)
filters = {}
if args.only != "guided":
    filters["bootstrap"] = BootstrapSMC(model, obs, args.n)
if args.only != "bootstrap":
    from genjax._amd.smc_fused import GuidedSMC

    filters["guided"] = GuidedSMC(model, obs, args.n, step_proposal=track_q, init_proposal=start_q)

with use_ops(ops):
    log_z = {}
    for name, alg in filters.items():  # warm-up: every shape the timed window uses
        for _ in range(3):
            log_z[name] = alg.run(key).log_marginal_likelihood
    torch.cuda.synchronize()
    times = {name: [] for name in filters}
    for _ in range(args.blocks):
        for name, alg in filters.items():
            bound = alg._bind(ops)
            sk, rk = W.smc_key_schedule(key, args.T)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.runs):
                ops._smc_run(bound, key.impl, args.n, sk, rk, False, 0.0)  # (the whole-run call alone: no read-back)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.runs)

out = dict(impl=args.impl, n=args.n, T=args.T, blocks=args.blocks, runs_per_block=args.runs, exact_log_z=exact,
           library=os.environ.get("GJX_HIP_LIB", "this tree's"))
for name, ts in times.items():
    q = statistics.quantiles(ts, n=4)
    med = statistics.median(ts)
    out[name] = dict(ms_per_run=med * 1e3, q1_ms=q[0] * 1e3, q3_ms=q[2] * 1e3, us_per_step=med / args.T * 1e6,
                     particle_steps_per_s=args.n * args.T / med, log_z=log_z[name])
    print(f"{name:10s} {med * 1e3:8.3f} ms per run (quartiles {q[0] * 1e3:.3f} .. {q[2] * 1e3:.3f}) = {med / args.T * 1e6:6.2f} us per step, "
          f"{args.n * args.T / med:.3e} particle-steps/s; log Z {log_z[name]:.4f} (exact {exact:.4f})")
if len(times) == 2:
    out["ratio_guided_over_bootstrap"] = out["guided"]["ms_per_run"] / out["bootstrap"]["ms_per_run"]
    print(f"guided / bootstrap = {out['ratio_guided_over_bootstrap']:.3f}")
print(json.dumps(out))
