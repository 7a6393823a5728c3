"""Time the conditional particle filter next to the unconditional record_history run of the same user-written model, through
the stepwise history route, back to back in one process (GPU box):

    python tools/time_csmc.py [philox|threefry] [--n 1000000] [--T 100] [--blocks 12] [--runs 3] [--parent-lib PATH]
    GJX_HIP_LIB=<parent's libgjx_hip.so> python tools/time_csmc.py --only unconditional    # (c) alone, as tools/ab_lib.sh selects a build
    python tools/time_csmc.py --sweeps 200 --n 1024         # time per particle Gibbs sweep instead

Three configurations ALTERNATE over `--blocks` timed blocks (a block is `--runs` whole runs ending in one device
synchronise), after a warm-up of each (compilation, code objects, allocator):

    (a) conditional      run(key, retained=path)        this tree's library
    (b) unconditional    run(key)                       this tree's library
    (c) parent           run(key)                       `--parent-lib`: a libgjx_hip.so built from the parent commit, loaded
                                                        next to this tree's in the same process, timed twice per round
                                                        ((c1), (c2): their spread is the margin of (b) against (c))

(b) against (c) is the regression check of the unconditional hot path; (a) against (b) is the cost of the feature.  Prints
medians and quartiles per run and one JSON line.  `--only unconditional`: configuration (b) alone — with
`GJX_HIP_LIB=<another build>` (the project's A/B switch: tools/ab_lib.sh, tools/time_guided.py) that is (c) in a process of
its own, the way to take it where two libraries in one process are not wanted; a library without include/gjx_csmc.h cannot
run (a).  `--sweeps S`: S sweeps of ParticleGibbs (refresh "trace" and "backward")
at `--n` and `--T`, wall time per sweep with the device idle at both ends, and the share of it the host spends enqueueing
(the time until `run` returns, before the final synchronise)."""
import argparse
import json
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
from genjax._amd.abi import GjxLib  # noqa: E402
from genjax._amd.ops import Ops  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402
from genjax._amd.smc_fused import BootstrapSMC, ParticleGibbs, StateSpaceModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("impl", nargs="?", default="philox", choices=["philox", "threefry"])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--T", type=int, default=100)
ap.add_argument("--blocks", type=int, default=12)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--parent-lib")
ap.add_argument("--only", choices=["unconditional"])
ap.add_argument("--sweeps", type=int, default=0)
args = ap.parse_args()

A, Q, R = W.LGSSM["a"], W.LGSSM["q"], W.LGSSM["r"]
y = W.lgssm_data(args.T)


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


ops = load_hip_ops()  # raises without a GPU: there is no other way to take these numbers
obs = C["y"].set(torch.tensor(y))
key = genjax.random.key(1, args.impl)
model = StateSpaceModel(init, step)
out = dict(impl=args.impl, n=args.n, T=args.T)

if args.sweeps:
    with use_ops(ops):
        smc = BootstrapSMC(model, obs, args.n, record_history=True)
        for refresh in ("trace", "backward"):
            pg = ParticleGibbs(smc, refresh=refresh)
            pg.run(key, 5)  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pg.run(key, args.sweeps)
            t_host = time.perf_counter() - t0
            torch.cuda.synchronize()
            t_all = time.perf_counter() - t0
            out[refresh] = dict(us_per_sweep=t_all / args.sweeps * 1e6, host_us_per_sweep=t_host / args.sweeps * 1e6)
            print(f"refresh={refresh:8s} n={args.n} T={args.T}: {t_all / args.sweeps * 1e6:9.1f} us per sweep, host enqueue "
                  f"{t_host / args.sweeps * 1e6:9.1f} us ({100 * t_host / t_all:.0f} %)")
    print(json.dumps(out))
    sys.exit(0)

path = torch.tensor(y).cuda() * 0.8  # (any path: the retained slot's work does not depend on its values)
configs = {}
here = BootstrapSMC(model, obs, args.n, record_history=True)
if not args.only:
    configs["a_conditional"] = (ops, here, dict(retained=path, log_z=False))
configs["b_unconditional"] = (ops, here, dict(log_z=False))
if args.parent_lib:
    parent_ops = Ops(GjxLib(args.parent_lib, "cuda"))
    for name in ("c1_parent", "c2_parent"):
        # (the bindings and the driver are this tree's; only the library — kernels and C entry points — is the parent's)
        configs[name] = (parent_ops, BootstrapSMC(model, obs, args.n, record_history=True), dict(log_z=False))


def run(o, alg, kw):
    with use_ops(o):
        return alg._run(key, **kw)  # (log_z=False: the stepwise route without its one host read)


for name, (o, alg, kw) in configs.items():  # warm-up: every shape the timed window uses
    for _ in range(2):
        run(o, alg, kw)
torch.cuda.synchronize()
times = {name: [] for name in configs}
for _ in range(args.blocks):
    for name, (o, alg, kw) in configs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.runs):
            run(o, alg, kw)
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / args.runs)

out.update(blocks=args.blocks, runs_per_block=args.runs, parent_lib=args.parent_lib, library=os.environ.get("GJX_HIP_LIB", "this tree's"))
for name, ts in times.items():
    q = statistics.quantiles(ts, n=4)
    med = statistics.median(ts)
    out[name] = dict(ms_per_run=med * 1e3, q1_ms=q[0] * 1e3, q3_ms=q[2] * 1e3, us_per_step=med / args.T * 1e6)
    print(f"{name:16s} {med * 1e3:8.3f} ms per run (quartiles {q[0] * 1e3:.3f} .. {q[2] * 1e3:.3f}) = {med / args.T * 1e6:6.2f} us per step")
m = {k: v["ms_per_run"] for k, v in out.items() if isinstance(v, dict) and "ms_per_run" in v}
if "a_conditional" in m:
    out["a_over_b"] = m["a_conditional"] / m["b_unconditional"]
    print(f"(a) conditional / (b) unconditional = {out['a_over_b']:.4f}")
if args.parent_lib:
    c = 0.5 * (m["c1_parent"] + m["c2_parent"])
    out["b_over_c"], out["c_spread"] = m["b_unconditional"] / c, abs(m["c1_parent"] - m["c2_parent"]) / c
    print(f"(b) this build / (c) parent = {out['b_over_c']:.4f}   spread of (c) measured twice = {out['c_spread']:.4f}")
print(json.dumps(out))
