"""Time the MCMC backward sampler (BootstrapSMC.backward_simulate(..., n_moves=K) -> gjx_backmove_run) in one process
(GPU box):

    python tools/time_backmove.py [philox|threefry] [--model lgssm hmm256] [--n 1000000] [--m N] [--T 100] [--K 0 1 2 4 8]
                                  [--calls 9] [--warmup 2] [--search coarse plain] [--baselines] [--only-K K]

Per model (the LinearGaussianSSM defaults / the 256-state DiscreteHMM of workloads.HMM) one `record_history=True` run of
n particles, then per search variant (GJX_BACKMOVE_SEARCH, read at every call) and per K: HIP-event times of `--calls`
gjx_backmove_run calls (ops.backmove_run: the library call and its output allocation, without the float64 moments and the
distinct counts `backward_simulate` adds — `api_ms` has one timing of those) of m (default n) paths after `--warmup`
untimed ones -> median and quartiles, ns per MOVE
(m K (T - 1) per call), ns per path-step (m T), the launches per call, and the distinct particles at t = 0.  `cdf_build` is
the CDF's share taken on its own: T times the median of one gjx_resample_multinomial with a single draw (the same three
launches over lw[t]).  `--baselines`: `SMCResult.trajectories` at the same n = m, and the exact `backward_simulate` at
n = 65 536, m = 1 024, per path-step.  Prints one JSON line per measurement.  `--only-K K`: one variant, one K, no extras —
e.g. under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax._amd import workloads as W  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402
from genjax._amd.smc_fused import BootstrapSMC, DiscreteHMM, LinearGaussianSSM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("impl", nargs="?", default="philox", choices=["philox", "threefry"])
ap.add_argument("--model", nargs="+", default=["lgssm", "hmm256"], choices=["lgssm", "hmm256"])
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--m", type=int, default=0)
ap.add_argument("--T", type=int, default=100)
ap.add_argument("--K", type=int, nargs="+", default=[0, 1, 2, 4, 8])
ap.add_argument("--calls", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--search", nargs="+", default=["coarse", "plain"], choices=["coarse", "plain"])
ap.add_argument("--baselines", action="store_true")
ap.add_argument("--only-K", type=int, default=None)
args = ap.parse_args()
m = args.m or args.n

ops = load_hip_ops()


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


def make(model, n, T):
    if model == "lgssm":
        return BootstrapSMC(LinearGaussianSSM(), W.lgssm_data(T), n, record_history=True)
    trans, emit = W.hmm_tables()
    return BootstrapSMC(DiscreteHMM(torch.tensor(trans, dtype=torch.float32), torch.tensor(emit, dtype=torch.float32), W.HMM["init_state"]),
                        W.hmm_data(T), n, record_history=True)


with use_ops(ops):
    for model in args.model:
        alg = make(model, args.n, args.T)
        res = alg.run(genjax.random.key(1, args.impl))
        key2 = genjax.random.key(2, args.impl)
        base = dict(tool="time_backmove", impl=args.impl, model=model, n=args.n, m=m, T=args.T)
        alg.backward_simulate(res, key2, n_paths=8, n_moves=1)  # (builds the transition plan, compiles the kernels)
        plan, rows = alg._transition
        cols = list(res.history) if isinstance(res.history, tuple) else [res.history]
        run = lambda K: ops.backmove_run(plan, key2, cols, res.log_weight_history, res.ancestors, rows, m, K)
        if args.only_K is not None:
            os.environ["GJX_BACKMOVE_SEARCH"] = args.search[0]
            k = timed(lambda: run(args.only_K), args.calls, args.warmup)
            print(json.dumps(dict(base, search=args.search[0], K=args.only_K, **k)), flush=True)
            continue
        lw_last = res.log_weight_history[-1].contiguous()
        c = timed(lambda: ops.resample("multinomial", key2.literal(), lw_last, 1), 4 * args.calls, args.warmup)
        for search in args.search:
            os.environ["GJX_BACKMOVE_SEARCH"] = search
            for K in args.K:
                k = timed(lambda: run(K), args.calls, args.warmup)
                holder = {}
                k["api_ms"] = timed(lambda: holder.update(sm=alg.backward_simulate(res, key2, n_paths=m, n_moves=K)), 1, 0)["median_ms"]
                sm = holder["sm"]
                cdfs = args.T if K > 0 else 1
                k.update(search=search, K=K, unique_at_0=int(sm.unique_ancestors[0]), unique_at_mid=int(sm.unique_ancestors[args.T // 2]),
                         launches_per_call=3 * cdfs + args.T, cdf_build_ms=cdfs * c["median_ms"],
                         ns_per_path_step=k["median_ms"] * 1e6 / (float(m) * args.T))
                if K > 0:
                    k["ns_per_move"] = k["median_ms"] * 1e6 / (float(m) * K * (args.T - 1))
                print(json.dumps(dict(base, **k)), flush=True)
        os.environ.pop("GJX_BACKMOVE_SEARCH", None)
        if args.baselines:
            key3 = genjax.random.key(3, args.impl)
            t = timed(lambda: res.trajectories(key3, n_paths=m), args.calls, args.warmup)
            tr = res.trajectories(key3, n_paths=m)
            t.update(what="SMCResult.trajectories", unique_at_0=int(tr.unique_ancestors[0]), ns_per_path_step=t["median_ms"] * 1e6 / (float(m) * args.T))
            print(json.dumps(dict(base, **t)), flush=True)
            ne, me = 65_536, 1024
            alg_e = make(model, ne, args.T)
            res_e = alg_e.run(genjax.random.key(1, args.impl))
            e = timed(lambda: alg_e.backward_simulate(res_e, key2, n_paths=me), max(3, args.calls // 3), 1)
            ex = alg_e.backward_simulate(res_e, key2, n_paths=me)
            e.update(what="exact backward_simulate", unique_at_0=int(ex.unique_ancestors[0]), ns_per_path_step=e["median_ms"] * 1e6 / (float(me) * args.T))
            print(json.dumps(dict(base, n=ne, m=me, **e)), flush=True)
