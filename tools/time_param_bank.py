"""Time the PARAMETERISED LGSSM user model (StateSpaceModel(..., params=("a", "q", "r")): one compiled plan, theta read from
a row of launch parameters) next to the same model with its numbers baked into the source as literals:

  (a) step time, n = 1e6, T = 100, one filter and a bank of 16 — the two plans' runs interleaved, medians over blocks;
  (b) what a user gets: wall time for log Z at 16 different theta — 16 literal plans built, compiled and run against ONE
      bank run of the parameterised plan — with the compile count of each.

  python tools/time_param_bank.py [philox|threefry] [--blocks 24] [--runs 4] [--json out.json]   (GPU box)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import smc_params_ref as R  # noqa: E402
from genjax._amd import prng, workloads as W  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402
from genjax.inference.smc import BootstrapSMC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("impl", nargs="?", default="philox", choices=["philox", "threefry"])
ap.add_argument("--blocks", type=int, default=24)
ap.add_argument("--runs", type=int, default=4, help="runs per timed block")
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--json", default=None)
args = ap.parse_args()

ops = load_hip_ops()
n, T = args.n, args.steps
obs = R.observations(T)
theta = np.asarray([W.LGSSM["a"], W.LGSSM["q"], W.LGSSM["r"]], dtype=np.float32)
out = dict(impl=args.impl, n=n, T=T, blocks=args.blocks, runs_per_block=args.runs)


def timed(fn, runs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / runs


with use_ops(ops):
    param = BootstrapSMC(R.lgssm_param_model(), obs, n, params=theta)
    baked = BootstrapSMC(R.lgssm_literal_model(theta), obs, n)
    # ---- (a) interleaved step times
    for F in (1, 16):
        keys = R.keys_for(args.impl, F, seed=3)
        pm, bm = param._bind(ops, theta), baked._bind(ops)
        pairs = [W.smc_key_schedule(k, T) for k in keys]
        sk, rk = (pairs[0] if F == 1 else (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])))
        param._set_rows(pm, theta[None] if F == 1 else np.tile(theta, (F, 1)) * (1.0 + 0.001 * np.arange(F))[:, None])
        run_p = lambda: ops._smc_run(pm, keys[0].impl, n, sk, rk)  # noqa: E731
        run_b = lambda: ops._smc_run(bm, keys[0].impl, n, sk, rk)  # noqa: E731
        for fn in (run_p, run_b):  # warm-up: compilation, buffers
            timed(fn, 2)
        tp, tb = [], []
        for _ in range(args.blocks):
            tb.append(timed(run_b, args.runs))
            tp.append(timed(run_p, args.runs))
        mp, mb = statistics.median(tp), statistics.median(tb)
        q = lambda xs: (sorted(xs)[len(xs) // 4], sorted(xs)[(3 * len(xs)) // 4])  # noqa: E731
        out[f"step_us_param_F{F}"], out[f"step_us_baked_F{F}"] = mp / T * 1e6, mb / T * 1e6
        out[f"quartiles_us_param_F{F}"] = [x / T * 1e6 for x in q(tp)]
        out[f"quartiles_us_baked_F{F}"] = [x / T * 1e6 for x in q(tb)]
        print(f"(a) F={F:2d}: per step  baked {mb / T * 1e6:8.3f} us (quartiles {q(tb)[0] / T * 1e6:.3f} .. {q(tb)[1] / T * 1e6:.3f})   "
              f"parameterised {mp / T * 1e6:8.3f} us (quartiles {q(tp)[0] / T * 1e6:.3f} .. {q(tp)[1] / T * 1e6:.3f})   "
              f"ratio {mp / mb:.4f}   {F * n * T / mp:.3e} particle-steps/s", flush=True)
    # ---- (b) log Z at 16 theta: 16 literal plans against one bank run
    F = 16
    rows = R.lgssm_rows(F) + np.float32(0.00123)  # (values no earlier plan of this process was compiled for)
    keys = R.keys_for(args.impl, F, seed=4)
    c0 = ops.jit_stats()["compiles"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lz_lit = [BootstrapSMC(R.lgssm_literal_model(rows[f]), obs, n).run(keys[f]).log_marginal_likelihood for f in range(F)]
    torch.cuda.synchronize()
    t_lit = time.perf_counter() - t0
    c1 = ops.jit_stats()["compiles"]
    fresh = BootstrapSMC(R.lgssm_param_model(), obs, n)  # a new filter object: lowering included, its kernel is cached
    t0 = time.perf_counter()
    lz_bank = fresh.log_marginal_likelihoods(keys, rows)
    torch.cuda.synchronize()
    t_bank = time.perf_counter() - t0
    c2 = ops.jit_stats()["compiles"]
    t0 = time.perf_counter()
    fresh.log_marginal_likelihoods(keys, rows + np.float32(0.002))
    torch.cuda.synchronize()
    t_bank2 = time.perf_counter() - t0
    assert lz_bank.tolist() == lz_lit, "the bank and the 16 literal plans disagree"
    out.update(wall_s_16_literal_plans=t_lit, compiles_16_literal_plans=int(c1 - c0), wall_s_bank_first=t_bank,
               compiles_bank=int(c2 - c1), wall_s_bank_next_theta=t_bank2)
    print(f"(b) log Z at 16 theta: 16 literal plans {t_lit:.3f} s ({c1 - c0} compilations); one bank run {t_bank * 1e3:.2f} ms "
          f"({c2 - c1} compilations), the next 16 theta {t_bank2 * 1e3:.2f} ms; results equal bit for bit")
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
