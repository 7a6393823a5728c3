"""Time the backward-simulation smoother (BootstrapSMC.backward_simulate -> gjx_backsim_run) next to the same computation
written in torch, in one process (GPU box):

    python tools/time_backsim.py [philox|threefry] [--n 65536 1000000] [--T 100] [--m 1024] [--calls 15] [--warmup 3] [--torch-calls 3]
                                 [--clock-ghz 2.4] [--lane-instr 124] [--only kernel|torch]

The model is the LinearGaussianSSM of the defaults; the history comes from one `record_history=True` run per n.  Per n:
HIP-event times of `--calls` whole backward passes after `--warmup` untimed ones -> the median and the quartiles, pairs
(candidate x trajectory x step) per second, time per backward step, and — with `--lane-instr`, the VALU instructions per
pair counted from the disassembled inner loop (tests/test_backsim_cpu.py prints it) — the share of the VALU issue rate
256 CUs x 4 SIMDs x 16 lanes x `--clock-ghz` this implies.  The torch version is what a user writes today: per step, for
chunks of trajectories, an [m_chunk, n] block of logits (log-weight + Normal transition log-density), an equal block of
Gumbels and an argmax; its draws are torch's own, so only times are compared.  Prints one JSON line per n.  `--only kernel`:
the smoother alone, e.g. under `rocprofv3 --kernel-trace --stats` (T launches and the final one per call).
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))
import torch  # noqa: E402

import genjax  # noqa: E402
from genjax._amd import workloads as W  # noqa: E402
from genjax._amd.runtime import load_hip_ops, use_ops  # noqa: E402
from genjax._amd.smc_fused import BootstrapSMC, LinearGaussianSSM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("impl", nargs="?", default="philox", choices=["philox", "threefry"])
ap.add_argument("--n", type=int, nargs="+", default=[65_536, 1_000_000])
ap.add_argument("--T", type=int, default=100)
ap.add_argument("--m", type=int, default=1024)
ap.add_argument("--calls", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--torch-calls", type=int, default=3)  # (a torch pass at n = 1e6 takes seconds)
ap.add_argument("--clock-ghz", type=float, default=2.4)
ap.add_argument("--lane-instr", type=float, default=0.0)
ap.add_argument("--only", choices=["kernel", "torch"])
args = ap.parse_args()

ops = load_hip_ops()
y = W.lgssm_data(args.T)
A, Q = W.LGSSM["a"], W.LGSSM["q"]
LOGNORM = -math.log(Q) - 0.5 * math.log(2.0 * math.pi)


def torch_backward(hist, lw, m):
    """The same pass as a user writes it: chunked [m, n] logits + Gumbel + argmax per step."""
    T, n = lw.shape
    chunk = max(1, min(m, (1 << 27) // n))  # three f32 blocks of at most 0.5 GB each
    idx = torch.empty((T, m), dtype=torch.int64, device=lw.device)
    for t in range(T - 1, -1, -1):
        for lo in range(0, m, chunk):
            hi = min(m, lo + chunk)
            if t == T - 1:
                logits = lw[t].expand(hi - lo, n)
            else:
                xn = hist[t + 1][idx[t + 1, lo:hi]]
                z = (xn[:, None] - A * hist[t][None, :]) / Q
                logits = lw[t][None, :] + (LOGNORM - 0.5 * z * z)
            g = -torch.log(-torch.log(torch.rand((hi - lo, n), device=lw.device).clamp_min(1e-38)))
            idx[t, lo:hi] = torch.argmax(logits + g, dim=1)
    return idx, torch.gather(hist, 1, idx)


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


with use_ops(ops):
    for n in args.n:
        alg = BootstrapSMC(LinearGaussianSSM(), y, n, record_history=True)
        res = alg.run(genjax.random.key(1, args.impl))
        key2 = genjax.random.key(2, args.impl)
        pairs = float(n) * args.m * args.T
        out = dict(tool="time_backsim", impl=args.impl, n=n, T=args.T, m=args.m, pairs_per_call=pairs)
        if args.only != "torch":
            k = timed(lambda: alg.backward_simulate(res, key2, n_paths=args.m), args.calls, args.warmup)
            k["pairs_per_s"] = pairs / (k["median_ms"] * 1e-3)
            k["ms_per_step"] = k["median_ms"] / args.T
            if args.lane_instr > 0:
                k["valu_issue_share"] = k["pairs_per_s"] * args.lane_instr / (256 * 4 * 16 * args.clock_ghz * 1e9)
            out["kernel"] = k
        if args.only != "kernel":
            hist, lw = res.history.contiguous(), res.log_weight_history.contiguous()
            tc = timed(lambda: torch_backward(hist, lw, args.m), args.torch_calls, 1)
            tc["pairs_per_s"] = pairs / (tc["median_ms"] * 1e-3)
            out["torch"] = tc
        if "kernel" in out and "torch" in out:
            out["torch_over_kernel"] = out["torch"]["median_ms"] / out["kernel"]["median_ms"]
        print(json.dumps(out), flush=True)
