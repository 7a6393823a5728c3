"""Trajectory trace-back and the history filter, HIP-event medians: python tools/time_paths.py [n] [T]
(a) gjx_paths_trace (one launch: lineage + paths of one f32 column) against the loop a user writes without it
    (`idx = anc[t][idx]; out[t] = x[t][idx]` in torch: 2 launches per step) and against its byte floor;
(b) the stepwise history filter (`record_history=True`) against the whole-run call (replayed graph), per step."""
import sys
sys.path.insert(0, "genjax-chi_amd")
import torch
import genjax
from genjax._amd import workloads as W
from genjax._amd.runtime import load_hip_ops, use_ops
from genjax._amd.smc_fused import BootstrapSMC, LinearGaussianSSM

ops = load_hip_ops()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
COPY_RATE = 6.3e12  # achievable copy rate of the MI355X's HBM, bytes/s


def median_ms(fn, reps=15, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


y = W.lgssm_data(T)
key = genjax.random.key(5, "philox")
with use_ops(ops):
    hist_alg = BootstrapSMC(LinearGaussianSSM(), y, n, record_history=True)
    whole_alg = BootstrapSMC(LinearGaussianSSM(), y, n, record_ancestors=True)
    plain_alg = BootstrapSMC(LinearGaussianSSM(), y, n)
    res = hist_alg.run(key)
    leaves, _, _ = ops.resample("systematic", genjax.random.key(6, "philox").literal(), res.log_weights.contiguous(), n)
    anc, x = res.ancestors, res.history

    def torch_loop():
        idx = leaves.long()
        lin = torch.empty((T, n), dtype=torch.int32, device="cuda")
        out = torch.empty((T, n), dtype=torch.float32, device="cuda")
        for t in range(T - 1, -1, -1):
            lin[t] = idx
            torch.index_select(x[t], 0, idx, out=out[t])
            if t:
                idx = anc[t][idx].long()
        return lin, out

    one = lambda **kw: ops.paths_trace(anc, [x], leaves, leaves_ordered=True, **kw)
    a, (b_lin, b_out) = one(), torch_loop()
    assert torch.equal(a["lineage"], b_lin) and torch.equal(a["paths"][0], b_out)
    floor_ms = 4.0 * T * n * 4 / COPY_RATE * 1e3  # lineage + paths written, ancestors + column read at most
    k_med, k_min = median_ms(one)
    s_med, s_min = median_ms(lambda: one(sums=True, unique=True))
    l_med, l_min = median_ms(torch_loop, reps=7, warm=2)
    print(f"(a) T={T} n=m={n}, one f32 column, lineage + paths:", flush=True)
    print(f"    gjx_paths_trace          {k_med:.3f} ms median (min {k_min:.3f}): {4.0 * T * n * 4 / k_med / 1e9:.2f} TB/s of the "
          f"{4.0 * T * n * 4 / 1e9:.2f} GB bound, {k_med / floor_ms:.2f} x the {floor_ms:.3f} ms byte floor")
    print(f"    ... + sums + distinct    {s_med:.3f} ms median (min {s_min:.3f})")
    print(f"    torch loop (2T launches) {l_med:.3f} ms median (min {l_min:.3f}): {l_med / k_med:.2f} x the one-launch kernel", flush=True)
    h_med, h_min = median_ms(lambda: hist_alg.run(key), reps=9, warm=2)
    w_med, w_min = median_ms(lambda: whole_alg.run(key), reps=9, warm=3)
    p_med, p_min = median_ms(lambda: plain_alg.run(key), reps=9, warm=3)
    print(f"(b) LGSSM filter T={T} n={n}, per step:")
    print(f"    record_history (stepwise)            {h_med * 1e3 / T:.2f} us median (min {h_min * 1e3 / T:.2f})")
    print(f"    run(), record_ancestors (graph)      {w_med * 1e3 / T:.2f} us median (min {w_min * 1e3 / T:.2f})")
    print(f"    run(), default (graph)               {p_med * 1e3 / T:.2f} us median (min {p_min * 1e3 / T:.2f})", flush=True)
