"""A/B of the waves-per-SIMD hint of the importance kernel in ONE process, interleaved rounds (one MI355X):
  GJX_PLAN_JIT_VERBOSE=1 python tools/ab_waves_hint.py [rounds] [form] [passes per launch]
Every variant is the same generated source built under GJX_JIT_DEFINE=GJX_WAVES_HINT=<k> (0 = no hint; "ship" = the
plan's own default, no define).  A hinted build that spills more than 32 B is replaced by the unhinted one, as in
production; with GJX_PLAN_JIT_VERBOSE=1 the library prints the registers and the scratch of every build.
Prints the median / min time per 1e6-particle pass of every variant."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))
import torch  # noqa: E402

from genjax._amd import workloads as W  # noqa: E402
from genjax._amd.ops import HipEvent  # noqa: E402
from genjax._amd.runtime import load_hip_ops  # noqa: E402

ops = load_hip_ops()
N = 1_000_000
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 12
form = sys.argv[2] if len(sys.argv) > 2 else "quad"
L = int(sys.argv[3]) if len(sys.argv) > 3 else 32
os.environ["GJX_JIT_FORM"] = form
variants = []
for hint in ("ship", 0, 4, 5, 6, 7, 8):
    if hint == "ship":
        os.environ.pop("GJX_JIT_DEFINE", None)
    else:
        os.environ["GJX_JIT_DEFINE"] = f"GJX_WAVES_HINT={hint}"
    print(f"--- hint {hint}", file=sys.stderr, flush=True)
    wl = W.Gaussian10(ops, 1, seed=0, n_local=N)
    prep = wl.prepare(fold_batch=L, passes=L)
    prep.launch_passes(0, L)  # builds the kernel under this hint now
    torch.cuda.synchronize()
    variants.append((f"hint {hint}", wl, prep))
os.environ.pop("GJX_JIT_DEFINE", None)
times = {v[0]: [] for v in variants}
for _ in range(10):  # clock ramp
    for name, wl, prep in variants:
        prep.launch_passes(0, L)
torch.cuda.synchronize()
for r in range(rounds):
    for name, wl, prep in variants:
        for _ in range(2):
            prep.launch_passes(0, L)
        a, b = HipEvent(), HipEvent()
        a.record(ops.stream())
        for _ in range(4):
            prep.launch_passes(0, L)
        b.record(ops.stream())
        times[name].append(a.elapsed_ms(b) * 1e3 / (4 * L))
for name, ts in times.items():
    print(f"{form} L={L} {name}: median {statistics.median(ts):7.3f} us/pass   min {min(ts):7.3f}   max {max(ts):7.3f}")
