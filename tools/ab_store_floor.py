"""The flagship importance launch against its two floors, in ONE process, interleaved rounds (one MI355X):
  python tools/ab_store_floor.py [--rounds R] [--passes L] [--particles N]
The 10-latent Gaussian plan, seeds 0, 1, ... as bench.py takes them, L (default 32) passes per launch, every launch between
two HIP events after an untimed ramp.  Variants:
  shipped      the kind of store the library's rule picks (ImportanceVariant::of_launch)
  no columns   the same model with no per-particle output: the launch passes only row_e and row_s, so the generated source has
               no column store — the vector-only time.  (Without value columns the quad form runs four rows per workgroup, and
               its source asks about every output: the guarded form, which prices 1 % above the full-outputs one.)
  plain | wt | nt | nt+wt
               every kind of store, forced through its escape (GJX_JIT_DEFINE=GJX_STORES_*)
Prints the median / min time per pass of every variant, the rate at which its columns are written, and the step time of
back-to-back launches (one event pair round a run of launches).  The kinds are timed in interleaved rounds whose order rotates;
the launch without columns is timed afterwards, on its own."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genjax-chi_amd"))
import torch  # noqa: E402

from genjax._amd import prng, workloads as W  # noqa: E402
from genjax._amd.ops import HipEvent  # noqa: E402
from genjax._amd.runtime import load_hip_ops  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--passes", type=int, default=32)
ap.add_argument("--particles", type=int, default=1_000_000)
args = ap.parse_args()
ops = load_hip_ops()
N, L = args.particles, args.passes
ESCAPES = {"shipped": None, "plain": "GJX_STORES_PLAIN", "wt": "GJX_STORES_WT", "nt": "GJX_STORES_NT", "nt+wt": "GJX_STORES_NT_WT"}


def force(escape):
    if escape is None:
        os.environ.pop("GJX_JIT_DEFINE", None)
    else:
        os.environ["GJX_JIT_DEFINE"] = escape


# ONE prepared launch, so that every kind writes the same buffers (the same 1.55 GB written from another allocation timed up to
# 10 % apart): the escape is read at each launch and picks the plan's kernel of that kind
wl = W.Gaussian10(ops, 1, seed=0, n_local=N)
prep = wl.prepare(fold_batch=L, passes=L)
variants = []  # (name, escape, prepared launch, bytes of columns per pass)
for name, escape in ESCAPES.items():
    force(escape)
    prep.launch_passes(0, L)  # builds the kernel of this kind now
    variants.append((name, escape, prep, 4 * N * (W.G10_LATENTS + 2)))
force(None)
sites = W.gaussian10_sites(W.gaussian10_data())
for s in sites:
    s.out_col = -1
plan = ops.plan_create(sites)
keys = [W.importance_particle_keys(prng.key(p, 1), N) for p in range(L)]
bare = ops.prepare_importance(plan, keys if L > 1 else keys[0], N, [], [], fold_batch=L, estimate_only=True)
bare.launch_passes(0, L)
torch.cuda.synchronize()

REPS = 4
times, steps = {}, {}


def measure(group, rounds):
    """Interleaved rounds over `group`, its order rotated by one every round: what a launch finds behind it (dirty lines, and the
    clock the chip settled at under the previous variant's power) is spread over the variants.  (Unrotated, with the launch that
    writes nothing in the same loop, the kind timed after it came out 12 % faster than the same kernel elsewhere in the order.)"""
    for name, *_ in group:
        times[name], steps[name] = [], []
    for _ in range(20):  # clock ramp
        for name, escape, p, _b in group:
            force(escape)
            p.launch_passes(0, L)
    torch.cuda.synchronize()
    for r in range(rounds):
        k = r % len(group)
        for name, escape, p, _b in group[k:] + group[:k]:
            force(escape)
            for _ in range(2):
                p.launch_passes(0, L)
            evs = [(HipEvent(), HipEvent()) for _ in range(REPS)]
            for a, b in evs:
                a.record(ops.stream())
                p.launch_passes(0, L)
                b.record(ops.stream())
            torch.cuda.synchronize()
            times[name] += [a.elapsed_ms(b) * 1e3 / L for a, b in evs]
            steps[name].append(evs[0][0].elapsed_ms(evs[-1][1]) * 1e3 / (REPS * L))


measure(variants, args.rounds)
none = [("no columns", None, bare, 0)]
measure(none, args.rounds)  # on its own: it draws less power than the others, and the chip's clock follows
variants = variants[:1] + none + variants[1:]
force(None)
print(f"{N} particles, {L} passes per launch, {args.rounds} rounds x {REPS} launches per variant")
for name, escape, prep, nbytes in variants:
    ts = times[name]
    med = statistics.median(ts)
    rate = f"{nbytes / (med * 1e-6) / 1e12:5.2f} TB/s" if nbytes else "    -     "
    print(f"{name:10s}: per pass median {med:6.2f} us  min {min(ts):6.2f}  ({rate})   step back to back median {statistics.median(steps[name]):6.2f} us per pass")
