"""Tempered SMC on the GPU (include/gjx_temper.h): the move launch held bit for bit (tolerance 0) to the replay
tests/temper_ref.py builds from unchanged oracle entry points, the ESS ladder against float64 numpy, the sampler end to end
against the closed form of the linear-Gaussian regression, and the launch counts of a stage."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import genjax
import temper_ref as R
from genjax._amd import abi, prng, temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from test_gpu_guided import _kernel_nodes

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 1000, 1025)  # one lane, a partial tile, a tile edge, quad and pair tails
MODELS = ("regression", "gamma_normal", "beta_bernoulli")
SCALES = {"regression": (1.0, 1.0), "gamma_normal": (1.0, 1.5), "beta_bernoulli": (0.5,)}
# 5 x the RMS error of tests/temper_ref.py's float64 restatement over 64 seeds (default_rng(1000 .. 1063)) at n = 4096,
# K = 2, ESS target 0.5: 0.0827 (profiles/temper_summary.md) — measured on the CPU, not on the code under test
LOG_Z_BOUND = 5 * 0.0827


@pytest.fixture(scope="module")
def lowered(hip_ops, oracle_ops):
    out = {}
    with use_ops(hip_ops):
        for name, target in R.models().items():
            tracer = temper.lower(target, 64)
            plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            plan.set_params(tracer.params)
            out[name] = (plan, {impl: R.Assess(oracle_ops, tracer, impl) for impl in (0, 1)})
    return out


def _columns(name, n, rng, outside=False):
    """Start columns of a model: draws from (about) its prior; `outside`: every fourth value outside a Gamma's / Beta's support."""
    if name == "regression":
        cols = [2.0 * rng.standard_normal(n), 2.0 * rng.standard_normal(n)]
    elif name == "gamma_normal":
        cols = [rng.gamma(2.0, 1.0, n), 2.0 * rng.standard_normal(n)]
    else:
        cols = [rng.beta(2.0, 2.0, n)]
    cols = [c.astype(np.float32) for c in cols]
    if outside and name != "regression":
        bad = np.array([-0.5, 0.0, 1.0, 1.5] if name == "beta_bernoulli" else [-0.5, 0.0, -3.0, -1e-30], dtype=np.float32)
        cols[0][::4] = bad[np.arange(len(cols[0][::4])) % 4]
    return cols


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same(a, b):
    """Equal bit for bit, or NaN in both (a NaN's payload is the platform's, not the specification's)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


@pytest.mark.parametrize("name", MODELS)
def test_assess_pin(hip_ops, lowered, name):
    """K = 0, recompute = 1 on given columns: lp and ll are the oracle's log-densities composed in f32 in table order, bit for
    bit — values outside a Gamma's / Beta's support included (log-density -inf by the header's support rule)."""
    plan, assess = lowered[name]
    rng = np.random.default_rng(7)
    for n in SIZES:
        for outside in (False, True):
            cols = _columns(name, n, rng, outside)
            lp_ref, ll_ref = assess[1](cols)
            if outside and name != "regression" and n >= 4:
                assert np.isneginf(lp_ref).sum() >= n // 4
            for impl in (0, 1):
                x, lp, ll, acc = hip_ops.temper_move(plan, genjax.random.key(3, "philox" if impl else "threefry"), _dev(cols), None,
                                                     None, 0.37, 0, None, recompute=True)
                assert all(np.array_equal(_bits(a.cpu().numpy()), _bits(b)) for a, b in zip(x, cols)), (n, impl)
                assert _same(lp.cpu().numpy(), lp_ref) and not np.isnan(lp_ref).any(), (n, impl, outside)
                assert _same(ll.cpu().numpy(), ll_ref), (n, impl, outside)  # (NaN where an argument is one: 1 / sqrt(tau < 0))
                assert int(acc.sum()) == 0


def _ancestors(n, rng):
    a = rng.integers(0, n, n).astype(np.int64)
    wild = np.array([-1, n, n + 5, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)  # out-of-range words: they clamp to n - 1
    k = min(len(wild), n)
    a[rng.permutation(n)[:k]] = wild[:k]
    return a.astype(np.int32)


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("name", MODELS)
def test_sweep_pin(hip_ops, oracle_ops, lowered, name, impl):
    """K = 3 sweeps, with and without an ancestors column (out-of-range words included), beta in {0, 0.37, 1}: x, lp, ll and
    n_accept are the replay's, bit for bit.  Every case is conditioned ON THE REPLAY first: at least 10 % accepts and 10 %
    rejects (the key of a case is the first of 64 seeds whose replay shows both — with n = 1 a case has three proposals),
    and the Gamma / Beta models reject proposals through lp' = -inf."""
    plan, assess = lowered[name]
    K, scales, impl_name = 3, SCALES[name], "philox" if impl else "threefry"
    outside_total = 0
    for n in SIZES:
        rng = np.random.default_rng(100 + n)
        cols = _columns(name, n, rng)
        lp0, ll0 = assess[impl](cols)
        for with_anc in (False, True):
            anc = _ancestors(n, rng) if with_anc else None
            for beta in (0.0, 0.37, 1.0):
                for seed in range(64):
                    key = genjax.random.key(1000 + seed, impl_name)
                    stats = {}
                    ref = R.move_ref(oracle_ops, assess[impl], key, cols, lp0, ll0, beta, K, scales, ancestors=anc, stats=stats)
                    rate = ref[3].sum() / (n * K)
                    if 0.1 <= rate <= 0.9:
                        break
                else:
                    pytest.fail(f"no key with 10 % accepts and rejects in the replay: {name} n={n} beta={beta}")
                outside_total += stats["outside"]
                x, lp, ll, acc = hip_ops.temper_move(plan, key, _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(),
                                                     beta, K, scales, ancestors=None if anc is None else torch.from_numpy(anc).cuda())
                case = (name, impl, n, with_anc, beta)
                assert np.array_equal(acc.cpu().numpy(), ref[3]), case
                for a, b in zip(x, ref[0]):
                    assert np.array_equal(_bits(a.cpu().numpy()), _bits(b)), case
                assert np.array_equal(_bits(lp.cpu().numpy()), _bits(ref[1])) and np.array_equal(_bits(ll.cpu().numpy()), _bits(ref[2])), case
    if name != "regression":
        assert outside_total > 0  # proposals outside the support were made, and rejected by the rule


def test_sweep_grid_independence(hip_ops, lowered):
    """Nothing depends on the grid: one workgroup striding over the population gives the same bits."""
    plan, assess = lowered["regression"]
    n = 1025
    cols = _columns("regression", n, np.random.default_rng(5))
    lp0, ll0 = assess[1](cols)
    key = genjax.random.key(9, "philox")
    args = (plan, key, _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(), 0.37, 2, (1.0, 1.0))
    a = hip_ops.temper_move(*args)
    b = hip_ops.temper_move(*args, max_workgroups=1)
    assert all(torch.equal(u, v) for u, v in zip(a[0], b[0])) and all(torch.equal(a[k], b[k]) for k in (1, 2, 3))


def _ess(out):
    o = out.cpu().numpy()
    return temper.ess_of(o[0:-1:2], o[1:-1:2]), o[0:-1:2], o[1:-1:2], o[-1]


@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_ess_ladder(hip_ops, n):
    """G = 32 temperatures in one launch: ESS within 1e-4 relative of float64 numpy (an f32 exponential with an argument up
    to about 100 carries at most about 6e-6 relative error from argument rounding); delta = 0 gives exactly n; -inf entries
    contribute nothing; an all-equal column has ESS n; an all -inf column has ESS 0; two calls are bit-equal."""
    rng = np.random.default_rng(n)
    ll = (-20.0 * rng.chisquare(2, n)).astype(np.float32)  # ll - max down to a few hundred below
    deltas = np.concatenate([[0.0], np.exp2(-np.arange(30, -1, -1) / 2.0)]).astype(np.float32)
    assert len(deltas) == 32 and deltas[-1] == 1.0
    ws = hip_ops.temper_ladder_workspace(n)
    out = hip_ops.temper_ess_ladder(torch.from_numpy(ll).cuda(), deltas, ws)
    again = hip_ops.temper_ess_ladder(torch.from_numpy(ll).cuda(), deltas, ws)  # (the same workspace: its ticket is zero again)
    assert torch.equal(out, again)
    ess, s1, s2, M = _ess(out)
    r1, r2, rM = R.ladder_ref(ll, deltas)
    assert M == rM and s1[0] == n and s2[0] == n and ess[0] == n
    ref = temper.ess_of(r1, r2)
    rel = np.abs(ess - ref) / ref
    print(f"n = {n}: largest relative ESS error {rel.max():.3e}; ESS from {ess[0]:.1f} down to {ess[-1]:.3f}")
    assert rel.max() <= 1e-4
    assert np.abs(s1 - r1).max() / n <= 1e-4 and np.all(np.abs(s1 - r1) <= 1e-4 * r1)
    if n >= 4:
        holes = ll.copy()
        holes[::3] = -np.inf
        ess_h, s1_h, _, M_h = _ess(hip_ops.temper_ess_ladder(torch.from_numpy(holes).cuda(), deltas, ws))
        h1, h2, hM = R.ladder_ref(holes, deltas)
        assert M_h == hM and s1_h[0] == np.isfinite(holes).sum() and np.all(np.abs(ess_h - temper.ess_of(h1, h2)) <= 1e-4 * temper.ess_of(h1, h2))
    flat = np.full(n, -3.25, dtype=np.float32)
    ess_f, s1_f, s2_f, M_f = _ess(hip_ops.temper_ess_ladder(torch.from_numpy(flat).cuda(), deltas, ws))
    assert np.all(ess_f == n) and np.all(s1_f == n) and np.all(s2_f == n) and M_f == -3.25
    none = np.full(n, -np.inf, dtype=np.float32)
    ess_n, s1_n, s2_n, M_n = _ess(hip_ops.temper_ess_ladder(torch.from_numpy(none).cuda(), deltas, ws))
    assert np.all(ess_n == 0) and np.all(s1_n == 0) and np.all(s2_n == 0) and M_n == -np.inf


@pytest.fixture(scope="module")
def end_to_end(hip_ops):
    with use_ops(hip_ops):
        alg = TemperedSMC(R.models()["regression"], 4096, n_moves=2, ess_target=0.5)
        key = genjax.random.key(2024, "philox")
        return alg, key, alg.run(key), alg.run(key)


def test_end_to_end_regression(hip_ops, end_to_end):
    """The regression (m = 20, noise 0.1), n = 4096, K = 2, ESS target 0.5."""
    alg, key, a, b = end_to_end
    model = R.Regression()
    assert a.log_marginal_likelihood == b.log_marginal_likelihood and a.betas == b.betas and a.ess == b.ess
    assert a.accept_rate == b.accept_rate and torch.equal(a.lp, b.lp) and torch.equal(a.ll, b.ll)
    assert all(torch.equal(u, v) for u, v in zip(a.columns, b.columns))
    assert torch.equal(a.choices["w"], b.choices["w"]) and torch.equal(a.choices["b"], b.choices["b"])
    sd = np.sqrt(np.diag(model.post_cov))
    w, bb = a.choices["w"].double().mean().item(), a.choices["b"].double().mean().item()
    print(f"stages {len(a.betas) - 1}, betas {a.betas}, ess {a.ess}, accept {a.accept_rate}")
    print(f"log Z-hat {a.log_marginal_likelihood:.4f} against {model.log_z:.4f}; mean errors in posterior deviations: "
          f"w {(w - model.post_mean[0]) / sd[0]:+.3f}, b {(bb - model.post_mean[1]) / sd[1]:+.3f}")
    assert abs(w - model.post_mean[0]) <= 0.25 * sd[0] and abs(bb - model.post_mean[1]) <= 0.25 * sd[1]
    assert abs(a.log_marginal_likelihood - model.log_z) <= LOG_Z_BOUND
    assert a.betas[0] == 0.0 and a.betas[-1] == 1.0 and all(y > x for x, y in zip(a.betas, a.betas[1:]))
    assert len(a.ess) == len(a.accept_rate) == len(a.betas) - 1 and all(0.0 < r < 1.0 for r in a.accept_rate)
    assert all(e >= 0.5 * 4096 * (1 - 1e-4) for e in a.ess)


def test_run_smc_and_estimate_agree_with_run(hip_ops, end_to_end):
    alg, key, a, _ = end_to_end
    with use_ops(hip_ops):
        coll = alg.run_smc(key)
        est = alg.log_marginal_likelihood_estimate(key)
    z32 = float(np.float32(a.log_marginal_likelihood))
    assert est.dtype == torch.float32 and float(est) == z32
    assert len(coll) == 4096 and torch.all(coll.get_log_weights() == z32)
    assert abs(float(coll.get_log_marginal_likelihood_estimate()) - z32) <= 1e-5 * abs(z32)
    ch = coll.get_particles().get_choices()
    assert torch.equal(ch["w"], a.choices["w"]) and torch.equal(ch["b"], a.choices["b"])
    assert coll.result.betas == a.betas


def test_launch_counts(hip_ops, lowered, end_to_end):
    """A stage enqueues exactly ONE move-kernel launch and at most two ladder launches: each library call is one kernel node
    of a captured graph, and a run makes one move call per stage (plus the K = 0 fill of stage 0) and at most two ladder calls."""
    plan, assess = lowered["regression"]
    n = 1000
    cols = _columns("regression", n, np.random.default_rng(1))
    lp0, ll0 = assess[1](cols)
    dev, lp_d, ll_d = _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda()
    key = genjax.random.key(4, "philox")
    anc = torch.arange(n, dtype=torch.int32).cuda()
    ws = hip_ops.temper_ladder_workspace(n)
    deltas = temper.ladder_deltas(0.0)
    hip_ops.temper_move(plan, key, dev, lp_d, ll_d, 0.5, 2, (0.1, 0.1), ancestors=anc)  # (compiled before the capture)
    hip_ops.temper_ess_ladder(ll_d, deltas, ws)
    counts = {}
    side = torch.cuda.Stream()
    for what in ("move", "ladder"):
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g, stream=side):
            if what == "move":
                out = hip_ops.temper_move(plan, key, dev, lp_d, ll_d, 0.5, 2, (0.1, 0.1), ancestors=anc)
            else:
                out = hip_ops.temper_ess_ladder(ll_d, deltas, ws)
        counts[what] = _kernel_nodes(g.raw_cuda_graph())
        g.replay()
        torch.cuda.synchronize()
        del g, out
    print("kernel nodes per call:", counts)
    assert counts == {"move": 1, "ladder": 1}
    alg, key, a, _ = end_to_end
    calls = {"move": 0, "ladder": 0}
    move, ladder = hip_ops.temper_move, hip_ops.temper_ess_ladder

    def count(name, fn):
        def wrapped(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)
        return wrapped

    hip_ops.temper_move, hip_ops.temper_ess_ladder = count("move", move), count("ladder", ladder)
    try:
        with use_ops(hip_ops):
            res = alg.run(key)
    finally:
        del hip_ops.temper_move, hip_ops.temper_ess_ladder
    stages = len(res.betas) - 1
    assert res.betas == a.betas and calls["move"] == stages + 1 and stages <= calls["ladder"] <= 2 * stages - 1
