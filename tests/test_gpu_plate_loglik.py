"""gjx_plate_loglik on the GPU: ll and lp bit for bit against the header's chunked float64 sum restated in numpy over the per-row
f32 terms of tests/group_ref.py's replay, against the move kernel at one chunk, whatever the grid; ImportanceK's route over it."""

import math

import numpy as np
import pytest
import torch

import genjax
import group_ref as G
import plate_ref as P
from genjax._amd import abi, prng, temper
from genjax._amd.plan import PlanUnsupported, _make_plan
from genjax._amd.runtime import use_ops
from genjax.inference.smc import ImportanceK
from test_gpu_plate import _dev, _equal, _same
from test_plate_loglik_cpu import MODELS, lower_all

pytestmark = pytest.mark.gpu

RS, D_MAX = (4, 8, 64), 2 * 64 + 3
EDGE = np.array([np.nan, 1e30, -1e30, 0.25], dtype=np.float32)  # the first latent's first entries; a Gamma latent gets -0.5


@pytest.fixture(scope="module")
def lowered(hip_ops):
    return lower_all(hip_ops, D_MAX)  # (a case sets the first D rows)


def population(tracer, n, seed):
    rng = np.random.default_rng(seed)
    lat = [s for s in tracer.sites if s.observed == 0]
    x = [(rng.gamma(4.0, 1.0, n) if s.dist == abi.DIST_GAMMA else 0.5 + 0.5 * rng.standard_normal(n)).astype(np.float32) for s in lat]
    x[0][:len(EDGE)] = EDGE[:n]
    x[-1][min(3, n - 1)] = -0.5 if lat[-1].dist == abi.DIST_GAMMA else x[-1][min(3, n - 1)]  # outside a Gamma's support
    return x


class Reference:
    """The header in numpy for one (model, population): lp and every term once; ll(D, R) folds the first D rows in chunks of R."""

    def __init__(self, oracle_ops, tracer, data, x):
        a = G.Assess(oracle_ops, tracer, data, [0, len(data[0])])
        n, ins = len(x[0]), a._ins(x)
        assert {kind for kind, _, _ in a.terms} == {"latent", "plated"}  # (the four models: ll is the plated sites' alone)
        with np.errstate(all="ignore"):
            self.lp = a.flat(x)[0]
            self.rows = [np.stack([a._row(plan, d, ins, n) for d in range(len(data[0]))]).astype(np.float64)
                         for kind, plan, _ in a.terms if kind == "plated"]

    def ll(self, D, R):
        ll = np.zeros(len(self.lp), dtype=np.float32)
        with np.errstate(all="ignore"):
            for t in self.rows:
                acc = np.zeros(len(ll), dtype=np.float64)
                for lo in range(0, D, R):
                    part = np.zeros(len(ll), dtype=np.float64)
                    for d in range(lo, min(lo + R, D)):
                        part = part + t[d]
                    acc = acc + part
                ll = (ll + acc.astype(np.float32)).astype(np.float32)
        return ll


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
@pytest.mark.parametrize("name", MODELS)
def test_bits_against_the_specification(hip_ops, oracle_ops, lowered, name, n):
    """ll_out and lp_out at every (R, D): one chunk, an exact boundary, every block-of-four remainder, a short last chunk."""
    tracer, plan, data = lowered[name]
    x = population(tracer, n, 100 + n)
    ref = Reference(oracle_ops, tracer, data, x)
    for R in RS:
        for D in sorted({1, 3, 4, 5, R - 1, R, R + 1, 2 * R + 3}):
            plan.set_data(_dev([c[:D] for c in data]))
            ll, lp = hip_ops.plate_loglik(plan, _dev(x), rows_per_chunk=R)
            assert _same(lp.cpu().numpy(), ref.lp) and _same(ll.cpu().numpy(), ref.ll(D, R)), (name, n, R, D)


@pytest.mark.parametrize("name", MODELS)
def test_one_chunk_is_the_move_kernel_and_no_grid_matters(hip_ops, lowered, name):
    """rows_per_chunk >= D: the bits of gjx_temper_move(n_moves = 0, recompute = 1); max_workgroups in {0, 1, 7}: equal bits."""
    tracer, plan, data = lowered[name]
    x = _dev(population(tracer, 1000, 7))
    for D in (5, D_MAX):
        plan.set_data(_dev([c[:D] for c in data]))
        _, lp_m, ll_m, _ = hip_ops.temper_move(plan, prng.key(1, 1), x, None, None, 0.0, 0, None, recompute=True, want_accept=False)
        for R in (D_MAX + 1, 4):
            first = None
            for wg in (0, 1, 7):
                ll, lp = hip_ops.plate_loglik(plan, x, rows_per_chunk=R, max_workgroups=wg)
                got = (lp.cpu().numpy(), ll.cpu().numpy())
                first = first or got
                assert _same(got[0], first[0]) and _same(got[1], first[1]), (name, D, R, wg)
            if R > D:
                assert _same(first[0], lp_m.cpu().numpy()) and _same(first[1], ll_m.cpu().numpy()), (name, D)


def test_importance_route(hip_ops, oracle_ops):
    """The columns are the prior-table plan's draws under the documented key batch, the log-weights the specification's ll, log Z
    their float64 log-sum-exp minus log K within the bound of tests/test_gpu_parity_abi.py::test_logsumexp (gjx_logsumexp_f32)."""
    K, D = 1000, 37
    target = P.target("normal", D, seed=3)[0]
    key = genjax.random.key(11, "philox")
    with use_ops(hip_ops):
        alg = ImportanceK(target, k_particles=K)
        choices, lw, ess = alg.weighted_population(key)
        est = alg.log_marginal_likelihood_estimate(key)
        with pytest.raises(PlanUnsupported, match="run_smc.*'y'"):
            alg.run_smc(key)
        with pytest.raises(PlanUnsupported, match="grouped latent at address 'a'"):
            ImportanceK(G.target("intercept", (3, 2, 4))[0], k_particles=K).log_marginal_likelihood_estimate(key)
        tracer = temper.lower(target, K)
        kb = prng.split_lazy(prng.split_at(prng.split_at(key, 1), 1), K)
        vals = hip_ops.importance_run(_make_plan(temper.prior_table(tracer)), kb, K, [], [torch.float32] * tracer.n_out,
                                      want_score=False, want_max_partials=False)[0]
    x = [choices["w"], choices["b"]]
    assert torch.equal(x[0], vals[0]) and torch.equal(x[1], vals[1])
    want = Reference(oracle_ops, tracer, [c.numpy() for c in tracer.data_columns("cpu")], [c.cpu().numpy() for c in x]).ll(D, 64)
    assert _equal(lw.cpu().numpy(), want)
    w = np.exp(want.astype(np.float64) - want.max())
    lz = float(np.float32(want.max() + math.log(w.sum()) - math.log(K)))
    assert est.dtype == torch.float32 and est.is_cuda and abs(float(est) - lz) < 1e-5 * max(1.0, abs(lz))
    assert float(ess) == pytest.approx(w.sum() ** 2 / (w * w).sum(), rel=1e-5)  # (f32 exponentials in the ladder: a few 2^-24 each)
