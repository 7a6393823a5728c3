"""The check kernels of a plan with grouped latents on the GPU (include/gjx_group_checks.h): the pointwise table against the
float64 reductions of the oracle's terms, PSIS-LOO against np.sort and the float64 restatement at the flat suite's
tolerances, the predictive draws bit for bit against the oracle's replay, kernels out of the JIT cache for other data and
another group layout, and pointwise / loo / predictive of the public API end to end against the closed form of the
random-intercept model."""

import math

import numpy as np
import pytest
import torch

import genjax
import group_checks_ref as GC
import group_ref as GR
import pointwise_ref as W
import predictive_ref as PR
import psis_ref as S
from genjax import ChoiceMap, Target
from genjax._amd import temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PSISLOO, PointwiseLikelihood, PosteriorPredictive, TemperedSMC
from test_gpu_pointwise import _check as check_pointwise
from test_gpu_psis import _check as check_psis

pytestmark = pytest.mark.gpu

POINTWISE_NS = (5, 301, 513)  # one chunk with a remainder; two chunks with a remainder each; three chunks, g * n + i odd-aligned
PSIS_NS = (301, 513, 6000)    # 6000: several chunks of more than one round of 256 (tests/test_gpu_psis_shapes.py TRIP_CASES)
PREDICTIVE_NS = (5, 301)


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


class Case:
    """One model over one layout, lowered once: the plan with its data and groups set, and the oracle's Assess."""

    def __init__(self, hip_ops, oracle_ops, name, G, seed=0):
        self.name, self.G, self.sizes = name, G, GC.LAYOUTS[G]
        with use_ops(hip_ops):
            self.target, self.g, self.off = GR.target(name, self.sizes, seed)
            self.tracer = temper.lower(self.target, 64)
            self.plan = hip_ops.temper_plan_create(self.tracer.sites, keep=(self.tracer.keep, self.tracer))
        self.data = [t.detach().to(torch.float32).numpy().copy() for t in self.tracer.data_columns("cpu")]
        self.D = len(self.g)
        assert self.D == GC.ROWS[G] and self.plan.n_grouped == GR.GROUPED[name]
        if self.tracer.params:
            self.plan.set_params(self.tracer.params)
        self.plan.set_data(_dev(self.data))
        self.plan.set_groups(torch.from_numpy(self.off).cuda())
        self.assess = GR.Assess(oracle_ops, self.tracer, self.data, self.off)

    def table_order(self, x, z):
        """The latent columns in table order, as `choices` holds them."""
        xs, zs = iter(x), iter(z)
        return [next(zs) if m.get("grouped") else next(xs) for m in self.tracer.meta if m["obs"] is None]


@pytest.fixture(scope="module")
def cases(hip_ops, oracle_ops):
    made = {}

    def get(name, G):
        if (name, G) not in made:
            made[name, G] = Case(hip_ops, oracle_ops, name, G)
        return made[name, G]

    return get


# ---- pointwise ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", sorted(GC.LAYOUTS), ids=lambda G: f"D{GC.ROWS[G]}-G{G}")
@pytest.mark.parametrize("name", ("intercept", "slope", "flat"))
def test_pointwise_pin(hip_ops, cases, name, G):
    c = cases(name, G)
    rng = np.random.default_rng(41)
    chunks = set()
    pops = [GC.centred_columns(name, c.sizes, n, rng) for n in POINTWISE_NS]
    for n, (x, z), t in zip(POINTWISE_NS, pops, GC.terms_many(c.assess, pops)):
        assert t.shape == (c.D, n) and np.isfinite(t).all()
        dx, dz = _dev(x), _dev(z)
        out = hip_ops.temper_pointwise(c.plan, dx, z=dz)
        again = hip_ops.temper_pointwise(c.plan, dx, z=dz)
        assert out.shape == (4, c.D) and out.dtype == torch.float64 and out.is_cuda
        assert torch.equal(out.view(torch.int64), again.view(torch.int64)), (name, G, n)
        check_pointwise(out.cpu().numpy(), t, (name, G, n))  # count exact, s1 / s2 within moment_bounds, lse within LSE_TOL
        chunks.add(int(hip_ops.lib.call("gjx_pointwise_chunks", n, c.D)))
    assert chunks == {1, 2, 3}


def test_pointwise_nan_terms(hip_ops, cases):
    """`gamma` with every fourth grouped value outside its support (negative, zero, NaN, a tiny negative scale): NaN terms
    reach s1 / s2 and skip lse / count."""
    c = cases("gamma", 7)
    n = 301
    x, z = GR.columns("gamma", c.G, n, np.random.default_rng(42), outside=True)
    t = GC.terms(c.assess, x, z)
    bad = np.isnan(t)
    assert bad.any(axis=1).all() and not bad.all(axis=1).any()
    got = hip_ops.temper_pointwise(c.plan, _dev(x), z=_dev(z)).cpu().numpy()
    ref = W.reduce64(t)
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and np.isnan(ref[1]).all()
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[3], n - (bad | np.isneginf(t)).sum(axis=1))
    print("NaN terms per row", bad.sum(axis=1).min(), "..", bad.sum(axis=1).max(), "; lse err", np.abs(got[0] - ref[0]).max())
    assert np.isfinite(ref[0]).all() and np.all(np.abs(got[0] - ref[0]) <= W.LSE_TOL)


# ---- PSIS --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (17, 7), ids=lambda G: f"D{GC.ROWS[G]}-G{G}")
@pytest.mark.parametrize("name", ("intercept", "flat"))
def test_psis_pin(hip_ops, cases, name, G):
    c = cases(name, G)
    rng = np.random.default_rng(43)
    pops = [GC.centred_columns(name, c.sizes, n, rng) for n in PSIS_NS]
    for n, (x, z), t in zip(PSIS_NS, pops, GC.terms_many(c.assess, pops)):
        M = S.tail_len(n)
        assert np.isfinite(t).all() and M == int(hip_ops.lib.call("gjx_psis_tail_len", n, 1.0))
        dx, dz = _dev(x), _dev(z)
        out, tail = hip_ops.temper_psis(c.plan, dx, M, want_tail=True, z=dz)
        out2, tail2 = hip_ops.temper_psis(c.plan, dx, M, want_tail=True, z=dz)
        assert out.shape == (7, c.D) and out.dtype == torch.float64 and tail.shape == (c.D, M + 1) and tail.dtype == torch.float32
        assert torch.equal(out.view(torch.int64), out2.view(torch.int64)) and torch.equal(tail.view(torch.int32), tail2.view(torch.int32))
        check_psis(out.cpu().numpy(), tail.cpu().numpy(), t, M, (name, G, n))
        # the public call on the columns in table order: the same table, and its pointwise table is the pointwise call's —
        # the term is one function in both kernels, so the smallest entry of a row's tail bounds its lse from below
        with use_ops(hip_ops):
            alg = TemperedSMC(c.target, n)
            cols = c.table_order(dx, dz)
            loo = alg.loo(cols)
            pw = alg.pointwise(cols)
        assert isinstance(loo, PSISLOO) and isinstance(pw, PointwiseLikelihood) and loo.tail_len == M
        assert torch.equal(loo.elpd_loo.view(torch.int64), out[0].view(torch.int64)) and torch.equal(loo.khat.view(torch.int64), out[1].view(torch.int64))
        direct = hip_ops.temper_pointwise(c.plan, dx, z=dz)
        assert torch.equal(loo.pointwise.lppd.view(torch.int64), pw.lppd.view(torch.int64))
        assert torch.equal(loo.pointwise.lppd.view(torch.int64), (direct[0] - math.log(n)).view(torch.int64))
        assert bool((direct[0] >= tail[:, M].double()).all())  # (lse >= the row's maximum >= its M-th smallest entry)


# ---- predictive ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ("threefry", "philox"))
@pytest.mark.parametrize("G", (1, 17, 7), ids=lambda G: f"D{GC.ROWS[G]}-G{G}")
@pytest.mark.parametrize("name", ("intercept", "slope", "gamma"))
def test_predictive_pin(hip_ops, oracle_ops, cases, name, G, impl):
    c = cases(name, G)
    key = genjax.random.key(7, impl)
    replay = GC.Replay(oracle_ops, c.tracer, c.data, c.off, key.impl)
    rng = np.random.default_rng(44)
    for n in PREDICTIVE_NS:
        x, z = GC.centred_columns(name, c.sizes, n, rng)
        y = replay.draws(key, x, z)
        assert y.shape == (1, c.D, n) and np.isfinite(y).all()
        dx, dz = _dev(x), _dev(z)
        for k in (1, 7):
            out, draws = hip_ops.temper_predictive(c.plan, key, dx, k, z=dz)
            again, draws2 = hip_ops.temper_predictive(c.plan, key, dx, k, z=dz)
            m = -(-n // k)
            assert out.shape == (1, 5, c.D) and out.dtype == torch.float64 and draws.shape == (1, m, c.D) and draws.dtype == torch.float32
            assert torch.equal(out.view(torch.int64), again.view(torch.int64)) and torch.equal(draws.view(torch.int32), draws2.view(torch.int32))
            assert PR.same_bits(draws.cpu().numpy(), np.transpose(y, (0, 2, 1))[:, ::k]), (name, G, impl, n, k)
            PR.check(out.cpu().numpy(), y, replay.observed(), (name, G, impl, n, k))
        none, nothing = hip_ops.temper_predictive(c.plan, key, dx, 0, z=dz)
        assert nothing is None and torch.equal(none.view(torch.int64), out.view(torch.int64))


# ---- routing ---------------------------------------------------------------------------------------------------------------------------------
def test_kernels_come_out_of_the_jit_cache(hip_ops, oracle_ops, cases):
    """A held-out target — other data, another D and another group layout of the same G — compiles nothing, and its table is
    the reference's on those rows."""
    c = cases("intercept", 5)
    n = 301
    x, z = GC.centred_columns("intercept", c.sizes, n, np.random.default_rng(45))
    key = genjax.random.key(8, "philox")
    other = [2, 0, 6, 1, 8]  # G = 5, D = 17
    with use_ops(hip_ops):
        alg = TemperedSMC(c.target, n)
        cols = c.table_order(_dev(x), _dev(z))
        first, _, _ = alg.pointwise(cols), alg.loo(cols), alg.predictive(cols, key)
        assert first.lppd.shape == (13,)
        before = hip_ops.jit_stats()["compiles"]
        held, g2, off2 = GR.target("intercept", other, seed=3)
        pw = alg.pointwise(cols, target=held)
        pp = alg.predictive(cols, key, target=held, draw_stride=1)
        assert hip_ops.jit_stats()["compiles"] == before
        tr2 = temper.lower(held, 64)
    data2 = [t.detach().to(torch.float32).numpy().copy() for t in tr2.data_columns("cpu")]
    t = GC.terms(GR.Assess(oracle_ops, tr2, data2, off2), x, z)
    assert pw.lppd.shape == (17,) and pw.n == n
    ref = W.reduce64(t)
    assert W.spread(t).max() < W.LSE_MAX_SPREAD
    assert np.all(np.abs((pw.lppd + math.log(n)).cpu().numpy() - ref[0]) <= W.LSE_TOL) and np.array_equal(pw.count.cpu().numpy(), ref[3])
    y = GC.Replay(oracle_ops, tr2, data2, off2, key.impl).draws(key, x, z)
    assert isinstance(pp, PosteriorPredictive) and PR.same_bits(pp.draws["y"].cpu().numpy(), y[0].T)
    # new inputs, nothing observed: the same draws, no PIT
    with use_ops(hip_ops):
        new = alg.predictive(cols, key, args=held.args, draw_stride=1)
        assert hip_ops.jit_stats()["compiles"] == before
    assert new.pit is None and torch.equal(new.draws["y"].view(torch.int32), pp.draws["y"].view(torch.int32))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def _e2e_target(m, xs=None, g=None, ys=None):
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    xs, g, ys = (m.xs if xs is None else xs), (m.g if g is None else g), (m.ys if ys is None else ys)
    return Target(GR.body("intercept", m.G), (f(xs), torch.from_numpy(np.asarray(g, dtype=np.int64))), ChoiceMap.d({"y": f(ys)}))


def test_end_to_end(hip_ops):
    """group_ref.e2e_model() (D = 200, G = 8), n = 8192: pointwise, loo and predictive of a TemperedResult against the closed
    form, each within FOUR TIMES the spread group_checks_ref records for the float64 restatement; a held-out target against
    its own closed form; no row above the k-hat threshold."""
    m = GR.e2e_model()
    n, F = GC.E2E_N, GC.E2E_FACTOR
    hx, hg, hy = GC.held_out_rows(m)
    with use_ops(hip_ops):
        alg = TemperedSMC(_e2e_target(m), n, n_moves=2, ess_target=0.5)
        res = alg.run(genjax.random.key(2027, "philox"))
        key = genjax.random.key(9, "philox")
        pw, loo, pp = alg.pointwise(res), alg.loo(res), alg.predictive(res, key, n_draws=64)
        held = _e2e_target(m, hx, hg, hy)
        before = hip_ops.jit_stats()["compiles"]
        pw_held, pp_held = alg.pointwise(res, target=held), alg.predictive(res, key, target=held)
        assert hip_ops.jit_stats()["compiles"] == before
        # the latent columns in table order are the same call
        cols = [res.choices["mu"], res.choices["b"], res.choices["a"]]
        assert torch.equal(alg.pointwise(cols).lppd.view(torch.int64), pw.lppd.view(torch.int64))
        assert torch.equal(alg.loo(cols).elpd_loo.view(torch.int64), loo.elpd_loo.view(torch.int64))
    assert isinstance(pw, PointwiseLikelihood) and isinstance(loo, PSISLOO) and isinstance(pp, PosteriorPredictive)
    assert pw.lppd.shape == (200,) and loo.elpd_loo.shape == (200,) and pp.mean["y"].shape == (200,) and pp.draws["y"].shape == (64, 200)
    assert pw_held.lppd.shape == (120,) and loo.tail_len == S.tail_len(n) and torch.equal(loo.pointwise.lppd, pw.lppd)
    exact, exact_loo = GC.closed_form_lppd(m).sum(), GC.closed_form_loo(m).sum()
    exact_held = GC.closed_form_lppd(m, hx, hg, hy).sum()
    e_lppd, e_loo, e_held = pw.log_predictive_density - exact, loo.elpd - exact_loo, pw_held.log_predictive_density - exact_held
    mu, V = GC.closed_form(m)
    mean, var, pit = (v["y"].cpu().numpy() for v in (pp.mean, pp.var, pp.pit))
    e_mean, e_var, e_pit = float(np.max(np.abs(mean - mu) / np.sqrt(V))), float(np.max(np.abs(var / V - 1.0))), PR.kolmogorov_uniform(pit)
    mu_h, V_h = GC.closed_form(m, hx, hg)
    e_mean_h = float(np.max(np.abs(pp_held.mean["y"].cpu().numpy() - mu_h) / np.sqrt(V_h)))
    e_var_h = float(np.max(np.abs(pp_held.var["y"].cpu().numpy() / V_h - 1.0)))
    print(f"lppd {pw.log_predictive_density:.4f} against {exact:.4f} (error {e_lppd:+.4f}, bound {F * GC.SPREAD_LPPD_SUM:.4f}); "
          f"held-out {e_held:+.4f} (bound {F * GC.SPREAD_HELD_SUM:.4f}); elpd_loo {loo.elpd:.4f} against {exact_loo:.4f} (error {e_loo:+.4f}, "
          f"bound {F * GC.SPREAD_ELPD_SUM:.4f}); largest khat {float(loo.khat.max()):.3f}; p_loo {loo.p_loo:.3f}; p_waic {pw.p_waic:.3f}")
    print(f"predictive mean {e_mean:.4f} (bound {F * GC.SPREAD_MEAN:.4f}), var {e_var:.4f} (bound {F * GC.SPREAD_VAR:.4f}), pit {e_pit:.4f} "
          f"(bound {F * GC.SPREAD_PIT:.4f}); held-out mean {e_mean_h:.4f}, var {e_var_h:.4f}")
    assert abs(e_lppd) <= F * GC.SPREAD_LPPD_SUM and abs(e_held) <= F * GC.SPREAD_HELD_SUM and abs(e_loo) <= F * GC.SPREAD_ELPD_SUM
    assert e_mean <= F * GC.SPREAD_MEAN and e_var <= F * GC.SPREAD_VAR and e_pit <= F * GC.SPREAD_PIT
    # (the held-out rows: the same per-row statistics, their maximum over 120 rows instead of 200 — the recorded spreads bound it)
    assert e_mean_h <= F * GC.SPREAD_MEAN and e_var_h <= F * GC.SPREAD_VAR
    assert loo.n_high == 0 and loo.khat_threshold == 0.7 and torch.equal(loo.bad, torch.zeros_like(loo.bad))
    assert torch.equal(pp.nan_count["y"], torch.zeros_like(pp.nan_count["y"]))
