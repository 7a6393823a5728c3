"""Parameterised state-space models on the GPU (include/gjx_smc_params.h): a bank of filters, one theta row each, per launch.
The reference of every parity test is the project's unchanged path — the same model with theta_f written as Python
literals, run by the CPU oracle (plain gjx_smc_plan_create) under the same key — at tolerance 0 (smc_params_ref.py).
Shapes: the tile is 1024 slots; n = 1000 is one partial tile, n = 2500 three tiles with a partial last."""

import math

import numpy as np
import pytest
import torch

import genjax
import guided_ref as G
import smc_params_ref as R
from genjax import gen, normal
from genjax._amd import prng, workloads as W
from genjax._amd.runtime import use_ops
from genjax._amd.smc_fused import _result
from genjax.inference.smc import BootstrapSMC, GuidedSMC, ParticleMH, StateSpaceModel

pytestmark = pytest.mark.gpu
IMPLS = ["threefry", "philox"]
T = 6
_REFS: dict = {}


def _ref(oracle_ops, name, theta, n, key, ess, history=False):
    """The oracle's literal-theta run, computed once per (model, theta, n, key, threshold) and shared."""
    k = (name, tuple(R.f32s(theta)), n, key, ess, history)
    if k not in _REFS:
        _REFS[k] = R.oracle_run(oracle_ops, R.MODELS[name][1](theta), R.observations(T), n, key, ess, history)
    return _REFS[k]


# ---- 1. a bank of F filters = F literal models ------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("ess", [0.0, 0.5])
@pytest.mark.parametrize("n", [1000, 2500])
@pytest.mark.parametrize("name", list(R.MODELS))
def test_bank_equals_literals(hip_ops, oracle_ops, name, n, ess, impl):
    make, _, rows = R.MODELS[name]
    with use_ops(hip_ops):
        smc = BootstrapSMC(make(), R.observations(T), n, record_ancestors=True, ess_threshold=ess)
        for F in (1, 3, 16):
            th, keys = rows(F), R.keys_for(impl, F)
            bank = smc.run_many(keys, params=th)
            torch.cuda.synchronize()
            assert len(bank) == F
            for f in range(F):
                R.assert_same_run(bank[f], _ref(oracle_ops, name, th[f], n, keys[f], ess), f"{name} F={F} filter {f}")
            for f in range(1, F):  # no two filters share an output: a bank that read row 0 everywhere cannot pass
                R.assert_runs_differ(bank[f], bank[f - 1], f"{name} F={F} filters {f - 1}, {f}")
                R.assert_runs_differ(bank[f], bank[0], f"{name} F={F} filters 0, {f}")


# ---- 2. one row for every filter; a single run is an element of the bank ----------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", list(R.MODELS))
def test_one_row_for_all_filters_and_single_runs(hip_ops, oracle_ops, name, impl):
    make, _, rows = R.MODELS[name]
    n, ess, F = 2500, 0.5, 3
    th, keys = rows(4), R.keys_for(impl, F)
    with use_ops(hip_ops):
        smc = BootstrapSMC(make(), R.observations(T), n, record_ancestors=True, ess_threshold=ess, params=th[3])
        shared = smc.run_many(keys, params=th[1])  # n_rows == 1
        default = smc.run_many(keys)               # the filter's default row
        bank = smc.run_many(keys, params=th[:F])
        singles = [smc.run(keys[f], params=th[f]) for f in range(F)]
        torch.cuda.synchronize()
    for f in range(F):
        R.assert_same_run(shared[f], _ref(oracle_ops, name, th[1], n, keys[f], ess), f"{name} shared row, filter {f}")
        R.assert_same_run(default[f], _ref(oracle_ops, name, th[3], n, keys[f], ess), f"{name} default row, filter {f}")
        R.assert_same_run(singles[f], bank[f], f"{name} run() against bank element {f}")
        R.assert_same_run(singles[f], _ref(oracle_ops, name, th[f], n, keys[f], ess), f"{name} run(), filter {f}")
    assert smc.log_marginal_likelihoods(keys, th[:F]).tolist() == [b.log_marginal_likelihood for b in bank]


# ---- 3. no recompilation, no stale values ---------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
def test_new_theta_compiles_nothing_and_back_to_back_runs_keep_their_rows(hip_ops, oracle_ops, impl):
    name, n = "lgssm", 2500
    make, _, rows = R.MODELS[name]
    th = rows(8)
    key = prng.key(5, impl)
    with use_ops(hip_ops):
        smc = BootstrapSMC(make(), R.observations(T), n, record_ancestors=True)
        smc.run(key, params=th[0])  # warm-up: the one compilation
        torch.cuda.synchronize()
        before = hip_ops.jit_stats()
        runs = [smc.run(key, params=th[1 + k]) for k in range(5)]
        torch.cuda.synchronize()
        after = hip_ops.jit_stats()
        assert after["compiles"] == before["compiles"], (before, after)
        for k in range(5):
            R.assert_same_run(runs[k], _ref(oracle_ops, name, th[1 + k], n, key, 0.0), f"theta {1 + k}")
        # two runs with different rows, issued back to back with no synchronisation between them, outputs in separate buffers
        model = smc._bind(hip_ops, th[0])
        sk, rk = W.smc_key_schedule(key, model.T)
        torch.cuda.synchronize()
        smc._set_rows(model, th[6:7])
        out_a = hip_ops._smc_run(model, key.impl, n, sk, rk, True, 0.0)
        smc._set_rows(model, th[7:8])
        out_b = hip_ops._smc_run(model, key.impl, n, sk, rk, True, 0.0)
        torch.cuda.synchronize()
        res_a, res_b = _result(hip_ops, n, out_a), _result(hip_ops, n, out_b)
    R.assert_same_run(res_a, _ref(oracle_ops, name, th[6], n, key, 0.0), "first of two back-to-back runs")
    R.assert_same_run(res_b, _ref(oracle_ops, name, th[7], n, key, 0.0), "second of two back-to-back runs")
    R.assert_runs_differ(res_a, res_b, "back-to-back runs")


# ---- 4. guided: a proposal that reads y and theta ----------------------------------------------------------------------------
def _guided_models(co):
    """The LGSSM (a, q literal; r a parameter) with proposals whose coefficients are parameters, and the same with every
    number a literal."""
    r, c1, c2, s, k0, s0 = (co[k] for k in ("r", "c1", "c2", "s", "k0", "s0"))

    @gen
    def init_p(theta):
        x = normal(0.0, 1.0) @ "x"
        normal(x, theta[0]) @ "y"
        return x

    @gen
    def step_p(x, theta):
        x2 = normal(G.A * x, G.Q) @ "x"
        normal(x2, theta[0]) @ "y"
        return x2

    @gen
    def track_p(carry, y, theta):
        normal(theta[1] * carry + theta[2] * y, theta[3]) @ "x"

    @gen
    def start_p(y, theta):
        normal(theta[4] * y, theta[5]) @ "x"

    @gen
    def track_l(carry, y):
        normal(c1 * carry + c2 * y, s) @ "x"

    @gen
    def start_l(y):
        normal(k0 * y, s0) @ "x"

    names = ("r", "c1", "c2", "s", "k0", "s0")
    return (StateSpaceModel(init_p, step_p, params=names), track_p, start_p,
            StateSpaceModel(*G.lgssm_model(r)), track_l, start_l)


@pytest.mark.parametrize("impl", IMPLS)
def test_guided_with_parameters_against_the_two_references(hip_ops, oracle_ops, impl):
    r, n, Tg = 0.05, 2500, T
    y, _ = G.lgssm_setting(r, Tg)
    co = {k: float(np.float32(v)) for k, v in G.lgssm_optimal(r)[2].items()}  # theta as the filter runs it: f32
    theta = [co[k] for k in ("r", "c1", "c2", "s", "k0", "s0")]
    pm, track_p, start_p, lm, track_l, start_l = _guided_models(co)
    key = genjax.random.key(7, impl)
    obs = R.C["y"].set(torch.tensor(y))
    with use_ops(hip_ops):
        alg = GuidedSMC(pm, obs, n, step_proposal=track_p, init_proposal=start_p, record_history=True, params=theta)
        res = alg.run(key)
        literal = GuidedSMC(lm, obs, n, step_proposal=track_l, init_proposal=start_l)
        literal_plan = literal._bind(hip_ops).plan  # (built, never run: the shadow's tables come from it)
    torch.cuda.synchronize()
    hist, lw, anc = res.history.cpu(), res.log_weight_history.cpu(), res.ancestors.cpu()
    assert bool(torch.isfinite(lw).all()) and math.isfinite(res.log_marginal_likelihood)
    shadow = G.shadow_plan(oracle_ops, literal_plan)
    sk, rk = W.smc_key_schedule(key, Tg)
    cfg = oracle_ops.smc_config(key.impl, n, 0, n, sk, rk, 0.0)
    for t in range(Tg):
        st, a = G.oracle_step_from(oracle_ops, shadow, cfg, t, y[t], [hist[t - 1]] if t else None, lw[t - 1] if t else None, n)
        assert torch.equal(a, anc[t]), f"(a) ancestors, step {t}"
        assert torch.equal(st[0].view(torch.int32), hist[t].contiguous().view(torch.int32)), f"(a) states, step {t}"
        x_prev = hist[t - 1][anc[t].long()].contiguous() if t else None
        want = G.lgssm_log_weights(oracle_ops, co, t, y[t], hist[t].contiguous(), x_prev)
        assert torch.equal(want.view(torch.int32), lw[t].contiguous().view(torch.int32)), f"(b) log-weights, step {t}"


# ---- 5. recorded history -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", list(R.MODELS))
def test_record_history_equals_the_whole_run_call(hip_ops, oracle_ops, name, impl):
    make, _, rows = R.MODELS[name]
    n, ess = 2500, 0.5
    th, key = rows(3)[2], prng.key(9, impl)
    with use_ops(hip_ops):
        whole = BootstrapSMC(make(), R.observations(T), n, record_ancestors=True, ess_threshold=ess).run(key, params=th)
        hist = BootstrapSMC(make(), R.observations(T), n, ess_threshold=ess, record_history=True, params=rows(3)[0])
        stepped = hist.run(key, params=th)
        again = hist.run_many([key, key], params=rows(3)[1:])[1]  # (one filter at a time, each with its row)
        torch.cuda.synchronize()
    R.assert_same_run(stepped, whole, f"{name}: stepwise against whole-run")
    R.assert_same_run(again, whole, f"{name}: run_many of a history filter")
    R.assert_same_run(stepped, _ref(oracle_ops, name, th, n, key, ess), f"{name}: stepwise against the oracle")
    cols = R.columns(stepped.history)
    assert all(c.shape == (T, n) for c in cols) and stepped.log_weight_history.shape == (T, n)
    for c, p in zip(cols, R.columns(stepped.particles)):
        assert torch.equal(c[T - 1], p)


# ---- 6. beyond the LDS route -------------------------------------------------------------------------------------------------
def test_a_population_beyond_the_lds_route(hip_ops, oracle_ops):
    n, Tb = (1 << 20) + 1024, 3  # 1025 tiles: the grouped tile-prefix route
    th, key = R.lgssm_rows(2)[1], prng.key(21, "philox")
    obs = R.C["y"].set(torch.as_tensor(W.lgssm_data(Tb), dtype=torch.float32))
    with use_ops(hip_ops):
        got = BootstrapSMC(R.lgssm_param_model(), obs, n, record_ancestors=True).run(key, params=th)
        torch.cuda.synchronize()
    ref = R.oracle_run(oracle_ops, R.lgssm_literal_model(th), obs, n, key)
    R.assert_same_run(got, ref, "n = 2^20 + 1024")


# ---- 7. PMMH, replayed ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
def test_particle_mh_replay(hip_ops, impl):
    Cn, iters, n, scale = 4, 6, 1000, np.asarray([0.05, 0.08, 0.04])
    theta0 = np.asarray([0.6, 0.9, 0.5], dtype=np.float32)

    def log_prior(th):  # a box: some proposals of the walk fall outside
        return 0.0 if (0.45 < th[0] < 0.75 and 0.7 < th[1] < 1.1 and 0.4 < th[2] < 0.6) else -math.inf

    key = prng.key(13, impl)
    with use_ops(hip_ops):
        smc = BootstrapSMC(R.lgssm_param_model(), R.observations(T), n)
        samples, lls, acc = ParticleMH(smc, log_prior, scale, n_chains=Cn).run(key, theta0, iters)
        # the specification, one filter run per chain and iteration
        rng = np.random.default_rng([key.k0, key.k1])

        def ll_of(i, c, th):
            return smc.run(prng.fold_in(prng.fold_in(key, i), c), params=th).log_marginal_likelihood

        theta = np.tile(theta0, (Cn, 1))
        ll = np.asarray([ll_of(0, c, theta[c]) for c in range(Cn)])
        lp = np.asarray([log_prior(theta[c]) for c in range(Cn)])
        want_s, want_l, want_a = [theta.astype(np.float64)], [ll.copy()], []
        for i in range(1, iters + 1):
            z = rng.standard_normal((Cn, 3))
            u = rng.random(Cn)
            prop = (theta.astype(np.float64) + scale * z).astype(np.float32)
            a = np.zeros(Cn, dtype=bool)
            for c in range(Cn):
                lp_new = log_prior(prop[c])
                ll_new = ll_of(i, c, prop[c] if lp_new > -math.inf else theta[c])
                if lp_new > -math.inf and math.log(u[c]) < (ll_new + lp_new) - (ll[c] + lp[c]):
                    a[c], theta[c], ll[c], lp[c] = True, prop[c], ll_new, lp_new
            want_s.append(theta.astype(np.float64))
            want_l.append(ll.copy())
            want_a.append(a)
    assert np.array_equal(samples, np.stack(want_s)) and np.array_equal(lls, np.stack(want_l))
    assert np.array_equal(acc, np.stack(want_a))
    assert 0 < acc.sum() < acc.size  # (both branches of the test were taken)


# ---- 8. PMMH is right in distribution ------------------------------------------------------------------------------------------
def test_particle_mh_posterior_mean(hip_ops):
    """|mean over chains - exact| <= 5 sd(chain means) / sqrt(8).  Plain MH with the exact likelihood meets this on 20 of 20
    seeds on the CPU (|z| <= 1.9), and with likelihood noise of sd 0.3 and 1.0 as well; exact posterior mean 0.4729, sd 0.161."""
    y = W.lgssm_data(50)
    exact = R.exact_posterior_mean_a(y)
    obs = R.C["y"].set(torch.as_tensor(y, dtype=torch.float32))
    with use_ops(hip_ops):
        smc = BootstrapSMC(R.lgssm_a_model(), obs, 4096)
        samples, lls, acc = ParticleMH(smc, R.uniform_log_prior, 0.15, n_chains=8).run(prng.key(2024, "philox"), [0.5], 400)
    err, bound = R.chains_criterion(samples, exact, burn=100)
    print(f"exact {exact:.4f}; chain means {samples[101:, :, 0].mean(axis=0).round(4).tolist()}; |mean - exact| = {err:.4f}, "
          f"bound {bound:.4f}; acceptance {acc.mean():.3f}")
    assert np.all(np.isfinite(lls)) and err <= bound
