"""The conditional particle filter on the product path (libgjx_hip.so on cuda:0).  The CPU oracle knows no
include/gjx_csmc.h, so a conditional run is pinned to it piece by piece, bit for bit, from the device's own previous
population: the ancestors of the free slots are the oracle's comb with n - 1 teeth, step 0 and every free slot are the
unconditional step's, the retained slot holds the retained path and the weight the oracle's log-densities give it, the
records are those of all n log-weights.  Then particle Gibbs on the device: invariance against the exact smoother at the
sizes of the float64 restatement (test_csmc_cpu.py), and a replay of single sweeps."""

import numpy as np
import pytest
import torch

import genjax
import backsim_ref as B
import csmc_ref as R
import guided_ref as G
import smc_params_ref as SP
from genjax import ChoiceMapBuilder as Cm
from genjax._amd import prng, workloads as W
from genjax._amd.runtime import use_ops
from genjax._amd.smc_plan import build_smc_plan
from genjax.inference.smc import BootstrapSMC, GuidedSMC, ParticleGibbs, StateSpaceModel

pytestmark = pytest.mark.gpu
IMPLS = ["threefry", "philox"]
T = 4
XSTAR = [0.3, -0.2, 1.1, 0.7]
# n: one free slot; the retained slot word 0 / word 2 of a second quad; last slot of a full tile; a tile holding only the
# retained particle; several tiles (wave route); more than 256 tiles; more than 1024 tiles
SHAPES = [2, 5, 7, 1024, 1025, 4099, 300 * 1024 + 1, 2 ** 20 + 1025]


def _cols(x):
    return list(x) if isinstance(x, tuple) else [x]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _host(res):
    torch.cuda.synchronize()
    return ([c.cpu() for c in _cols(res.history)], res.log_weight_history.cpu(), res.ancestors.cpu(), res.step_e.cpu(),
            res.step_q.cpu())


def _resample_key(rk, t, impl):
    return prng.PRNGKey(int(rk[t, 0]), int(rk[t, 1]), impl).literal()


def _check_generic(oracle_ops, oracle_plan, key, y, n, uncond, cond, xstar):
    """Pins 1, 2, 3, 5 and the state half of 4 for any model.  `oracle_plan`: the model's own plan on the oracle, or the
    shadow plan of a guided one; `uncond` / `cond`: the device's runs under `key`; `xstar`: the retained columns [T]."""
    uh, ulw, uanc, _, _ = _host(uncond)
    ch, clw, canc, ce, cq = _host(cond)
    Tn = len(y)
    sk, rk = W.smc_key_schedule(key, Tn)
    cfg = oracle_ops.smc_config(key.impl, n, 0, n, sk, rk, 0.0)
    ident = torch.arange(n, dtype=torch.int32)
    # 2. step 0: the free slots are the unconditional run's
    for a, b in zip(ch, uh):
        assert torch.equal(_bits(a[0, :n - 1]), _bits(b[0, :n - 1])), "step 0 states of the free slots"
    assert torch.equal(_bits(clw[0, :n - 1]), _bits(ulw[0, :n - 1])), "step 0 log-weights of the free slots"
    assert torch.equal(canc[0], ident)
    for t in range(Tn):
        # 4. the retained slot holds the retained path
        for k, col in enumerate(ch):
            assert float(col[t, n - 1]) == float(np.float32(xstar[k][t])), f"retained state, component {k}, step {t}"
        # 5. the records are those of all n log-weights
        assert (int(ce[t]), int(cq[t])) == R.records(oracle_ops, clw[t]), f"step_e / step_q at step {t}"
        if t == 0:
            continue
        kb = _resample_key(rk, t, key.impl)
        # 1. the construction, on code this change does not touch: an unconditional run's ancestors are the oracle's comb
        full, _, _ = oracle_ops.resample("systematic", kb, ulw[t - 1].contiguous(), n)
        assert torch.equal(full, uanc[t]), f"the reference construction itself is off at step {t}"
        # ... and the conditional run's free slots are the same comb with n - 1 teeth; the retained slot is forced
        free, _, _ = oracle_ops.resample("systematic", kb, clw[t - 1].contiguous(), n - 1)
        assert torch.equal(free, canc[t, :n - 1]), f"ancestors of the free slots at step {t}"
        assert int(canc[t, n - 1]) == n - 1, f"the retained slot's ancestor at step {t}"
        # 3. the free slots are propagated and weighted as the unconditional step does it
        parents = [col[t - 1][canc[t].long()] for col in ch]
        st, lw, a = R.oracle_free_step(oracle_ops, oracle_plan, cfg, t, y[t], parents, n)
        assert torch.equal(a, ident), "the oracle's comb over equal weights is not the identity"
        for k, col in enumerate(ch):
            assert torch.equal(_bits(st[k][:n - 1]), _bits(col[t, :n - 1])), f"free states, component {k}, step {t}"
        if oracle_plan.n_obs and not getattr(oracle_plan, "_shadow", False):
            assert torch.equal(_bits(lw[:n - 1]), _bits(clw[t, :n - 1])), f"free log-weights at step {t}"
    return ch, clw, canc


def _lgssm_runs(hip_ops, n, impl, seed=5):
    y = W.lgssm_data(T)
    key = genjax.random.key(seed, impl)
    model = StateSpaceModel(*B.lgssm_model())
    with use_ops(hip_ops):
        smc = BootstrapSMC(model, Cm["y"].set(torch.tensor(y)), n, record_history=True)
        uncond = smc.run(key)
        cond = smc.run(key, retained=torch.tensor(XSTAR))
    return model, y, key, uncond, cond


@pytest.fixture(scope="module")
def lgssm_oracle_plan(oracle_ops):
    with use_ops(oracle_ops):
        return build_smc_plan(StateSpaceModel(*B.lgssm_model()), [("y",)])[0]


# ---- pins 1 - 5 over the shapes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", SHAPES)
def test_conditional_lgssm_against_the_oracle(hip_ops, oracle_ops, lgssm_oracle_plan, n, impl):
    _, y, key, uncond, cond = _lgssm_runs(hip_ops, n, impl)
    ch, clw, _ = _check_generic(oracle_ops, lgssm_oracle_plan, key, y, n, uncond, cond, [XSTAR])
    # 4. the retained slot's weight: the observed site's log-density at the retained value, w = 0 + lp_y
    for t in range(T):
        x = torch.tensor([XSTAR[t]], dtype=torch.float32)
        ly = oracle_ops.logpdf("normal", 1, float(np.float32(y[t])), (G.f32(1.0) * x) + G.f32(0.0), B.R)
        want = torch.zeros(1, dtype=torch.float32) + ly
        assert torch.equal(_bits(want), _bits(clw[t, n - 1:n])), f"retained log-weight at step {t}"
    assert np.isfinite(cond.log_marginal_likelihood)
    # an ordinary SMCResult: trace-back of the retained leaf returns the retained path
    with use_ops(hip_ops):
        out = hip_ops.paths_trace(cond.ancestors, [cond.history], torch.tensor([n - 1], dtype=torch.int32, device="cuda"))
    assert torch.equal(out["paths"][0][:, 0].cpu(), torch.tensor(XSTAR)) and bool((out["lineage"].cpu() == n - 1).all())


# ---- 6. other models -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", [1025, 4099])
def test_two_component_model(hip_ops, oracle_ops, n, impl):
    y = W.lgssm_data(T)
    key = genjax.random.key(9, impl)
    model = StateSpaceModel(*B.two_component_model())
    xstar = [[0.4, 0.1, -0.3, 0.9], [0.2, -0.5, 0.25, 0.0]]
    with use_ops(hip_ops):
        smc = BootstrapSMC(model, Cm["y"].set(torch.tensor(y)), n, record_history=True)
        uncond, cond = smc.run(key), smc.run(key, retained=tuple(torch.tensor(c) for c in xstar))
    with use_ops(oracle_ops):
        plan = build_smc_plan(model, [("y",)])[0]
    _, clw, _ = _check_generic(oracle_ops, plan, key, y, n, uncond, cond, xstar)
    for t in range(T):  # y ~ normal(p, 0.6): w = 0 + lp_y at the retained p
        p = torch.tensor([xstar[0][t]], dtype=torch.float32)
        ly = oracle_ops.logpdf("normal", 1, float(np.float32(y[t])), (G.f32(1.0) * p) + G.f32(0.0), 0.6)
        assert torch.equal(_bits(torch.zeros(1) + ly), _bits(clw[t, n - 1:n])), f"retained log-weight at step {t}"


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", [1025, 4099])
def test_guided_model(hip_ops, oracle_ops, n, impl):
    r = 0.05
    y, _ = G.lgssm_setting(r, T)
    tq, sq, co = G.lgssm_optimal(r)
    key = genjax.random.key(7, impl)
    xstar = [float(v) for v in np.asarray(y, dtype=np.float32) + np.float32(0.01)]  # (near the sharp observations: finite weights)
    with use_ops(hip_ops):
        smc = GuidedSMC(StateSpaceModel(*G.lgssm_model(r)), Cm["y"].set(torch.tensor(y)), n, step_proposal=tq, init_proposal=sq,
                        record_history=True)
        uncond, cond = smc.run(key), smc.run(key, retained=torch.tensor(xstar))
    shadow = G.shadow_plan(oracle_ops, smc._plan[0])
    shadow._shadow = True  # (its sites are all latent: the oracle's weights are not the guided ones)
    ch, clw, canc = _check_generic(oracle_ops, shadow, key, y, n, uncond, cond, [xstar])
    # every slot's weight — the retained one's at the retained values: (0 + (lp - lq)) + lp_y by the oracle's log-densities
    for t in range(T):
        x_prev = ch[0][t - 1][canc[t].long()].contiguous() if t else None
        want = G.lgssm_log_weights(oracle_ops, co, t, y[t], ch[0][t].contiguous(), x_prev)
        assert torch.equal(_bits(want), _bits(clw[t])), f"guided log-weights at step {t}"
        assert bool(torch.isfinite(clw[t, n - 1]))


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", [1025, 4099])
def test_categorical_latent_model(hip_ops, oracle_ops, n, impl):
    trans, emit = B.hmm_tables()
    xs = torch.tensor([1, 2, 0, 5, 3, 3, 7, 4][:T], dtype=torch.int32)
    obs = Cm["x"].set(xs)
    key = genjax.random.key(11, impl)
    xstar = [[1.0, 3.0, 0.0, 6.0]]
    with use_ops(hip_ops):
        smc = BootstrapSMC(StateSpaceModel(*B.hmm_model(trans.cuda(), emit.cuda())), obs, n, record_history=True)
        uncond, cond = smc.run(key), smc.run(key, retained=torch.tensor(xstar[0]))
    with use_ops(oracle_ops):
        plan = build_smc_plan(StateSpaceModel(*B.hmm_model(trans, emit)), [("x",)])[0]
    ch, clw, _ = _check_generic(oracle_ops, plan, key, xs.numpy(), n, uncond, cond, xstar)
    le = torch.log_softmax(emit.double(), 1)
    for t in range(T):  # the weight depends on (z_t, x_t) alone: a free slot in the same state has the same bits
        same = (ch[0][t, :n - 1] == xstar[0][t]).nonzero()
        assert same.numel() > 0
        assert torch.equal(_bits(clw[t, n - 1:n]), _bits(clw[t, int(same[0]):int(same[0]) + 1])), f"retained log-weight at step {t}"
        assert abs(float(clw[t, n - 1]) - float(le[int(xstar[0][t]), int(xs[t])])) < 1e-5


# ---- 7. parameterised ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
def test_parameterised_run_equals_the_literal_model(hip_ops, impl):
    n, theta = 4099, (0.7, 0.9, 0.45)
    obs, key, path = SP.observations(T), genjax.random.key(13, impl), torch.tensor(XSTAR)
    with use_ops(hip_ops):
        par = BootstrapSMC(SP.lgssm_param_model(), obs, n, record_history=True, params=(0.1, 2.0, 3.0))
        got = par.run(key, params=theta, retained=path)
        ref = BootstrapSMC(SP.lgssm_literal_model(theta), obs, n, record_history=True).run(key, retained=path)
        plain = par.run(key, params=theta)
    torch.cuda.synchronize()
    for a, b in ((got.history, ref.history), (got.log_weight_history, ref.log_weight_history), (got.ancestors, ref.ancestors),
                 (got.step_e, ref.step_e), (got.step_q, ref.step_q)):
        assert torch.equal(a, b)
    assert got.log_marginal_likelihood == ref.log_marginal_likelihood
    assert not torch.equal(got.ancestors, plain.ancestors) and float(got.history[2, n - 1]) == float(np.float32(XSTAR[2]))


# ---- 8. zero mass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", [7, 1025])
def test_zero_total_mass(hip_ops, n, impl):
    y = np.asarray(W.lgssm_data(T), dtype=np.float32).copy()
    y[1] = 1e30  # an impossible observation: every log-weight of step 1 is -inf, so step 2 resamples from no mass at all
    with use_ops(hip_ops):
        smc = BootstrapSMC(StateSpaceModel(*B.lgssm_model()), Cm["y"].set(torch.tensor(y)), n, record_history=True)
        cond = smc.run(genjax.random.key(3, impl), retained=torch.tensor(XSTAR))
    torch.cuda.synchronize()
    lw, anc, hist = cond.log_weight_history.cpu(), cond.ancestors.cpu(), cond.history.cpu()
    assert bool((lw[1] == -float("inf")).all())
    want = torch.floor(torch.arange(n - 1, dtype=torch.float64) * (n / (n - 1))).to(torch.int32)
    assert torch.equal(anc[2, :n - 1], want) and int(anc[2, n - 1]) == n - 1
    assert [float(hist[t, n - 1]) for t in range(T)] == [float(np.float32(v)) for v in XSTAR]
    assert bool(torch.isfinite(lw[2]).all()) and bool(torch.isfinite(lw[3]).all())


# ---- particle Gibbs on the device --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth():
    return R.lgssm_truth(R.T_INV)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("refresh", ["trace", "backward"])
def test_particle_gibbs_leaves_the_smoothing_distribution_invariant(hip_ops, truth, refresh, impl):
    """The criterion and the cap of the float64 restatement, at its sizes, on the device."""
    y, mean, var = truth
    paths = np.empty((R.SWEEPS, R.CHAINS, R.T_INV))
    with use_ops(hip_ops):
        smc = BootstrapSMC(StateSpaceModel(*B.lgssm_model()), Cm["y"].set(torch.tensor(y)), R.N_INV, record_history=True)
        pg = ParticleGibbs(smc, refresh=refresh)
        root = genjax.random.key(2024, impl)
        for c in range(R.CHAINS):
            paths[:, c, :] = pg.run(prng.fold_in(root, c), R.SWEEPS).paths.double().cpu().numpy()
    R.assert_invariant(paths, mean, var, f"device, {impl}, refresh={refresh}")


@pytest.mark.parametrize("impl", IMPLS)
def test_a_run_replays_sweep_by_sweep(hip_ops, impl):
    y = W.lgssm_data(T)
    n, key = 8, genjax.random.key(77, impl)
    with use_ops(hip_ops):
        smc = BootstrapSMC(StateSpaceModel(*B.lgssm_model()), Cm["y"].set(torch.tensor(y)), n, record_history=True)
        paths = ParticleGibbs(smc, refresh="trace").run(key, 4).paths
        assert paths.shape == (4, T)
        prev = None
        for s in range(4):
            k_s = prng.fold_in(key, s)
            res = smc.run(prng.fold_in(k_s, 0), retained=prev)  # (sweep 0: no path yet, an unconditional run)
            leaf = hip_ops.categorical_index(prng.fold_in(k_s, 1).literal(), res.log_weights.contiguous())
            new = hip_ops.paths_trace(res.ancestors, [res.history], leaf.to(torch.int32))["paths"][0][:, 0]
            assert torch.equal(new, paths[s]), f"sweep {s}"
            prev = new.contiguous()
        # a given first path: sweep 0 is conditional on it
        given = ParticleGibbs(smc, refresh="trace").run(key, 1, init=torch.tensor(XSTAR)).paths
        res = smc.run(prng.fold_in(prng.fold_in(key, 0), 0), retained=torch.tensor(XSTAR))
        leaf = hip_ops.categorical_index(prng.fold_in(prng.fold_in(key, 0), 1).literal(), res.log_weights.contiguous())
        assert torch.equal(hip_ops.paths_trace(res.ancestors, [res.history], leaf.to(torch.int32))["paths"][0][:, 0], given[0])
        # the backward refresh under its own key
        back = ParticleGibbs(smc, refresh="backward").run(key, 2).paths
        k_1 = prng.fold_in(key, 1)
        res = smc.run(prng.fold_in(k_1, 0), retained=back[0])
        assert torch.equal(smc.backward_simulate(res, prng.fold_in(k_1, 2), 1).paths[:, 0], back[1])
    torch.cuda.synchronize()


@pytest.mark.parametrize("impl", IMPLS)
def test_parameter_updates_travel_with_the_sweeps(hip_ops, impl):
    y = W.lgssm_data(T)
    seen = []

    def update(key, path, theta):
        seen.append((key.words(), tuple(path.shape), theta.copy()))
        return theta * np.asarray([0.5, 1.0, 1.0])

    with use_ops(hip_ops):
        smc = BootstrapSMC(SP.lgssm_param_model(), Cm["y"].set(torch.tensor(y)), 8, record_history=True, params=(0.8, 1.0, 0.5))
        out = ParticleGibbs(smc, param_update=update).run(genjax.random.key(5, impl), 3)
        assert out.paths.shape == (3, T) and out.thetas.shape == (3, 3)
        assert np.allclose(out.thetas[:, 0], [0.4, 0.2, 0.1]) and [s[1] for s in seen] == [(T,)] * 3
        assert seen[1][0] == prng.fold_in(prng.fold_in(genjax.random.key(5, impl), 1), 3).words()
        # sweep 2 ran at the row sweep 1's update returned
        k_2 = prng.fold_in(genjax.random.key(5, impl), 2)
        res = smc.run(prng.fold_in(k_2, 0), params=out.thetas[1], retained=out.paths[1])
        leaf = hip_ops.categorical_index(prng.fold_in(k_2, 1).literal(), res.log_weights.contiguous())
        assert torch.equal(hip_ops.paths_trace(res.ancestors, [res.history], leaf.to(torch.int32))["paths"][0][:, 0], out.paths[2])
    torch.cuda.synchronize()
