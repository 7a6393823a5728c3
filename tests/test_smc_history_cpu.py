"""`BootstrapSMC(..., record_history=True)` on the CPU oracle: the stepwise driver that places every step's population
in row t of `[T, stride]` buffers returns, bit for bit, what the whole-run call returns — plus the history."""

import numpy as np
import pytest
import torch

import genjax
import paths_ref as P
from genjax._amd import workloads as W
from genjax._amd.runtime import use_ops
from genjax._amd.smc_fused import BootstrapSMC, LinearGaussianSSM, SMCResult, run_with_history
from genjax.inference.smc import Trajectories  # noqa: F401  (re-exported)


def _eq(a, b):
    return all(torch.equal(x, y) for x, y in zip(P.as_cols(a), P.as_cols(b)))


@pytest.mark.parametrize("impl", ["threefry", "philox"])
@pytest.mark.parametrize("n,ess", P.SIZES)
@pytest.mark.parametrize("kind", P.KINDS)
def test_history_run_equals_whole_run(oracle_ops, kind, n, ess, impl):
    model, obs = P.model_and_obs(kind)
    key = genjax.random.key(11, impl)
    T = P.T_GRID
    with use_ops(oracle_ops):
        a = BootstrapSMC(model, obs, n, record_ancestors=True, ess_threshold=ess).run(key)
        b = BootstrapSMC(model, obs, n, ess_threshold=ess, record_history=True).run(key)
    assert a.history is None and a.log_weight_history is None
    # the contract: tolerance 0
    assert torch.equal(a.step_e, b.step_e) and torch.equal(a.step_q, b.step_q)
    assert a.log_marginal_likelihood == b.log_marginal_likelihood
    assert (a.resampled is None) == (b.resampled is None)
    if a.resampled is not None:
        assert torch.equal(a.resampled, b.resampled)
        assert 0 < int(b.resampled.sum()) < T - 1 or kind != "lgssm"  # (the adaptive case does both: resample and keep)
    assert torch.equal(a.ancestors, b.ancestors)
    assert _eq(a.particles, b.particles) and torch.equal(a.log_weights, b.log_weights)
    hist = P.as_cols(b.history)
    assert _eq(a.particles, tuple(h[T - 1] for h in hist)) and torch.equal(a.log_weights, b.log_weight_history[T - 1])
    # shapes, dtypes, layout
    assert len(hist) == len(P.as_cols(a.particles)) == (2 if kind == "ssm2" else 1)
    stride = oracle_ops.num_tiles(n) * oracle_ops.tile
    for h, p in zip(hist, P.as_cols(a.particles)):
        assert h.shape == (T, n) and h.dtype == p.dtype and h.stride() == (stride, 1) and h[3].is_contiguous()
    assert hist[0].dtype == (torch.int32 if kind == "hmm16" else torch.float32)
    assert b.log_weight_history.shape == (T, n) and b.log_weight_history.dtype == torch.float32
    assert b.log_weight_history.stride() == (stride, 1)
    assert b.ancestors.shape == (T, n) and b.ancestors.dtype == torch.int32
    assert torch.equal(b.ancestors[0], torch.arange(n, dtype=torch.int32))
    anc = b.ancestors.numpy()
    assert np.all(np.diff(anc, axis=1) >= 0) and anc.min() >= 0 and anc.max() < n  # monotone ancestors, every row
    assert bool(torch.isfinite(b.log_weight_history).all())
    # the function form, for drivers that hold an `ops` of their own
    if kind == "lgssm":
        c = run_with_history(oracle_ops, model, obs, n, key, ess)
        assert torch.equal(c.history, b.history) and torch.equal(c.log_weight_history, b.log_weight_history)


def test_history_is_a_consistent_genealogy(oracle_ops):
    """Non-adaptive LGSSM: history[t][j] was propagated from history[t-1][ancestors[t][j]] — the transition's noise
    (x_t - a x_parent) / q is standard normal over the population."""
    y = W.lgssm_data(6)
    with use_ops(oracle_ops):
        r = BootstrapSMC(LinearGaussianSSM(), y, 20000, record_history=True).run(genjax.random.key(3))
    h, anc = r.history.numpy().astype(np.float64), r.ancestors.numpy()
    for t in range(1, 6):
        eps = h[t] - 0.9 * h[t - 1][anc[t]]
        assert abs(eps.mean()) < 0.05 and abs(eps.std() - 1.0) < 0.05


def test_old_result_constructions_still_work():
    z = torch.zeros(3)
    r = SMCResult(0.5, z, z, z, z, None)
    assert r.history is None and r.log_weight_history is None and r.resampled is None
    r = SMCResult(0.5, z, z, z, z, None, z)
    assert r.resampled is z and r.history is None
    with pytest.raises(ValueError, match="record_history=True"):
        r.trajectories()


def test_run_many_with_history_runs_one_at_a_time(oracle_ops):
    y = W.lgssm_data(5)
    keys = [genjax.random.key(i) for i in range(3)]
    with use_ops(oracle_ops):
        alg = BootstrapSMC(LinearGaussianSSM(), y, 2000, record_history=True)
        many = alg.run_many(keys)
        for k, r in zip(keys, many):
            one = alg.run(k)
            assert r.history.shape == (5, 2000) and torch.equal(r.history, one.history)
            assert r.log_marginal_likelihood == one.log_marginal_likelihood


def test_smoothing_means_match_the_rts_smoother(oracle_ops):
    """The statistics check in its CPU form: oracle history + the numpy trace-back.  R runs of n particles; the leaves are
    systematic draws from the final weights, so the paths are equally weighted and their mean is the smoothing mean."""
    y = W.lgssm_data(P.STAT_T)
    means, uniq0 = [], None
    with use_ops(oracle_ops):
        alg = BootstrapSMC(LinearGaussianSSM(**W.LGSSM), y, P.STAT_N, record_history=True)
        for i in range(P.STAT_R):
            fk, lk = P.stat_keys(i)
            r = alg.run(fk)
            leaves, _, _ = oracle_ops.resample("systematic", lk.literal(), r.log_weights.contiguous(), P.STAT_N)
            assert bool((leaves[1:] >= leaves[:-1]).all())
            lin, (paths,), uniq = P.trace_ref(r.ancestors.numpy(), [r.history.numpy()], leaves.numpy(), P.STAT_N)
            means.append(paths.astype(np.float64).mean(axis=1))
            assert uniq[-1] == len(np.unique(leaves.numpy())) and np.all(np.diff(uniq) >= 0)
            uniq0 = int(uniq[0])
    z = P.check_smoothing_means(means)
    # bit-reproducible: the figures recorded when this check was specified
    assert np.allclose(z, [-1.22, 0.85, 0.72, 0.48, 0.77, -0.95, -1.94, -0.00], atol=0.006)
    assert uniq0 == 27787


def test_run_many_builds_the_plan_without_running_a_filter(oracle_ops):
    """`run_many` on a fresh StateSpaceModel filter: the plan comes from its builder, not from a filter that is run and
    thrown away — three keys are ONE `gjx_smc_run_plan` call (one batch), and element b still equals `run(keys[b])`."""
    model, obs = P.model_and_obs("ssm2")
    keys = [genjax.random.key(s) for s in (3, 8, 9)]
    calls, call = [], oracle_ops.lib.call
    oracle_ops.lib.call = lambda name, *a: (calls.append(name), call(name, *a))[1]
    try:
        with use_ops(oracle_ops):
            alg = BootstrapSMC(model, obs, 2000, record_ancestors=True)
            many = alg.run_many(keys)
    finally:
        del oracle_ops.lib.call
    assert calls.count("gjx_smc_run_plan") == 1 and calls.count("gjx_smc_plan_create") == 1
    with use_ops(oracle_ops):
        for k, m in zip(keys, many):
            one = alg.run(k)
            assert torch.equal(m.step_q, one.step_q) and torch.equal(m.ancestors, one.ancestors) and _eq(m.particles, one.particles)
            assert m.log_marginal_likelihood == one.log_marginal_likelihood
