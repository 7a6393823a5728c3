"""History and trajectory trace-back on the product path: libgjx_hip.so on cuda:0 against the CPU oracle (history) and
against the numpy reference of include/gjx_paths.h written in paths_ref.py (trace-back), tolerance 0."""

import numpy as np
import pytest
import torch

import genjax
import paths_ref as P
from genjax import ChoiceMapBuilder as C, gen, normal
from genjax._amd import workloads as W
from genjax._amd.runtime import use_ops
from genjax._amd.smc_fused import BootstrapSMC, LinearGaussianSSM, SMCResult, run_with_history
from genjax.inference.smc import StateSpaceModel, Trajectories

pytestmark = pytest.mark.gpu


def _np(x):
    return x.detach().cpu().numpy()


def _same_result(g, o):
    assert torch.equal(g.step_e.cpu(), o.step_e) and torch.equal(g.step_q.cpu(), o.step_q)
    assert g.log_marginal_likelihood == o.log_marginal_likelihood
    assert torch.equal(g.ancestors.cpu(), o.ancestors)
    assert (g.resampled is None) == (o.resampled is None)
    if o.resampled is not None:
        assert torch.equal(g.resampled.cpu(), o.resampled)
    for a, b in zip(P.as_cols(g.history), P.as_cols(o.history)):
        assert a.dtype == b.dtype and torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))
    assert torch.equal(g.log_weight_history.cpu().view(torch.int32), o.log_weight_history.view(torch.int32))
    for a, b in zip(P.as_cols(g.particles), P.as_cols(o.particles)):
        assert torch.equal(a.cpu(), b)
    assert torch.equal(g.log_weights.cpu(), o.log_weights)


# ---- 1. history: HIP == oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["threefry", "philox"])
@pytest.mark.parametrize("n,ess", P.SIZES)
@pytest.mark.parametrize("kind", P.KINDS)
def test_history_matches_oracle(hip_ops, oracle_ops, kind, n, ess, impl):
    model, obs = P.model_and_obs(kind)
    key = genjax.random.key(11, impl)
    with use_ops(hip_ops):
        alg = BootstrapSMC(model, obs, n, ess_threshold=ess, record_history=True)
        g = alg.run(key)
        whole = BootstrapSMC(model, obs, n, record_ancestors=True, ess_threshold=ess).run(key)
    with use_ops(oracle_ops):
        o = BootstrapSMC(model, obs, n, ess_threshold=ess, record_history=True).run(key)
    _same_result(g, o)
    # ... and the contract with the default (whole-run, replayed graph) path on the device itself
    assert torch.equal(g.step_e, whole.step_e) and torch.equal(g.step_q, whole.step_q) and torch.equal(g.ancestors, whole.ancestors)
    assert torch.equal(g.log_weights, whole.log_weights) and g.log_marginal_likelihood == whole.log_marginal_likelihood
    for a, b in zip(P.as_cols(g.particles), P.as_cols(whole.particles)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("impl", ["threefry", "philox"])
def test_history_matches_oracle_beyond_1024_tiles(hip_ops, oracle_ops, impl):
    n, y, key = 1_100_000, W.lgssm_data(6), genjax.random.key(5, impl)  # the `prefix` route of the step
    g = run_with_history(hip_ops, LinearGaussianSSM(), y, n, key)
    o = run_with_history(oracle_ops, LinearGaussianSSM(), y, n, key)
    _same_result(g, o)


# ---- 2. / 3. the kernel against the numpy reference ----------------------------------------------------------------------
def _check(hip_ops, anc, cols, leaves, n, ordered=False, pad=0, **kw):
    """anc / cols: numpy [T, n]; runs the kernel on (optionally row-padded) device copies and compares everything asked for."""
    T = anc.shape[0]

    def dev(a):
        buf = torch.full((T, n + pad), 0x7FC00000 if a.dtype == np.float32 else -12345, dtype=torch.int32, device="cuda")
        buf[:, :n] = torch.from_numpy(a.view(np.int32)).cuda()
        return buf.view(torch.float32 if a.dtype == np.float32 else torch.int32)[:, :n]

    d_leaves = None if leaves is None else torch.from_numpy(leaves.astype(np.int32)).cuda()
    out = hip_ops.paths_trace(dev(anc), [dev(c) for c in cols], d_leaves, sums=True, unique=ordered, leaves_ordered=ordered, **kw)
    lin, paths, uniq = P.trace_ref(anc, cols, leaves, n)
    m = lin.shape[1]
    assert np.array_equal(_np(out["lineage"]), lin)
    for got, want in zip(out["paths"], paths):
        assert got.shape == (T, m) and np.array_equal(_np(got).view(np.int32), want.view(np.int32))
    if ordered:
        assert np.array_equal(_np(out["unique"]), uniq)
    # sums: the any-order bound (m - 1) u sum|x|, u = 2^-53, once for the kernel and once for numpy
    s, q = _np(out["sum"]), _np(out["sumsq"])
    for c, want in enumerate(paths):
        if want.dtype != np.float32:
            assert not s[c].any() and not q[c].any()
            continue
        x = want.astype(np.float64)
        for t in range(T):
            if not np.isfinite(x[t]).all():
                assert not np.isfinite(s[c, t])
                continue
            assert abs(s[c, t] - x[t].sum()) <= m * 2.0 ** -52 * np.abs(x[t]).sum(), (c, t)
            assert abs(q[c, t] - (x[t] * x[t]).sum()) <= m * 2.0 ** -52 * (x[t] * x[t]).sum(), (c, t)
    return out


def _random_case(rng, T, n, n_cols=1, int_col=False):
    anc = rng.integers(0, n, size=(T, n), dtype=np.int32)
    cols = [rng.standard_normal((T, n)).astype(np.float32) for _ in range(n_cols)]
    if int_col:
        cols[-1] = rng.integers(-1000, 1000, size=(T, n), dtype=np.int32)
    return anc, cols


def test_random_tables_arbitrary_leaves(hip_ops):
    rng = np.random.default_rng(0)
    for T, n, m in ((7, 5000, 5000), (5, 3001, 777), (9, 1024, 4099), (4, 10, 1), (1, 2500, 2500), (1, 300, 77), (3, 1, 5)):
        anc, cols = _random_case(rng, T, n)
        _check(hip_ops, anc, cols, rng.integers(0, n, size=m, dtype=np.int32), n)
        if m == n:
            _check(hip_ops, anc, cols, None, n)  # identity leaves (unique_out not requested: the table is not monotone)


def test_strides_larger_than_n_and_five_columns(hip_ops):
    rng = np.random.default_rng(1)
    anc, cols = _random_case(rng, 6, 3333, n_cols=5, int_col=True)
    cols[1][2, 17] = np.nan  # copied as bits; its row's sum is not finite
    cols[0][:] = (cols[0] * 1e18).astype(np.float32)  # squares near the top of the f32 range: exact in f64
    _check(hip_ops, anc, cols, rng.integers(0, 3333, size=2100, dtype=np.int32), 3333, pad=763)
    _check(hip_ops, anc, cols, None, 3333, pad=5)  # rows that are not 16-byte aligned


def test_out_of_range_indices_are_clamped(hip_ops):
    rng = np.random.default_rng(2)
    n = 2000
    anc, cols = _random_case(rng, 8, n)
    anc[rng.integers(0, 8, 400), rng.integers(0, n, 400)] = -1
    anc[rng.integers(0, 8, 400), rng.integers(0, n, 400)] = n + 7
    anc[3, :] = np.iinfo(np.int32).min
    leaves = rng.integers(0, n, size=n, dtype=np.int32)
    leaves[::7], leaves[3::11] = -1, n + 7
    out = _check(hip_ops, anc, cols, leaves, n, pad=24)
    assert int(out["lineage"].min()) >= 0 and int(out["lineage"].max()) == n - 1


def test_every_output_alone(hip_ops):
    rng = np.random.default_rng(3)
    T, n = 5, 4000
    anc = np.sort(rng.integers(0, n, size=(T, n), dtype=np.int32), axis=1)
    col = rng.standard_normal((T, n)).astype(np.float32)
    leaves = np.sort(rng.integers(0, n, size=1500, dtype=np.int32))
    lin, (paths,), uniq = P.trace_ref(anc, [col], leaves, n)
    d = lambda a: torch.from_numpy(a).cuda()
    kw = dict(lineage=False, paths=False, sums=False, unique=False, leaves_ordered=True)
    o = hip_ops.paths_trace(d(anc), [d(col)], d(leaves), **{**kw, "lineage": True})
    assert np.array_equal(_np(o["lineage"]), lin) and o["paths"] is None and o["sum"] is None and o["unique"] is None
    o = hip_ops.paths_trace(d(anc), [d(col)], d(leaves), **{**kw, "paths": True})
    assert np.array_equal(_np(o["paths"][0]), paths) and o["lineage"] is None
    o = hip_ops.paths_trace(d(anc), [], d(leaves), **{**kw, "unique": True})
    assert np.array_equal(_np(o["unique"]), uniq)
    o = hip_ops.paths_trace(d(anc), [d(col)], d(leaves), **{**kw, "sums": True})
    assert o["lineage"] is None and abs(_np(o["sum"])[0, 0] - paths[0].astype(np.float64).sum()) < 1e-6


@pytest.mark.parametrize("kind,n,ess", [("lgssm", 5000, 0.0), ("hmm16", 3000, 0.5), ("ssm2", 70_000, 0.0)])
def test_real_filter_outputs(hip_ops, kind, n, ess):
    """Tables of real filters: monotone, so the distinct count is checked too; m != n; all columns + the log-weights."""
    model, obs = P.model_and_obs(kind)
    with use_ops(hip_ops):
        r = BootstrapSMC(model, obs, n, ess_threshold=ess, record_history=True).run(genjax.random.key(2))
        anc = _np(r.ancestors)
        cols = [_np(c) for c in P.as_cols(r.history)] + [_np(r.log_weight_history)]
        for m, key in ((n, genjax.random.key(8)), (n // 3 + 1, genjax.random.key(9)), (1, genjax.random.key(10))):
            tr = r.trajectories(key, n_paths=m, with_log_weights=True)
            leaves = _np(tr.lineage[-1])
            assert np.all(np.diff(leaves) >= 0)
            lin, paths, uniq = P.trace_ref(anc, cols, leaves, n)
            assert np.array_equal(_np(tr.lineage), lin) and np.array_equal(_np(tr.unique_ancestors), uniq)
            for got, want in zip(P.as_cols(tr.paths) + [tr.log_weight_paths], paths):
                assert np.array_equal(_np(got).view(np.int32), want.view(np.int32))
        tr = r.trajectories()  # identity leaves: weighted paths
        lin, paths, uniq = P.trace_ref(anc, cols[:-1], None, n)
        assert np.array_equal(_np(tr.lineage), lin) and np.array_equal(_np(tr.unique_ancestors), uniq)
        assert torch.equal(tr.log_weights, r.log_weights) and tr.log_weight_paths is None
        with pytest.raises(ValueError, match="equally weighted"):
            tr.mean()
    _check(hip_ops, anc, cols, None, n, ordered=True)


def test_sums_are_deterministic_and_independent_of_the_grid(hip_ops):
    rng = np.random.default_rng(4)
    T, n = 12, 300_000
    anc = torch.from_numpy(np.sort(rng.integers(0, n, size=(T, n), dtype=np.int32), axis=1)).cuda()
    cols = [torch.from_numpy((rng.standard_normal((T, n)) * 10.0 ** rng.integers(-3, 4, size=(T, n))).astype(np.float32)).cuda()
            for _ in range(2)]
    leaves = torch.from_numpy(np.sort(rng.integers(0, n, size=n, dtype=np.int32))).cuda()
    run = lambda **kw: hip_ops.paths_trace(anc, cols, leaves, sums=True, unique=True, leaves_ordered=True, **kw)
    a, b, c, d = run(), run(), run(max_workgroups=7), run(max_workgroups=1)
    for o in (b, c, d):
        for k in ("sum", "sumsq", "unique", "lineage"):
            assert torch.equal(a[k].view(torch.int64) if a[k].dtype == torch.float64 else a[k], o[k].view(torch.int64) if o[k].dtype == torch.float64 else o[k]), k
        assert torch.equal(a["paths"][1], o["paths"][1])
    assert int(hip_ops.tickets()[0]) == 0  # the arrival counter is left zero


def test_full_size_once(hip_ops):
    """T = 100, n = m = 1e6: the size the feature is for."""
    T, n = 100, 1_000_000
    y = W.lgssm_data(T)
    r = run_with_history(hip_ops, LinearGaussianSSM(), y, n, genjax.random.key(1, "philox"))
    with use_ops(hip_ops):
        tr = r.trajectories(genjax.random.key(2, "philox"))
    anc, col = _np(r.ancestors), _np(r.history)
    lin, (paths,), uniq = P.trace_ref(anc, [col], _np(tr.lineage[-1]), n)
    assert np.array_equal(_np(tr.lineage), lin) and np.array_equal(_np(tr.paths).view(np.int32), paths.view(np.int32))
    assert np.array_equal(_np(tr.unique_ancestors), uniq)
    x = paths.astype(np.float64)
    assert np.all(np.abs(_np(tr._sum)[0] - x.sum(axis=1)) <= n * 2.0 ** -52 * np.abs(x).sum(axis=1))
    assert np.all(np.abs(_np(tr._sumsq)[0] - (x * x).sum(axis=1)) <= n * 2.0 ** -52 * (x * x).sum(axis=1))
    print("distinct ancestors at t = 0, 50, 99:", uniq[0], uniq[50], uniq[99])


# ---- 4. statistics -------------------------------------------------------------------------------------------------------
def test_smoothing_means_match_the_rts_smoother(hip_ops):
    y = W.lgssm_data(P.STAT_T)
    means = []
    with use_ops(hip_ops):
        alg = BootstrapSMC(LinearGaussianSSM(**W.LGSSM), y, P.STAT_N, record_history=True)
        for i in range(P.STAT_R):
            fk, lk = P.stat_keys(i)
            tr = alg.run(fk).trajectories(lk)
            means.append(tr.mean().numpy())
            u = _np(tr.unique_ancestors)
            assert u[-1] == len(np.unique(_np(tr.lineage[-1]))) and np.all(np.diff(u) >= 0)
            assert np.all(tr.var().numpy() > 0)
    z = P.check_smoothing_means(means)
    assert np.allclose(z, [-1.22, 0.85, 0.72, 0.48, 0.77, -0.95, -1.94, -0.00], atol=0.006)  # (the oracle's figures: HIP == oracle)
    assert int(u[0]) == 27787


# ---- 5. the public interface ---------------------------------------------------------------------------------------------
def test_public_api_on_the_readme_model(hip_ops):
    @gen
    def init():
        p = normal(0.0, 1.0) @ "p"
        v = normal(0.0, 0.5) @ "v"
        normal(p, 0.6) @ "y"
        return p, v

    @gen
    def step(carry):  # constant-velocity tracking: the README's `step`
        p, v = carry
        v2 = normal(0.95 * v, 0.3) @ "v"
        normal(p + 0.5 * v2, 0.6) @ "y"
        return p + 0.5 * v2, v2

    T, n = 20, 100_000
    obs = C["y"].set(torch.tensor(W.lgssm_data(T)))
    key, key2 = genjax.random.key(0), genjax.random.key(1)
    with use_ops(hip_ops):
        res = BootstrapSMC(StateSpaceModel(init, step), obs, n, record_history=True).run(key)
        assert isinstance(res, SMCResult) and len(res.history) == 2 and res.history[0].shape == (T, n)
        tr = res.trajectories(key2)
        assert isinstance(tr, Trajectories) and tr.log_weights is None and tr.log_weight_paths is None
        assert len(tr.paths) == 2 and all(p.shape == (T, n) and p.dtype == torch.float32 and p.is_contiguous() for p in tr.paths)
        assert tr.lineage.shape == (T, n) and tr.lineage.dtype == torch.int32
        assert tr.unique_ancestors.shape == (T,) and tr.unique_ancestors.dtype == torch.int64
        leaves = tr.lineage[T - 1].long()
        for k in range(2):
            assert torch.equal(tr.paths[k][T - 1], res.history[k][T - 1][leaves])
            assert torch.equal(tr.paths[k][0], res.history[k][0][tr.lineage[0].long()])
        mean, var = tr.mean(), tr.var()
        assert len(mean) == 2 and mean[0].shape == (T,) and mean[0].dtype == torch.float64 and bool((var[1] > 0).all())
        assert np.allclose(mean[0].numpy(), _np(tr.paths[0]).astype(np.float64).mean(axis=1), rtol=0, atol=1e-9)
        small = res.trajectories(key2, n_paths=1000, with_log_weights=True)
        assert small.paths[0].shape == (T, 1000) and small.log_weight_paths.shape == (T, 1000)
        plain = BootstrapSMC(StateSpaceModel(init, step), obs, n, record_ancestors=True).run(key)
        with pytest.raises(ValueError, match="record_history=True"):
            plain.trajectories(key2)
        with pytest.raises(ValueError, match="n_paths"):
            res.trajectories(n_paths=10)
