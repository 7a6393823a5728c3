"""Pointwise predictive densities on the GPU (include/gjx_pointwise.h): the four outputs per row held to float64 numpy
reductions of the bit-exact f32 terms tests/plate_ref.py replays from unchanged oracle entry points, NaN and -inf terms,
held-out rows through a second Target without a second compilation, the closed form of the conjugate regression, and the
public call end to end in two kernel launches."""

import math

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import pointwise_ref as W
from genjax import ChoiceMap, Target
from genjax._amd import temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PointwiseLikelihood, TemperedSMC
from test_gpu_guided import _kernel_nodes

pytestmark = pytest.mark.gpu

NS = (1, 257, 1000)           # one particle; two chunks with a four-block remainder; several chunks
DS = (1, 63, 64, 65, 257, 513)  # a lone row, a wave's edge, a tile's edge, three tiles


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


def _f32(t):
    return t.detach().to(torch.float32).numpy().copy()


@pytest.fixture(scope="module")
def lowered(hip_ops):
    """Per model: (tracer, plan) lowered once, from 20 rows — the plan knows no length: data of any D is set per case."""
    out = {}
    with use_ops(hip_ops):
        for name in P.MODELS:
            target, _ = P.target(name, 20)
            tracer = temper.lower(target, 64)
            plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            if tracer.params:
                plan.set_params(tracer.params)
            out[name] = (tracer, plan)
    return out


def _case(lowered, oracle_ops, name, D, inf_row=False):
    tracer, plan = lowered[name]
    _, data = P.target(name, max(D, 2), seed=1)
    data = [_f32(t)[:D] for t in data]
    if inf_row:
        data[-1][D // 2] = np.inf
    plan.set_data(_dev(data))
    return plan, P.Assess(oracle_ops, tracer, data)


def _check(got, t, case, rows=None):
    """got float64 [4, D] against the float64 reductions of the terms t [D, n], at the tolerances of pointwise_ref."""
    ref = W.reduce64(t)
    b1, b2 = W.moment_bounds(t)
    rows = np.arange(t.shape[0]) if rows is None else rows
    assert W.spread(t)[rows].max() < W.LSE_MAX_SPREAD, case  # (the lse tolerance is derived for such rows)
    with np.errstate(invalid="ignore"):  # (rows left out of `rows` may hold infinities)
        e0 = np.abs(got[0] - ref[0])[rows]
        e1, e2 = np.abs(got[1] - ref[1])[rows], np.abs(got[2] - ref[2])[rows]
    print(case, f"lse err {e0.max():.3g} (tol {W.LSE_TOL}); s1 err / bound {np.max(e1 / b1[rows]):.3g}; s2 err / bound {np.max(e2 / b2[rows]):.3g}")
    assert np.all(e0 <= W.LSE_TOL), case
    assert np.all(e1 <= b1[rows]) and np.all(e2 <= b2[rows]), case
    assert np.array_equal(got[3][rows], ref[3][rows]), case


@pytest.mark.parametrize("name", P.MODELS)
def test_pointwise_pin(hip_ops, oracle_ops, lowered, name):
    rng = np.random.default_rng(21)
    chunks = set()
    for D in DS:
        plan, assess = _case(lowered, oracle_ops, name, D)
        for n in NS:
            cols = W.centred_columns(name, n, rng)
            t = W.terms(assess, cols)
            assert t.shape == (D, n) and np.isfinite(t).all()
            dev = _dev(cols)
            out = hip_ops.temper_pointwise(plan, dev)
            again = hip_ops.temper_pointwise(plan, dev)
            assert out.shape == (4, D) and out.dtype == torch.float64 and out.is_cuda
            assert torch.equal(out, again), (name, D, n)
            _check(out.cpu().numpy(), t, (name, D, n))
            chunks.add(int(hip_ops.lib.call("gjx_pointwise_chunks", n, D)))
    assert chunks == {1, 2, 4}  # one chunk, two, several


def test_pointwise_edges(hip_ops, oracle_ops, lowered):
    n = 1000
    rng = np.random.default_rng(22)
    # NaN terms: every fourth particle's Gamma latent lies outside its support (negative, zero, NaN, tiny negative scale)
    plan, assess = _case(lowered, oracle_ops, "hetero", 65)
    cols = P.columns("hetero", n, rng, outside=True)
    t = W.terms(assess, cols)
    bad = np.isnan(t)
    assert bad.any(axis=1).all() and np.array_equal(bad.any(axis=0), np.arange(n) % 4 == 0)  # every fourth particle
    got = hip_ops.temper_pointwise(plan, _dev(cols)).cpu().numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
    live = np.where(t > -np.inf, t, -np.inf)  # (false on NaN: those entries leave)
    ref = W.reduce64(live)
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[3], n - (bad | np.isneginf(t)).sum(axis=1))
    print("NaN terms per row", bad.sum(axis=1).min(), "..", bad.sum(axis=1).max(), "; largest spread of the rest", W.spread(t).max(),
          "; lse err", np.abs(got[0] - ref[0]).max())
    assert np.isfinite(ref[0]).all() and np.all(np.abs(got[0] - ref[0]) <= W.LSE_TOL)
    # one +inf observed value: that row's terms are all -inf
    plan, assess = _case(lowered, oracle_ops, "hetero", 65, inf_row=True)
    cols = W.centred_columns("hetero", n, rng)
    t = W.terms(assess, cols)
    r = 65 // 2
    assert np.isneginf(t[r]).all() and np.isfinite(np.delete(t, r, axis=0)).all()
    got = hip_ops.temper_pointwise(plan, _dev(cols)).cpu().numpy()
    assert got[0][r] == -np.inf and got[3][r] == 0.0 and got[1][r] == -np.inf and got[2][r] == np.inf
    _check(got, t, ("hetero", "inf_row"), rows=np.delete(np.arange(65), r))


def test_held_out(hip_ops, oracle_ops):
    """Columns and a second Target of 65 other rows: the result is the reference's on those rows, and the kernel comes out of
    the JIT cache."""
    n = 1000
    cols = W.centred_columns("normal", n, np.random.default_rng(23))
    with use_ops(hip_ops):
        train, _ = P.target("normal", 40, seed=2)
        alg = TemperedSMC(train, n)
        first = alg.pointwise(_dev(cols))
        assert first.lppd.shape == (40,)
        before = hip_ops.jit_stats()["compiles"]
        held, data = P.target("normal", 65, seed=7)
        pw = alg.pointwise(_dev(cols), target=held)
        assert hip_ops.jit_stats()["compiles"] == before
        tracer = temper.lower(held, 64)
    assert isinstance(pw, PointwiseLikelihood) and pw.lppd.shape == (65,) and pw.n == n
    t = W.terms(P.Assess(oracle_ops, tracer, [_f32(c) for c in data]), cols)
    got = np.stack([(pw.lppd + math.log(n)).cpu().numpy(), (pw.mean * n).cpu().numpy(), np.zeros(65), pw.count.cpu().numpy()])
    ref = W.reduce64(t)
    b1, _ = W.moment_bounds(t)
    assert W.spread(t).max() < W.LSE_MAX_SPREAD
    assert np.all(np.abs(got[0] - ref[0]) <= W.LSE_TOL) and np.all(np.abs(got[1] - ref[1]) <= b1 + np.abs(ref[1]) * 2.0 ** -51)
    assert np.array_equal(got[3], ref[3])
    var = t.astype(np.float64).var(axis=1, ddof=1)
    assert np.allclose(pw.var.cpu().numpy(), var, rtol=1e-9, atol=0)
    assert not torch.equal(first.lppd[:40], pw.lppd[:40])


def test_closed_form(hip_ops):
    """n = 8192 columns from the exact posterior of the conjugate regression with 500 rows: sum_d lppd_d within FOUR TIMES
    the spread pointwise_ref records of sum_d log N(y_d; x_d' mu, noise^2 + x_d' Sigma x_d); p_waic within the same relative
    margin of its float64 numpy value on the same columns."""
    model = P.conjugate(500)
    n = 8192
    cols = W.posterior_columns(model, n, 7000)
    xs, ys = torch.tensor(model.xs, dtype=torch.float32), torch.tensor(model.ys, dtype=torch.float32)
    target = Target(P.bodies()["normal"], (xs, model.noise), ChoiceMap.d({"y": ys}))
    with use_ops(hip_ops):
        pw = TemperedSMC(target, n).pointwise(_dev(cols))
    exact = W.closed_form_lppd(model).sum()
    bound = W.CLOSED_FORM_FACTOR * W.SPREAD_LPPD_SUM
    p_ref = W.terms_f64(model, cols).var(axis=1, ddof=1).sum()
    rel = bound / abs(exact)
    print(f"sum lppd {pw.log_predictive_density:.6f} against {exact:.6f} (error {pw.log_predictive_density - exact:+.6f}, bound {bound:.6f}); "
          f"p_waic {pw.p_waic:.8f} against {p_ref:.8f} (relative error {(pw.p_waic - p_ref) / p_ref:+.3g}, margin {rel:.3g})")
    assert abs(pw.log_predictive_density - exact) <= bound
    assert abs(pw.p_waic - p_ref) <= rel * abs(p_ref)
    assert torch.equal(pw.count, torch.full((500,), float(n), dtype=torch.float64, device=pw.count.device))


def test_end_to_end_api(hip_ops):
    """TemperedSMC over the plated regression, then pointwise(res): [D] fields, a finite WAIC that is -2 sum (lppd - var) of
    its own fields, and exactly two kernel nodes per call."""
    D, n = 100, 4096
    target, _ = P.target("normal", D, seed=3)
    with use_ops(hip_ops):
        alg = TemperedSMC(target, n, n_moves=2)
        res = alg.run(genjax.random.key(11, "philox"))
        pw = alg.pointwise(res)
        assert pw.lppd.shape == pw.mean.shape == pw.var.shape == pw.count.shape == (D,) and pw.lppd.dtype == torch.float64 and pw.lppd.is_cuda
        own = -2.0 * float((pw.lppd - pw.var).sum())
        print(f"waic {pw.waic:.4f}, p_waic {pw.p_waic:.4f}, lpd {pw.log_predictive_density:.4f}, se {pw.elpd_waic_se:.4f}")
        assert math.isfinite(pw.waic) and math.isclose(pw.waic, own, rel_tol=1e-12) and pw.p_waic > 0.0 and math.isfinite(pw.elpd_waic_se)
        assert torch.equal(pw.count, torch.full_like(pw.count, float(n)))
        assert torch.equal(alg.pointwise(res.columns).lppd, pw.lppd)  # a list of columns is the same call
        # the call's launches, counted by graph capture (compiled above: nothing compiles inside the capture)
        plan = alg._state()["tplan"]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g, stream=side):
            out = hip_ops.temper_pointwise(plan, res.columns)
        nodes = _kernel_nodes(g.raw_cuda_graph())
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0] - math.log(n), pw.lppd)
        del g, out
    assert nodes == 2
