"""The CPU oracle's Gamma, Beta and Bernoulli sites pinned against float64 over the WHOLE parameter range (dist_range_ref.py:
shapes 0.01 .. 1e4), where f32 code goes wrong and hierarchical priors routinely go: the `conc < 1` boost underflows, m_exp
flushes below -86, m_lgamma changes branch at 8, lgamma(a) + lgamma(b) - lgamma(a + b) cancels, draws land on 0, on
subnormals and on 1.  The GPU suite (test_gpu_dist_range.py) then holds the HIP library to this oracle bit for bit."""

import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy import special, stats

import dist_range_ref as R
from genjax._amd.ops import KeyBatch
from offline import importance_source, ops as hip_lib_nogpu  # noqa: F401

N = 100_000


def test_lgamma_over_sixty_decades(oracle_ops):
    """m_lgamma on exp(U(-30, 30)) under the bound test_math_spec_accuracy sets on [e^-6, e^6] (probed: 3.5e-6, at x = 0.42)."""
    raw = oracle_ops.lib._dll
    x = np.exp(np.random.default_rng(0).uniform(-30, 30, 200000)).astype(np.float32)
    x[:len(R.SHAPES)] = R.SHAPES
    y = np.empty_like(x)
    raw.gjo_math(3, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_uint64(x.size))
    ref = special.gammaln(x.astype(np.float64))
    assert np.max(np.abs(y - ref) / np.maximum(1, np.abs(ref))) < 1e-5


def test_logpdf_grid_against_float64(oracle_ops):
    R.check_logpdf_grid(oracle_ops)


def test_golden_fixture_is_the_grid():
    """logpdf_wide.json holds every (shape, rate) and every Beta pair of the grid, with the support's edges and the smallest
    normal and subnormal f32 among the points."""
    g = R.golden()
    assert [(r["concentration"], r["rate"]) for r in g["gamma"]] == [(R.f32(a), R.f32(b)) for a, b in R.gamma_density_params()]
    assert [(r["a"], r["b"]) for r in g["beta"]] == [(R.f32(a), R.f32(b)) for a, b in R.BETA_PAIRS]
    for r in g["gamma"] + g["beta"]:
        assert {0.0, R.F32_MIN_NORMAL, R.F32_MIN_SUBNORMAL} <= set(r["x"]) and len(r["x"]) == len(r["logpdf"])
        assert all(float(np.float32(x)) == x for x in r["x"])
    assert all(1.0 in r["x"] for r in g["beta"])


def _draw(ops, dist, impl, a, b):
    kb = KeyBatch(impl, 1, parent=(123, 456), first=0)
    v, s = ops.sample_logpdf(dist, kb.with_fold(2 if dist == "gamma" else 3), N, R.f32(a), R.f32(b))
    return v.numpy(), s.numpy()


def _check_scores(v, s, ref, tol, what):
    """The fused score is the density formula at the drawn value: finite within the density tolerance, infinite with scipy's sign."""
    R.compare_logpdf(s, ref, tol, what + " score")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("a,rate", R.gamma_sampler_cases())
def test_gamma_sampler(oracle_ops, impl, a, rate):
    v, s = _draw(oracle_ops, "gamma", impl, a, rate)
    assert not np.isnan(v).any() and (v >= 0).all()
    a32, r32 = R.f32(a), R.f32(rate)
    d = stats.gamma(a32, scale=1.0 / r32)
    D, p = R.clipped_ks(v, d.cdf, *R.GAMMA_WINDOW)
    print(f"gamma({a}, {rate}) impl {impl}: D = {D:.4g}, p = {p:.4g}, zeros {np.mean(v == 0):.3g}")
    assert p > 1e-3, (D, p)
    with np.errstate(all="ignore"):
        ref = d.logpdf(v.astype(np.float64))
    fin = np.isfinite(v)  # (+inf at rate 1e-3 would be an overflow of the division: none in the grid)
    assert fin.all()
    _check_scores(v, s, ref, R.gamma_tolerance(v, a32, r32), f"gamma({a}, {rate})")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("a,b", R.BETA_PAIRS)
def test_beta_sampler(oracle_ops, impl, a, b):
    """Before beta_from_gammas the draws of (0.01, 0.01) were NaN for 17.8 % of the particles and those of (0.05, 0.05) for
    0.02 % (both gammas flushed to 0: 0 / 0), with both generators; every other case passed as it does now."""
    v, s = _draw(oracle_ops, "beta", impl, a, b)
    assert not np.isnan(v).any(), f"{np.isnan(v).mean():.3%} NaN draws"
    assert (v >= 0).all() and (v <= 1).all()
    a32, b32 = R.f32(a), R.f32(b)
    d = stats.beta(a32, b32)
    D, p = R.clipped_ks(v, d.cdf, *R.BETA_WINDOW)
    print(f"beta({a}, {b}) impl {impl}: D = {D:.4g}, p = {p:.4g}, zeros {np.mean(v == 0):.3g}, ones {np.mean(v == 1):.3g}")
    assert p > 1e-3, (D, p)
    with np.errstate(all="ignore"):
        ref = d.logpdf(v.astype(np.float64))
    _check_scores(v, s, ref, R.beta_tolerance(v, a32, b32), f"beta({a}, {b})")


@pytest.mark.parametrize("impl", [0, 1])
def test_beta_edge_draws_score_the_matching_infinity(oracle_ops, impl):
    """Beta(0.01, 0.01) puts most of its f32 draws ON 0 and 1 (inherent to f32): each scores +inf (a, b < 1), every draw
    strictly inside the support scores a finite number."""
    v, s = _draw(oracle_ops, "beta", impl, 0.01, 0.01)
    edge = (v == 0) | (v == 1)
    assert edge.any() and np.isposinf(s[edge]).all()
    assert np.isfinite(s[~edge]).all()


@pytest.mark.parametrize("impl", [0, 1])
def test_bernoulli_on_the_p_grid(oracle_ops, impl):
    """The sampler compares a 23-bit uniform with p: the frequency of 1 is floor(p 2^23) / 2^23 up to 4 sigma.  The density
    is log p / log(1 - p), -inf at the impossible outcome (dist_range_ref.check_bernoulli_logpdf, part of the grid test)."""
    kb = KeyBatch(impl, 1, parent=(123, 456), first=0).with_fold(4)
    for p in R.BERNOULLI_P:
        p32 = R.f32(p)
        v, s = oracle_ops.sample_logpdf("bernoulli", kb, N, p32)
        v, s = v.numpy(), s.numpy()
        q = math.floor(p32 * 2**23) / 2**23
        assert abs(v.mean() - q) <= 4 * math.sqrt(q * (1 - q) / N), (p, v.mean(), q)
        for e in (0, 1):
            if (v == e).any():
                ref = R.bernoulli_ref(e, p)
                assert math.isfinite(ref), f"p = {p}: the impossible outcome {e} was drawn"
                assert np.all(np.abs(s[v == e] - ref) <= 2e-7 * max(1.0, abs(ref)) + 1e-7)


def test_generated_kernels_take_the_log_space_branch_only_where_it_can_run(hip_lib_nogpu, monkeypatch):
    """The plans of the GPU suite as generated sources: a Beta site whose shapes are columns, parameters, earlier draws or
    literals below 1 goes through beta_from_gammas in every kernel form; a literal shape that is not below 1 (the benchmark's
    Beta(2, 2)) keeps the bare ratio, so its kernel is the one it was.  The 'inputs' plan compiles for gfx950 offline."""
    from genjax._amd import abi, workloads as W  # noqa: F401

    ops = hip_lib_nogpu
    for kind, n_beta in (("inputs", 2), ("site_shape", 1), ("lit_beta", 1), ("lit_gamma", 1)):
        plan = ops.plan_create(R.importance_sites(kind)[0])
        for impl, form, per_lane in ((0, None, 1), (1, None, 4), (1, "pair", 2), (1, "one", 1)):
            if form:
                monkeypatch.setenv("GJX_JIT_FORM", form)
            else:
                monkeypatch.delenv("GJX_JIT_FORM", raising=False)
            src = importance_source(ops, plan, impl)
            assert src.count("beta_from_gammas<") == n_beta * per_lane, (kind, impl, form)
    monkeypatch.delenv("GJX_JIT_FORM", raising=False)
    A = abi.Arg
    for a, b, helper in ((2.0, 2.0, 0), (0.5, 3.0, 0), (1.0, 0.5, 0), (0.999, 0.5, 1)):
        s_ = R._site(abi.DIST_BETA, A(abi.ARG_CONST, 0, 0.0, a, None), A(abi.ARG_CONST, 0, 0.0, b, None), out_col=0)
        for impl in (0, 1):
            src = importance_source(ops, ops.plan_create([s_]), impl)
            assert (src.count("beta_from_gammas<") > 0) == bool(helper), (a, b, impl)
    plan = ops.plan_create(R.importance_sites("inputs")[0])
    for impl in (0, 1):
        ops.lib.call("gjx_plan_compile_check", plan.handle, impl)
