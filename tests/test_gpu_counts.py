"""The count families on the GPU (include/gjx_counts.h): the stand-alone density kernels against the scipy fixture, the draw
kernels against a float64 replay of the header's rule from the same cipher words, the negative binomial's moments, the plated
route (run, pointwise, loo, predictive over Poisson and negative-binomial regressions and a mixed body), the per-site route,
and a conjugate Gamma-Poisson model end to end against its closed forms.  References, tolerances and recorded noise:
tests/counts_ref.py."""

import math

import numpy as np
import pytest
import torch

import counts_ref as K
import genjax
import pointwise_ref as W
import psis_ref as S
from genjax import ChoiceMap, Target, gamma, gen, negative_binomial, normal, poisson
from genjax._amd import abi, prng, temper
from genjax._amd.ops import KeyBatch
from genjax._amd.runtime import use_ops
from genjax.inference.smc import ImportanceK, PSISLOO, PointwiseLikelihood, TemperedSMC

pytestmark = pytest.mark.gpu

IMPLS = [0, 1]
U32 = 2.0 ** -23  # one f32 ulp, relative


def dev(a, ops, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=ops.device(), dtype=dtype).contiguous()


# ---- stand-alone kernels: densities -------------------------------------------------------------------------------------------
def _grid():
    """(family, k, a0, a1, want) flattened over the fixture."""
    g = K.golden()
    poi = [(k, c["rate"], w) for c in g["poisson"] for k, w in zip(c["k"], c["logpmf"])]
    nb = [(k, c["total_count"], c["probs"], w) for c in g["negative_binomial"] for k, w in zip(c["k"], c["logpmf"])]
    return np.array(poi, dtype=np.float64), np.array(nb, dtype=np.float64)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_densities_against_float64(hip_ops, n):
    poi, nb = _grid()
    worst = {}
    for name, tab, tol in (("poisson", poi, K.poisson_tolerance), ("negative_binomial", nb, K.nb_tolerance)):
        idx = (np.arange(n) * 7 + 3 * n) % len(tab)  # n points of the grid, another walk through it per n
        for part in [tab[idx]] + ([tab] if n == 257 else []):  # (n = 257: the whole grid as well, one launch)
            m = len(part)
            k = dev(part[:, 0], hip_ops, torch.int32)
            args = [dev(part[:, j], hip_ops) for j in range(1, part.shape[1] - 1)]
            got = hip_ops.logpdf(name, m, k if m > 1 else int(part[0, 0]), *args).cpu().numpy().astype(np.float64)
            t = tol(*[part[:, j] for j in range(part.shape[1] - 1)])
            err = np.abs(got - part[:, -1])
            worst[name] = max(worst.get(name, 0.0), float(np.max(err / t)))
            assert np.all(err <= t), (name, n, part[np.argmax(err / t)], got[np.argmax(err / t)])
            # a scalar value and a column value agree bit for bit
            j = m // 2
            one = hip_ops.logpdf(name, 1, int(part[j, 0]), *[float(a[j]) for a in args]).cpu().numpy()
            assert one.view(np.uint32)[0] == got.astype(np.float32).view(np.uint32)[j], (name, n, j)
    print("n", n, "largest error / tolerance", worst)


def test_density_edges(hip_ops):
    """Outside the support: -inf; outside the domain: NaN (checked first); rate 0 and probs 1 follow the formula."""
    lp = lambda name, v, *a: float(hip_ops.logpdf(name, 1, v, *a).cpu()[0])  # noqa: E731
    assert lp("poisson", -1, 3.0) == -math.inf and lp("negative_binomial", -2, 3.0, 0.5) == -math.inf
    assert math.isnan(lp("poisson", 2, -1.0)) and math.isnan(lp("poisson", -1, float("nan")))
    assert math.isnan(lp("negative_binomial", 2, 0.0, 0.5)) and math.isnan(lp("negative_binomial", 2, 3.0, 1.5))
    assert math.isnan(lp("negative_binomial", 2, -1.0, 0.5)) and math.isnan(lp("negative_binomial", -1, 3.0, -0.1))
    assert abs(lp("poisson", 0, 0.0)) <= 1e-5 and lp("poisson", 3, 0.0) == -math.inf
    assert lp("negative_binomial", 3, 2.0, 1.0) == -math.inf


# ---- stand-alone kernels: draws -----------------------------------------------------------------------------------------------
N = K.N_DRAWS
RATE_CASES = [0.05, 3.0, 9.99, 10.0, 50.0, 1e3, 1e4, "mixed"]


def _rates(case):
    if case == "mixed":  # both sides of 10 inside every wave, with 0 and the edges of the PTRS branch among them
        cyc = np.array([0.0, 0.3, 2.5, 9.5, 9.99, 10.0, 10.01, 12.0, 40.0, 300.0, 7.0, 1.0, 25.0], dtype=np.float32)
        return cyc[np.arange(N) % len(cyc)]
    return np.full(N, case, dtype=np.float32)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case", RATE_CASES)
def test_poisson_draws_replay_the_header(hip_ops, impl, case):
    parent, first, fold = (41, 42), 10, 2
    kb = KeyBatch(impl, 1, parent=parent, first=first).with_fold(fold)
    st = K.Streams(impl, parent, first, N, fold)
    if case == 0.05:  # the host ciphers against the device's words, once per cipher
        for sub in (1, 5):
            bits = hip_ops.rng_bits(kb, N, sub).cpu().numpy().view(np.uint32).astype(np.uint64)
            assert np.array_equal(bits, st.bits32(sub)), (impl, sub)
    rate = _rates(case)
    a = float(rate[0]) if case != "mixed" else dev(rate, hip_ops)
    v, s = hip_ops.sample_logpdf("poisson", kb, N, a)
    assert v.dtype == torch.int32 and v.shape == (N,) and s.dtype == torch.float32
    ref = K.poisson_replay(st, 0, rate.astype(np.float64))
    got = v.cpu().numpy().astype(np.int64)
    frac = float(np.mean(got != ref))
    allowed = 1e-2 if case == 1e4 else 2e-3
    mean, want = got.mean(), float(rate.astype(np.float64).mean())
    print(f"impl {impl} rate {case}: {frac:.2e} of the draws differ from the float64 replay (allowed {allowed}); mean {mean:.4f} against {want:.4f}")
    assert frac <= allowed
    assert got.min() >= 0 and abs(mean - want) <= 6.0 * math.sqrt(max(want, 1e-3) / N) + 1e-9  # (not a replay of nothing)
    # each value's score is the density kernel's at it, bit for bit
    again = hip_ops.logpdf("poisson", N, v, a)
    assert torch.equal(s.view(torch.int32), again.view(torch.int32))
    assert bool(torch.isfinite(s).all())


def test_poisson_draw_edges(hip_ops):
    """Rates outside the rule's two branches: 0, an invalid one, the saturation above 2^30 — no word is read, nothing waits."""
    rate = dev(np.array([0.0, -1.0, np.nan, 2.0 ** 30 * 1.5, np.inf, 2.0 ** 30], dtype=np.float32), hip_ops)
    for impl in IMPLS:
        v, s = hip_ops.sample_logpdf("poisson", KeyBatch(impl, 1, parent=(5, 6), first=0).with_fold(1), 6, rate)
        v, s = v.cpu().numpy(), s.cpu().numpy()
        assert v[0] == 0 and v[1] == -1 and v[2] == -1 and v[3] == 1 << 30 and v[4] == 1 << 30 and 0 <= v[5] < 2 ** 31
        assert np.isnan(s[1]) and np.isnan(s[2])
        # the negative binomial: outside the domain -1 with a NaN score; probs == 1 (no finite count) -1 with score -inf
        kb = KeyBatch(impl, 1, parent=(5, 6), first=0).with_fold(1)
        r = dev(np.array([0.0, 2.0, 2.0, 1e-3, 2.0], dtype=np.float32), hip_ops)
        p = dev(np.array([0.5, 1.5, 1.0, 1.0, 0.0], dtype=np.float32), hip_ops)
        v, s = (t.cpu().numpy() for t in hip_ops.sample_logpdf("negative_binomial", kb, 5, r, p))
        assert list(v) == [-1, -1, -1, -1, 0] and np.isnan(s[0]) and np.isnan(s[1]) and s[2] == -np.inf and s[3] == -np.inf and abs(s[4]) <= 1e-5


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("r, p", K.NB_MOMENT_CASES)
def test_negative_binomial_moments(hip_ops, impl, r, p):
    kb = KeyBatch(impl, 1, parent=(51, 52), first=0).with_fold(1)
    v, s = hip_ops.sample_logpdf("negative_binomial", kb, N, r, p)
    x = v.cpu().numpy().astype(np.float64)
    m, var = r * p / (1 - p), r * p / (1 - p) ** 2
    rm, rv = K.NB_MOMENT_RMS[(r, p)]
    print(f"impl {impl} NB({r}, {p}): mean {x.mean():.5f} against {m:.5f} (allowed {4 * rm:.5f}); variance {x.var():.4f} against {var:.4f} (allowed {4 * rv:.4f})")
    assert x.min() >= 0 and abs(x.mean() - m) <= 4.0 * rm and abs(x.var() - var) <= 4.0 * rv
    again = hip_ops.logpdf("negative_binomial", N, v, r, p)
    assert torch.equal(s.view(torch.int32), again.view(torch.int32))
    # the gamma owns sub-streams 0 .. 128 and the Poisson part starts at 256: the draws replay from the gamma kernel's value
    g, _ = hip_ops.sample_logpdf("gamma", kb, N, r, 1.0)
    lam = (g.cpu().numpy() * np.float32(np.float32(p) / (np.float32(1.0) - np.float32(p)))).astype(np.float32)
    ref = K.poisson_replay(K.Streams(impl, (51, 52), 0, N, 1), 256, lam.astype(np.float64))
    frac = float(np.mean(x.astype(np.int64) != ref))
    print(f"   {frac:.2e} of the draws differ from the float64 replay over the gamma kernel's rates")
    assert frac <= 2e-3


# ---- the plated route ---------------------------------------------------------------------------------------------------------
@gen
def pois_rate(xs):
    w = normal(0.0, 1.0) @ "w"
    b = normal(0.0, 1.0) @ "b"
    poisson(torch.exp(w * xs + b)) @ "y"


@gen
def pois_log(xs):
    w = normal(0.0, 1.0) @ "w"
    b = normal(0.0, 1.0) @ "b"
    poisson(log_rate=w * xs + b) @ "y"


@gen
def negbin(xs):
    w = normal(0.0, 1.0) @ "w"
    r = gamma(4.0, 1.0) @ "r"
    negative_binomial(r, logits=w * xs) @ "y"


@gen
def mixed(xs):
    w = normal(0.0, 1.0) @ "w"
    b = normal(0.0, 1.0) @ "b"
    normal(w * xs + b, 0.5) @ "z"
    poisson(log_rate=w * xs + b) @ "y"
    poisson(3.0 * w * w + 1.0) @ "c"  # a scalar OBSERVED count site: log k! in the kernel, its value a launch parameter


MODELS = {"pois_rate": pois_rate, "pois_log": pois_log, "negbin": negbin, "mixed": mixed}
DS = [1, 3, 4, 5, 9, 257, 513]  # the row block of 4 and its remainder, PSIS's four rows, predictive's two rows per lane, the tiles
N_PART = 512
C_OBS = 4  # the observed value of the scalar site "c"
U24 = 2.0 ** -24  # the relative error of one f32 rounding


def case(name, D, seed=0):
    """-> (Target, xs, {address: observed column}) of model `name` over D >= 2 rows, data drawn at w = 0.8, b = 0.5 (r = 4)."""
    rng = np.random.default_rng(100 + seed + D)
    xs = np.linspace(-1.0, 1.0, D).astype(np.float32)
    eta = 0.8 * xs.astype(np.float64) + 0.5
    if name == "negbin":
        pr = 1.0 / (1.0 + np.exp(-0.8 * xs.astype(np.float64)))
        obs = {"y": rng.negative_binomial(4.0, 1.0 - pr).astype(np.float32)}
    else:
        obs = {"y": rng.poisson(np.exp(eta)).astype(np.float32)}
    if name == "mixed":
        obs["z"] = (eta + 0.5 * rng.standard_normal(D)).astype(np.float32)
    con = [(a, torch.from_numpy(v)) for a, v in obs.items()] + ([("c", C_OBS)] if name == "mixed" else [])
    return Target(MODELS[name], (torch.from_numpy(xs),), ChoiceMap.from_mapping(con)), xs, obs


def lowered(ops, name, D, n=N_PART):
    """-> (plan with the data of D rows set, xs [D], {address: observed [D]}).  The source of a plan holds no row count, and a
    one-element tensor is not a data column to the tracer: D = 1 is the first row of the two-row lowering."""
    target, xs, obs = case(name, max(D, 2))
    with use_ops(ops):
        tr = temper.lower(target, n)
        plan = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
        if tr.params:
            plan.set_params(tr.params)
        plan.set_data([c[:D].contiguous() for c in tr.data_columns(ops.device())])
    return plan, xs[:D], {a: v[:D] for a, v in obs.items()}


def population(name, n, seed, width=0.1):
    """Latent columns around the values the data were drawn at, `width` wide (float32 numpy)."""
    rng = np.random.default_rng(seed)
    w = (0.8 + width * rng.standard_normal(n)).astype(np.float32)
    if name == "negbin":
        return [w, (4.0 * np.exp(width * rng.standard_normal(n))).astype(np.float32)]
    return [w, (0.5 + width * rng.standard_normal(n)).astype(np.float32)]


def terms64(ops, name, xs, obs, cols):
    """The float64 reference of the plated sites' row terms AT THE KERNEL'S OWN f32 ARGUMENTS, and its tolerance.

    The arguments are the programs' values, one f32 rounding per operator: w * x and + b are torch's f32 operations, exp and the
    division of the sigmoid the spec's own functions through gjx_map_f32 (test_predictive_draws holds the draws at exactly these
    arguments to the stand-alone kernel's, bit for bit).  The count sites' tolerances are counts_ref's, nothing added.
    -> (t [D, n]: the f32-ordered sum over the plated sites, tol [D, n], parts: {address: its terms [D, n]}).

    The Normal site of `mixed`, for which there is no pinned tolerance: the kernel computes d = z rs - loc rs with rs = 2 (both
    products exact, one rounding of the difference), then (-d / 2) d - lognorm (one rounding of the product, one of the
    difference) with lognorm the f32 of 0.9189385 + m_log(0.5), off by at most 3.2e-7 (m_log to 2e-7, two roundings of numbers
    below 1).  So |term - truth| <= 2^-23 d^2 + 2^-24 |term| + 3.2e-7.  The two sites' terms are added in f32: 2^-24 |t| more."""
    x = dev(xs, ops)[:, None]
    c = [dev(v, ops)[None, :] for v in cols]
    y = obs["y"].astype(np.float64)[:, None]
    wx = c[0] * x
    f64 = lambda v: v.cpu().numpy().astype(np.float64)  # noqa: E731
    if name == "negbin":
        p = f64(ops.map_f32(abi.MAP_RDIV, ops.map_f32(abi.MAP_EXP, -wx) + 1.0, 1.0))
        r = np.asarray(cols[1], dtype=np.float64)[None, :]
        t = K.nb_logpmf(y, r, p)
        return t, K.nb_tolerance(y, r, p), {"y": t}
    eta = wx + c[1]
    rate = f64(ops.map_f32(abi.MAP_EXP, eta))
    t, tol = K.poisson_logpmf(y, rate), K.poisson_tolerance(y, rate)
    parts = {"y": t}
    if name == "mixed":
        d = 2.0 * obs["z"].astype(np.float64)[:, None] - 2.0 * f64(eta)
        tz = -0.5 * d * d - (0.5 * math.log(2 * math.pi) + math.log(0.5))
        parts["z"] = tz
        t, tol = tz + t, tol + (2.0 * U24 * d * d + U24 * np.abs(tz) + 3.2e-7) + U24 * np.abs(tz + t)
    return t, tol, parts


def _ll_check(ops, name, D, xs, obs, cols, got):
    """ll against the float64 sum over the rows: the per-row tolerances summed, plus one f32 ulp of the total.  `mixed` has
    three observed sites where that bound has one: ll = ((float) acc_z + (float) acc_y) + term_c rounds each plated total, their
    sum and the last add — the roundings of acc_z, acc_y and of their sum are added to the bound, with the scalar site's own
    tolerance (counts_ref's, at its f32 rate ((3 w) w) + 1)."""
    t, tol, parts = terms64(ops, name, xs, obs, cols)
    want, bound = t.sum(axis=0), tol.sum(axis=0)
    if name == "mixed":
        w = dev(cols[0], ops)
        rate_c = (((w * 3.0) * w) + 1.0).cpu().numpy().astype(np.float64)
        tz, ty = parts["z"].sum(axis=0), parts["y"].sum(axis=0)
        want = tz + ty + K.poisson_logpmf(float(C_OBS), rate_c)
        bound = bound + K.poisson_tolerance(float(C_OBS), rate_c) + U24 * (np.abs(tz) + np.abs(ty) + np.abs(tz + ty))
    bound = bound + U32 * np.abs(want)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    err = np.abs(got.astype(np.float64) - want)
    print(name, D, f"largest ll error / bound {np.max(err / bound):.3g}; |ll| up to {np.abs(want).max():.4g}")
    assert np.all(err <= bound), (name, D)


@pytest.mark.parametrize("name", list(MODELS))
def test_recompute_ll(hip_ops, name):
    """gjx_temper_move with n_moves = 0 and recompute: the ll column against the float64 sum over the rows."""
    for D in DS:
        plan, xs, obs = lowered(hip_ops, name, D)
        cols = population(name, N_PART, 11 * D, width=0.5)
        x, lp, ll, _ = hip_ops.temper_move(plan, prng.key(1, 1), [dev(c, hip_ops) for c in cols], None, None, 0.0, 0, None,
                                           recompute=True, want_accept=False)
        assert all(torch.equal(a, dev(c, hip_ops)) for a, c in zip(x, cols))
        _ll_check(hip_ops, name, D, xs, obs, cols, ll.cpu().numpy())


@pytest.mark.parametrize("name", list(MODELS))
def test_run_without_moves(hip_ops, name):
    """TemperedSMC.run with n_moves = 0: the prior's population, resampled; its ll column is stage 0's recompute, carried."""
    D = 5
    target, xs, obs = case(name, D)
    with use_ops(hip_ops):
        res = TemperedSMC(target, N_PART, n_moves=0).run(prng.key(7, 1))
    assert math.isfinite(res.log_marginal_likelihood) and len(res.betas) >= 2
    _ll_check(hip_ops, name, D, xs, obs, [c.cpu().numpy() for c in res.columns], res.ll.cpu().numpy())


def _own_terms(ops, plan, x):
    """The kernel's own t[d, i], float32 [D, n]: the pointwise kernel over ONE particle at a time (its s1 row is the term)."""
    n = x[0].numel()
    rows = [ops.temper_pointwise(plan, [c[i:i + 1] for c in x])[1] for i in range(n)]
    t = torch.stack(rows, dim=1).cpu().numpy()
    assert np.array_equal(t, t.astype(np.float32).astype(np.float64))
    return t.astype(np.float32)


@pytest.mark.parametrize("name", list(MODELS))
def test_pointwise_and_loo(hip_ops, name):
    n = N_PART
    for D in DS:
        plan, xs, obs = lowered(hip_ops, name, D)
        cols = population(name, n, 3 * D + 1)
        x = [dev(c, hip_ops) for c in cols]
        t = _own_terms(hip_ops, plan, x)
        pw = PointwiseLikelihood(hip_ops.temper_pointwise(plan, x), n)
        M = S.tail_len(n)
        assert M == int(hip_ops.lib.call("gjx_psis_tail_len", n, 1.0))
        out, tail = hip_ops.temper_psis(plan, x, M, want_tail=True)
        loo = PSISLOO(out, pw, n, M)
        # every term against float64
        t64, tol, _ = terms64(hip_ops, name, xs, obs, cols)
        ratio = np.abs(t.astype(np.float64) - t64) / tol
        print(name, D, f"largest term error / tolerance {ratio.max():.3g}")
        assert t.shape == t64.shape == (D, n) and np.all(ratio <= 1.0), (name, D)
        # the reductions against the float64 reductions of the same table, with pointwise_ref's bounds
        ref = W.reduce64(t)
        b1, b2 = W.moment_bounds(t)
        assert W.spread(t).max() < W.LSE_MAX_SPREAD
        lppd, mean, var = (v.cpu().numpy() for v in (pw.lppd, pw.mean, pw.var))
        assert np.all(np.abs(lppd - (ref[0] - math.log(n))) <= W.LSE_TOL), (name, D)
        assert np.all(np.abs(mean - ref[1] / n) <= b1 / n), (name, D)
        # (var = (s2 - s1^2 / n) / (n - 1): the bounds of s1 and s2 through it, and the float64 roundings of the expression)
        vref = (ref[2] - ref[1] * ref[1] / n) / (n - 1)
        vb = (b2 + 2.0 * np.abs(ref[1]) * b1 / n + b1 * b1 / n + 4.0 * W.U52 * (np.abs(ref[2]) + ref[1] * ref[1] / n)) / (n - 1)
        assert np.all(np.abs(var - vref) <= vb), (name, D)
        # the tail: bit-equal to the sort of the kernel's own terms under the header's order
        tail = tail.cpu().numpy()
        assert tail.shape == (D, M + 1)
        for d in range(D):
            want, _ = S.select(t[d], M)
            assert np.array_equal(S.keys(tail[d]), S.keys(want)), (name, D, d)
        assert bool(torch.isfinite(loo.elpd_loo).all()) and math.isfinite(loo.elpd)
        print(name, D, f"elpd_loo {loo.elpd:.4f}, lppd {pw.log_predictive_density:.4f}, largest khat {float(loo.khat.max()):.3f}")
    # the public calls over the fitted rows give those tables
    target, _, _ = case(name, 9)
    with use_ops(hip_ops):
        alg = TemperedSMC(target, n)
        cols9 = [dev(c, hip_ops) for c in population(name, n, 28)]
        plan9, _, _ = lowered(hip_ops, name, 9)
        assert torch.equal(alg.pointwise(cols9).lppd, PointwiseLikelihood(hip_ops.temper_pointwise(plan9, cols9), n).lppd)
        assert torch.equal(alg.loo(cols9).elpd_loo, hip_ops.temper_psis(plan9, cols9, S.tail_len(n))[0][0])


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", ["pois_log", "negbin", "mixed"])
def test_predictive_draws(hip_ops, impl, name):
    """The draws (draw_stride = 1) of a plated count site are the stand-alone kernel's for the key batch
    split_lazy(fold_in(key, i), D) under the site's number among the plated sites, at the arguments the body computes (through
    the spec's own functions: lang.SpecTensor); below / equal / s1 / s2 follow from the draws in float64.  n = 512: blocks of
    particles and their remainder; at D <= 9 several chunks of particles per row tile."""
    n = N_PART
    key = prng.key(77, impl)
    site = 1 if name == "mixed" else 0  # ("z" is plated site 0 of the mixed body)
    for D in (1, 3, 4, 5, 9, 257, 513):
        plan, xs, obs = lowered(hip_ops, name, D, n)
        cols = population(name, n, 5 * D + impl)
        x = [dev(c, hip_ops) for c in cols]
        table, draws = hip_ops.temper_predictive(plan, key, x, 1)
        xd = dev(xs, hip_ops)
        rows = []
        for i in range(n):
            kb = prng.split_lazy(prng.fold_in(key, i), D).with_fold(site + 1 if impl == 0 else site)
            wx = float(cols[0][i]) * xd  # (f32: one rounding per operator, as the program's)
            if name == "negbin":
                e = hip_ops.map_f32(abi.MAP_EXP, -wx)
                p = hip_ops.map_f32(abi.MAP_RDIV, e + 1.0, 1.0)
                v, _ = hip_ops.sample_logpdf("negative_binomial", kb, D, float(cols[1][i]), p if D > 1 else float(p))
            else:
                rate = hip_ops.map_f32(abi.MAP_EXP, wx + float(cols[1][i]))
                v, _ = hip_ops.sample_logpdf("poisson", kb, D, rate if D > 1 else float(rate))
            rows.append(v)
        ref = torch.stack(rows).cpu().numpy().astype(np.float32)  # (one host read)
        got = draws[site].cpu().numpy()
        assert got.shape == (n, D) and np.array_equal(got, ref), (name, impl, D, int((got != ref).sum()))
        y64 = ref.astype(np.float64)
        o = np.rint(obs["y"]).astype(np.float64)[None, :]
        tab = table[site].cpu().numpy()  # rows s1, s2, below, equal, nan
        assert np.array_equal(tab[2], (y64 < o).sum(axis=0)) and np.array_equal(tab[3], (y64 == o).sum(axis=0)) and not tab[4].any()
        assert np.array_equal(tab[0], y64.sum(axis=0)) and np.array_equal(tab[1], (y64 * y64).sum(axis=0))  # (integers: exact)
    # the public call; args=: nothing observed, no pit, the same draws (the fill of the unobserved count site is zeros)
    target, _, _ = case(name, 5)
    with use_ops(hip_ops):
        alg = TemperedSMC(target, n)
        x = [dev(c, hip_ops) for c in population(name, n, 9)]
        seen = alg.predictive(x, key, draw_stride=1)
        free = alg.predictive(x, key, args=target.args, draw_stride=1)
    assert seen.pit is not None and seen.draws["y"].shape == (n, 5) and bool(((seen.pit["y"] >= 0) & (seen.pit["y"] <= 1)).all())
    assert free.pit is None and free.below is None and torch.equal(free.draws["y"], seen.draws["y"])
    assert torch.equal(free.mean["y"], seen.mean["y"])


@gen
def scalar_counts():
    lam = gamma(2.0, 1.0) @ "lam"
    poisson(lam) @ "k"
    negative_binomial(2.0, logits=lam) @ "m"


def test_scalar_observed_count_sites(hip_ops):
    """A body with count sites and NO data column: stage 0 draws from the table without them (the importance kernels do not know
    the ids), the move kernel evaluates log k! itself.  ll of the run without moves is the stand-alone kernels' sum, bit for bit
    (the same device functions at the same f32 arguments, added in table order)."""
    n = 4096
    for impl in IMPLS:
        with use_ops(hip_ops):
            alg = TemperedSMC(Target(scalar_counts, (), ChoiceMap.d({"k": 4, "m": 3})), n, n_moves=0)
            res = alg.run(prng.key(5, impl))
            lam = res.columns[0]
            p = hip_ops.map_f32(abi.MAP_RDIV, hip_ops.map_f32(abi.MAP_EXP, -lam) + 1.0, 1.0)
            want = hip_ops.logpdf("poisson", n, 4, lam) + hip_ops.logpdf("negative_binomial", n, 3, 2.0, p)
        assert math.isfinite(res.log_marginal_likelihood) and bool((lam > 0).all())
        assert torch.equal(res.ll.view(torch.int32), want.view(torch.int32)), int((res.ll != want).sum())
        with use_ops(hip_ops):
            moved = TemperedSMC(Target(scalar_counts, (), ChoiceMap.d({"k": 4, "m": 3})), n).run(prng.key(6, impl))
        assert math.isfinite(moved.log_marginal_likelihood) and abs(moved.log_marginal_likelihood - res.log_marginal_likelihood) < 0.5


# ---- the per-site route -------------------------------------------------------------------------------------------------------
@gen
def per_site(c):
    lam = gamma(3.0, c) @ "lam"
    k = poisson(lam) @ "k"
    m = negative_binomial(2.5, probs=0.4) @ "m"
    return k + m


def test_per_site_route(hip_ops):
    n = 1000
    with use_ops(hip_ops):
        for impl in IMPLS:
            keys = genjax.random.split(prng.key(3, impl), n)
            tr = per_site.simulate(keys, (1.5,))
            ch = tr.get_choices()
            lam, k, m = ch["lam"], ch["k"], ch["m"]
            assert k.dtype == torch.int32 and m.dtype == torch.int32 and k.shape == (n,)
            sk = hip_ops.logpdf("poisson", n, k, lam)
            sm = hip_ops.logpdf("negative_binomial", n, m, 2.5, 0.4)
            sl = hip_ops.logpdf("gamma", n, lam, 3.0, 1.5)
            assert torch.allclose(tr.get_score(), (sl + sk) + sm, rtol=0.0, atol=1e-5)
            w, _ = per_site.assess(ch, (1.5,))
            assert torch.allclose(w, tr.get_score(), rtol=0.0, atol=1e-5)
            tr2, w2 = per_site.importance(keys, ChoiceMap.d({"k": 4}), (1.5,))
            lam2 = tr2.get_choices()["lam"]
            assert torch.equal(w2, hip_ops.logpdf("poisson", n, 4, lam2))
            # log_rate= / logits= go through the spec's exp and sigmoid
            a = poisson.logpdf(torch.tensor(3), log_rate=0.7)
            b = hip_ops.logpdf("poisson", 1, 3, float(hip_ops.map_f32(0, torch.tensor(0.7)).cpu()))[0]
            assert float(a) == float(b)
            with pytest.raises(ValueError, match="above 2\\^24"):  # a column of observed counts is checked as a scalar is
                poisson.logpdf(torch.full((n,), 2 ** 24 + 2, dtype=torch.int32), lam)
        est = ImportanceK(Target(per_site, (1.5,), ChoiceMap.d({"k": 4})), k_particles=500)
        z = est.log_marginal_likelihood_estimate(prng.key(11, 1))  # (the fused plan knows no count site: the per-site route)
        assert math.isfinite(float(z))
        # k ~ NB(3, 1 / (1 + c)) marginally: log p(k = 4) in closed form, within six standard errors of a 500-particle estimate
        exact = float(K.nb_logpmf(4.0, 3.0, 1.0 / 2.5))
        print(f"ImportanceK over a count site: {float(z):.4f} against {exact:.4f}")
        assert abs(float(z) - exact) < 0.5


# ---- end to end against a closed form -------------------------------------------------------------------------------------------
@gen
def gamma_poisson(a, b):
    lam = gamma(a, b) @ "lam"
    poisson(lam) @ "y"


def test_end_to_end_closed_form(hip_ops):
    """lam ~ Gamma(a, b), y_d ~ Poisson(lam) over D = 200 counts: log Z, the posterior mean, the predictive moments and
    sum_d elpd_loo_d against the closed forms, each within 4 times the recorded noise of the same statistic (counts_ref.E2E_RMS)."""
    model = K.GammaPoisson()
    n = K.E2E_N
    ys = torch.from_numpy(model.ys.astype(np.float32))
    target = Target(gamma_poisson, (model.a, model.b), ChoiceMap.d({"y": ys}))
    with use_ops(hip_ops):
        alg = TemperedSMC(target, n)
        key = prng.key(2024, 1)
        res = alg.run(key)
        pp = alg.predictive(res, prng.fold_in(key, 99))
        loo = alg.loo(res)
    lam = res.columns[0].cpu().numpy().astype(np.float64)
    st = K.e2e_statistics(model, lam, pred=(pp.mean["y"].cpu().numpy(), pp.var["y"].cpu().numpy()), loo=loo.elpd)
    st["log_z"] = res.log_marginal_likelihood - model.log_z
    for k, v in st.items():
        print(f"{k}: {v:+.5f} (allowed {K.E2E_FACTOR * K.E2E_RMS[k]:.5f})")
    print(f"stages {len(res.betas) - 1}, largest khat {float(loo.khat.max()):.3f}")
    for k, v in st.items():
        assert abs(v) <= K.E2E_FACTOR * K.E2E_RMS[k], (k, v)
