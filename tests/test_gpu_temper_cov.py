"""The covariance proposal of the tempered sampler on the GPU (include/gjx_temper_cov.h): the one-launch moments against the
float64 numpy of tests/temper_cov_ref.py and their factor bit for bit against its Cholesky rule, the covariance move held bit
for bit (tolerance 0) to the replay built from unchanged oracle entry points, plated plans included, the sampler end to end on
the correlated regression against its closed form, and the launch counts."""

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import temper_cov_ref as V
import temper_ref as R
from genjax._amd import temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from test_gpu_guided import _kernel_nodes
from test_gpu_temper import SIZES, _ancestors, _bits, _columns, _dev

pytestmark = pytest.mark.gpu

# tests/temper_cov_ref.py: the float64 restatement on the correlated regression over 64 seeds (default_rng(1000 .. 1063)) at
# n = 4096, K = 2, ESS target 0.5 — measured on the CPU, not on the code under test (profiles/temper_cov_summary.md;
# tests/test_temper_cov_cpu.py re-measures them): RMS log Z error 0.0954, last-stage acceptance at least 0.3409; the DIAGONAL
# proposal's last-stage acceptance at most 0.0736 there.
LOG_Z_BOUND = 5 * V.COV_RMS_LOG_Z
ACCEPT_FLOOR = max(0.5 * V.COV_MIN_ACCEPT, V.DIAG_MAX_ACCEPT)

MODELS = ("regression", "gamma_normal", "beta_bernoulli", "gaussian5", "gaussian16")
# the size of the fixed triangle's entries: the deviation of the proposal of latent l is FACTOR_SIZE * |row l of a standard
# normal triangle| (chosen on the CPU replay so that its cases show accepts and rejects)
FACTOR_SIZE = {"regression": 0.7, "gamma_normal": 0.7, "beta_bernoulli": 0.5, "gaussian5": 0.4, "gaussian16": 0.15}


def _targets():
    out = dict(R.models())
    out["gaussian5"], out["gaussian16"] = V.gaussian_chain_target(5), V.gaussian_chain_target(16)
    return out


@pytest.fixture(scope="module")
def lowered(hip_ops, oracle_ops):
    out = {}
    with use_ops(hip_ops):
        for name, target in _targets().items():
            tracer = temper.lower(target, 64)
            plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            plan.set_params(tracer.params)
            out[name] = (plan, {impl: R.Assess(oracle_ops, tracer, impl) for impl in (0, 1)})
    return out


def _start(name, n, rng):
    if name.startswith("gaussian"):
        return [(2.0 * rng.standard_normal(n)).astype(np.float32) for _ in range(int(name[8:]))]
    return _columns(name, n, rng)


def _factor(name, L):
    """A fixed dense lower triangle with entries of both signs, packed f32."""
    for seed in range(40, 50):  # (the first seed whose triangle has both signs)
        F = np.tril(np.random.default_rng(seed).standard_normal((L, L)))
        if L == 1 or ((F < 0).any() and (F > 0).any()):
            break
    return (FACTOR_SIZE[name] * V.pack(F)).astype(np.float32)


# ---- the moments ------------------------------------------------------------------------------------------------------------
def _population(n, L, rng):
    """L correlated f32 columns with means far from 0 against their deviations (what the shift by particle 0 is for)."""
    z = rng.standard_normal((L, n))
    mix = np.tril(rng.standard_normal((L, L))) + 2.0 * np.eye(L)
    return [c.astype(np.float32) for c in (mix @ z) * 0.3 + np.linspace(-50.0, 100.0, L)[:, None]]


def _moments(hip_ops, x, lw, ws=None, **kw):
    m, f, s, nd = hip_ops.temper_moments(_dev(x), None if lw is None else torch.from_numpy(lw).cuda(), ws, **kw)
    return m.cpu().numpy(), f.cpu().numpy(), s.cpu().numpy(), int(nd.item())


def _check(hip_ops, x, lw, tol, what):
    """The kernel's moments against moments_ref within tol (relative to the deviations), the scales against
    TemperedSMC.population_scales, the factor against factor_ref on the covariance the kernel itself returned (bit for bit),
    a second call on the same workspace and one workgroup (bit for bit)."""
    L, n = len(x), len(x[0])
    ws = hip_ops.temper_moments_workspace(n, L)
    m, f, s, nd = _moments(hip_ops, x, lw, ws)
    rs, rmean, rS = V.moments_ref(x, lw)
    sd = np.sqrt(np.array([rS[V.tri(l, l)] for l in range(L)]))
    pair = np.array([sd[l] * sd[j] for l in range(L) for j in range(l + 1)])
    e_mean = np.abs(m[1:1 + L] - rmean)
    e_cov = np.abs(m[1 + L:] - rS)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{what}: n = {n}, L = {L}: weight sum {m[0]:.6g} (reference {rs:.6g}); largest mean error / sd "
              f"{np.nanmax(np.where(sd > 0, e_mean / sd, 0)):.2e}, largest covariance error / sqrt(S_ll S_jj) "
              f"{np.nanmax(np.where(pair > 0, e_cov / pair, 0)):.2e}; n_degenerate {nd}")
    assert np.all(e_mean <= tol * sd) and np.all(e_cov <= tol * pair), what
    assert abs(m[0] - rs) <= max(tol, 1e-12) * rs
    # (population_scales has no rule for a NaN weight: it sees the entry as the kernel does, without weight)
    lw_t = torch.zeros(n, dtype=torch.float32).cuda() if lw is None else torch.from_numpy(np.where(np.isnan(lw), -np.inf, lw).astype(np.float32)).cuda()
    want = TemperedSMC.population_scales(_dev(x), lw_t).cpu().numpy()
    assert np.all(np.abs(s - want) <= 1e-4 * want), (what, s, want)
    G, ndeg = V.factor_ref(m[1 + L:], L)
    assert np.array_equal(_bits(f), _bits(G.astype(np.float32))) and nd == ndeg, what
    assert np.array_equal(_bits(s), _bits(V.scales_ref(m[1 + L:], L))), what
    for kw in ({}, dict(max_workgroups=1)):
        m2, f2, s2, nd2 = _moments(hip_ops, x, lw, ws, **kw)
        assert np.array_equal(m.view(np.uint64), m2.view(np.uint64)) and np.array_equal(_bits(f), _bits(f2)), (what, kw)
        assert np.array_equal(_bits(s), _bits(s2)) and nd == nd2, (what, kw)
    return m, f, s, nd


@pytest.mark.parametrize("L", [1, 2, 5, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 1000, 70001])
def test_moments(hip_ops, n, L):
    """Equal weights (lw NULL) within 1e-10 of the two-pass float64 reference, relative to the deviations: float64 sums of at
    most 70001 terms.  Weighted, lw = (-20 chisquare(2)) * delta in f32: within 1e-4 — a weight carries up to 6e-6 relative
    error from f32 argument rounding (the bound test_gpu_temper.py::test_ess_ladder states) and a weighted second moment
    amplifies it at most fourfold.  n = 1: S = 0, a zero factor, every latent degenerate."""
    rng = np.random.default_rng(1000 * L + n)
    x = _population(n, L, rng)
    m, f, s, nd = _check(hip_ops, x, None, 1e-10, "equal weights")
    assert m[0] == n
    if n == 1:
        assert np.all(m[1 + L:] == 0) and np.all(f == 0) and np.all(s == 0) and nd == L
        assert np.array_equal(m[1:1 + L], np.array([c[0] for c in x], dtype=np.float64))
    else:
        assert nd == 0
    for delta in (2.0 ** -10, 1.0):
        lw = ((-20.0 * rng.chisquare(2, n)) * delta).astype(np.float32)
        _check(hip_ops, x, lw, 1e-4, f"delta = {delta}")
    if n >= 4:
        holes = ((-20.0 * rng.chisquare(2, n)) * 2.0 ** -4).astype(np.float32)
        holes[::3] = -np.inf
        holes[3::6] = np.nan  # (every third entry: -inf and NaN alternate)
        m_h, _, _, _ = _check(hip_ops, x, holes, 1e-4, "holes")
        keep = np.isfinite(holes)
        r_keep = V.moments_ref([c[keep] for c in x], holes[keep])
        r_all = V.moments_ref(x, holes)
        assert r_keep[0] == r_all[0] and np.array_equal(r_keep[2], r_all[2])  # (the reference over the rest)
    none = np.full(n, -np.inf, dtype=np.float32)
    m_n, f_n, s_n, nd_n = _moments(hip_ops, x, none)
    assert np.all(m_n == 0) and np.all(f_n == 0) and np.all(s_n == 0) and nd_n == L


@pytest.mark.parametrize("n", [1000, 70001])
def test_moments_fallback_rows(hip_ops, n):
    """A duplicated column and a constant column: the fallback rows of factor_ref — the duplicate moves on its own at its own
    deviation, the constant stays put.  (The rule divides a later row by the fallback diagonal as it stands, so a row behind a
    duplicate may fall back too: whatever factor_ref says of it.)"""
    rng = np.random.default_rng(n)
    L = 5
    x = _population(n, L, rng)
    x[2] = x[0].copy()
    x[3] = np.full(n, 7.25, dtype=np.float32)
    lw = ((-20.0 * rng.chisquare(2, n)) * 2.0 ** -6).astype(np.float32)
    for w in (None, lw):
        m, f, s, nd = _moments(hip_ops, x, w)
        S = m[1 + L:]
        G, ndeg = V.factor_ref(S, L)
        assert nd == ndeg and ndeg >= 2 and np.array_equal(_bits(f), _bits(G.astype(np.float32)))
        F = V.unpack(f, L)
        c = 2.38 / np.sqrt(5.0)
        assert S[V.tri(2, 2)] == S[V.tri(0, 0)] == S[V.tri(2, 0)] and S[V.tri(3, 3)] == 0.0
        assert F[2, 0] == 0 and F[2, 1] == 0 and F[2, 2] == np.float32(c * np.sqrt(S[V.tri(2, 2)])) and F[2, 2] == s[2]
        assert np.all(F[3] == 0) and s[3] == 0 and F[4, 3] == 0 and F[4, 4] > 0 and F[1, 1] > 0 and F[1, 0] != 0


# ---- the move ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("name", MODELS)
def test_sweep_pin(hip_ops, oracle_ops, lowered, name, impl):
    """K = 3 sweeps through a fixed dense triangle, with and without an ancestors column (out-of-range words included), beta in
    {0, 0.37, 1}: x, lp, ll and n_accept are the replay's, bit for bit, and one workgroup gives the same bits.  Every case is
    conditioned ON THE REPLAY first: 10 % to 90 % accepts (the first of 64 seeds whose replay shows that)."""
    plan, assess = lowered[name]
    L = plan.n_latents
    K, F, impl_name = 3, _factor(name, L), "philox" if impl else "threefry"
    F_dev = torch.from_numpy(F).cuda()
    for n in SIZES:
        rng = np.random.default_rng(100 + n)
        cols = _start(name, n, rng)
        lp0, ll0 = assess[impl](cols)
        for with_anc in (False, True):
            anc = _ancestors(n, rng) if with_anc else None
            for beta in (0.0, 0.37, 1.0):
                for seed in range(64):
                    key = genjax.random.key(1000 + seed, impl_name)
                    ref = V.move_cov_ref(oracle_ops, assess[impl], key, cols, lp0, ll0, beta, K, F, ancestors=anc)
                    rate = ref[3].sum() / (n * K)
                    if 0.1 <= rate <= 0.9:
                        break
                else:
                    pytest.fail(f"no key with 10 % accepts and rejects in the replay: {name} n={n} beta={beta}")
                args = (plan, key, _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(), beta, K, F_dev)
                anc_d = None if anc is None else torch.from_numpy(anc).cuda()
                case = (name, impl, n, with_anc, beta)
                for kw in ({}, dict(max_workgroups=1)):
                    x, lp, ll, acc = hip_ops.temper_move_cov(*args, ancestors=anc_d, **kw)
                    assert np.array_equal(acc.cpu().numpy(), ref[3]), (case, kw)
                    for a, b in zip(x, ref[0]):
                        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b)), (case, kw)
                    assert np.array_equal(_bits(lp.cpu().numpy()), _bits(ref[1])), (case, kw)
                    assert np.array_equal(_bits(ll.cpu().numpy()), _bits(ref[2])), (case, kw)


def test_diagonal_factor_is_the_diagonal_move(hip_ops, lowered):
    """F = diag(scales) gives gjx_temper_move's outputs with those scales, bit for bit (the products with the zeros of the
    triangle add +-0 to a nonzero draw)."""
    plan, assess = lowered["regression"]
    n, K = 1025, 3
    cols = _columns("regression", n, np.random.default_rng(5))
    lp0, ll0 = assess[1](cols)
    scales = (0.8, 1.3)
    F = torch.tensor([scales[0], 0.0, scales[1]], dtype=torch.float32).cuda()
    for impl_name in ("threefry", "philox"):
        key = genjax.random.key(9, impl_name)
        args = (plan, key, _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(), 0.37, K)
        a = hip_ops.temper_move(*args, scales)
        b = hip_ops.temper_move_cov(*args, F)
        assert 0.1 <= a[3].sum().item() / (n * K) <= 0.9
        assert all(torch.equal(u, v) for u, v in zip(a[0], b[0])) and all(torch.equal(a[k], b[k]) for k in (1, 2, 3))


@pytest.mark.parametrize("D", [20, 37])
def test_plated_move(hip_ops, oracle_ops, D):
    """The plated correlated regression (37 rows: nine blocks of four and a remainder of one): one temper_move_cov call is the
    replay with plate_ref's assess, bit for bit."""
    n, K = 257, 2
    with use_ops(hip_ops):
        tracer = temper.lower(V.correlated_target(D, plated=True), 64)
        plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
    plan.set_params(tracer.params)
    data = [t.to(torch.float32) for t in tracer.data]
    plan.set_data([t.cuda() for t in data])
    rng = np.random.default_rng(D)
    model = V.correlated(D)
    sd = np.sqrt(np.diag(model.post_cov))
    cols = [(model.post_mean[k] + 3.0 * sd[k] * rng.standard_normal(n)).astype(np.float32) for k in range(2)]
    F = (2.38 / np.sqrt(2.0) * V.pack(np.linalg.cholesky(model.post_cov))).astype(np.float32)
    for impl in (0, 1):
        assess = P.Assess(oracle_ops, tracer, [t.numpy() for t in data], impl)
        lp0, ll0 = assess(cols)
        key = genjax.random.key(77, "philox" if impl else "threefry")
        ref = V.move_cov_ref(oracle_ops, assess, key, cols, lp0, ll0, 1.0, K, F)
        assert 0.1 <= ref[3].sum() / (n * K) <= 0.9
        x, lp, ll, acc = hip_ops.temper_move_cov(plan, key, _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(), 1.0, K,
                                                 torch.from_numpy(F).cuda())
        assert np.array_equal(acc.cpu().numpy(), ref[3]), (D, impl)
        assert all(np.array_equal(_bits(a.cpu().numpy()), _bits(b)) for a, b in zip(x, ref[0])), (D, impl)
        assert np.array_equal(_bits(lp.cpu().numpy()), _bits(ref[1])) and np.array_equal(_bits(ll.cpu().numpy()), _bits(ref[2])), (D, impl)


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def end_to_end(hip_ops):
    with use_ops(hip_ops):
        alg = TemperedSMC(V.correlated_target(), 4096, n_moves=2, ess_target=0.5, proposal="covariance")
        key = genjax.random.key(2024, "philox")
        return alg, key, alg.run(key), alg.run(key)


def _check_result(a, model, what):
    sd = np.sqrt(np.diag(model.post_cov))
    w, b = a.choices["w"].double().mean().item(), a.choices["b"].double().mean().item()
    print(f"{what}: stages {len(a.betas) - 1}, accept {a.accept_rate}, n_degenerate {a.n_degenerate}")
    print(f"{what}: log Z-hat {a.log_marginal_likelihood:.4f} against {model.log_z:.4f}; mean errors in posterior deviations: "
          f"w {(w - model.post_mean[0]) / sd[0]:+.3f}, b {(b - model.post_mean[1]) / sd[1]:+.3f}")
    assert abs(a.log_marginal_likelihood - model.log_z) <= LOG_Z_BOUND
    assert abs(w - model.post_mean[0]) <= 0.25 * sd[0] and abs(b - model.post_mean[1]) <= 0.25 * sd[1]
    assert len(a.n_degenerate) == len(a.betas) - 1 and all(d == 0 for d in a.n_degenerate)
    assert a.accept_rate[-1] >= 0.5 * V.COV_MIN_ACCEPT and a.accept_rate[-1] > V.DIAG_MAX_ACCEPT and a.accept_rate[-1] >= ACCEPT_FLOOR
    assert a.factor.shape == (2, 2) and a.factor.dtype == torch.float32 and a.factor.is_cuda
    f = a.factor.cpu().numpy()
    assert f[0, 1] == 0 and f[0, 0] > 0 and f[1, 1] > 0 and f[1, 0] < 0  # (w and b are negatively correlated)
    assert a.betas[0] == 0.0 and a.betas[-1] == 1.0 and all(y > x for x, y in zip(a.betas, a.betas[1:]))


def test_end_to_end_correlated_regression(hip_ops, end_to_end):
    """The correlated regression (xs = linspace(2, 3, 20): posterior correlation -0.99), n = 4096, K = 2, ESS target 0.5."""
    alg, key, a, b = end_to_end
    assert a.log_marginal_likelihood == b.log_marginal_likelihood and a.betas == b.betas and a.ess == b.ess
    assert a.accept_rate == b.accept_rate and torch.equal(a.lp, b.lp) and torch.equal(a.ll, b.ll)
    assert all(torch.equal(u, v) for u, v in zip(a.columns, b.columns))
    assert torch.equal(a.choices["w"], b.choices["w"]) and torch.equal(a.choices["b"], b.choices["b"])
    assert torch.equal(a.factor, b.factor) and a.n_degenerate == b.n_degenerate
    _check_result(a, V.correlated(), "site table")


def test_end_to_end_plated(hip_ops):
    with use_ops(hip_ops):
        res = TemperedSMC(V.correlated_target(plated=True), 4096, n_moves=2, ess_target=0.5, proposal="covariance").run(
            genjax.random.key(2025, "philox"))
    _check_result(res, V.correlated(), "plated")


def test_diagonal_route_is_unchanged(hip_ops):
    """proposal="diagonal" is the default's code path: the same bits, and no factor."""
    with use_ops(hip_ops):
        key = genjax.random.key(5, "philox")
        a = TemperedSMC(V.correlated_target(), 1000, n_moves=2).run(key)
        b = TemperedSMC(V.correlated_target(), 1000, n_moves=2, proposal="diagonal").run(key)
    assert a.log_marginal_likelihood == b.log_marginal_likelihood and a.betas == b.betas and a.accept_rate == b.accept_rate
    assert all(torch.equal(u, v) for u, v in zip(a.columns, b.columns))
    assert a.factor is None and a.n_degenerate is None and b.factor is None and b.n_degenerate is None


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
    assert coll.result.betas == a.betas and torch.equal(coll.result.factor, a.factor)


def test_launch_counts(hip_ops, lowered, end_to_end):
    """temper_moments and temper_move_cov are ONE kernel node of a captured graph each; a run makes one moments call and one
    covariance move per stage, and never calls the diagonal move after the K = 0 fill of stage 0."""
    plan, assess = lowered["regression"]
    n = 1000
    cols = _columns("regression", n, np.random.default_rng(1))
    lp0, ll0 = assess[1](cols)
    dev, lp_d, ll_d = _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda()
    lw = (ll_d * 0.01).contiguous()
    key = genjax.random.key(4, "philox")
    anc = torch.arange(n, dtype=torch.int32).cuda()
    ws = hip_ops.temper_moments_workspace(n, 2)
    F = hip_ops.temper_moments(dev, lw, ws)[1]
    hip_ops.temper_move_cov(plan, key, dev, lp_d, ll_d, 0.5, 2, F, ancestors=anc)  # (compiled before the capture)
    counts = {}
    side = torch.cuda.Stream()
    for what in ("moments", "move_cov"):
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g, stream=side):
            if what == "moments":
                out = hip_ops.temper_moments(dev, lw, ws)
            else:
                out = hip_ops.temper_move_cov(plan, key, dev, lp_d, ll_d, 0.5, 2, F, ancestors=anc)
        counts[what] = _kernel_nodes(g.raw_cuda_graph())
        g.replay()
        torch.cuda.synchronize()
        del g, out
    print("kernel nodes per call:", counts)
    assert counts == {"moments": 1, "move_cov": 1}
    alg, key, a, _ = end_to_end
    calls = {"move": 0, "move_cov": 0, "moments": 0}
    saved = {k: getattr(hip_ops, "temper_" + k) for k in calls}

    def count(name, fn):
        def wrapped(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)
        return wrapped

    for k, fn in saved.items():
        setattr(hip_ops, "temper_" + k, count(k, fn))
    try:
        with use_ops(hip_ops):
            res = alg.run(key)
    finally:
        for k in saved:
            delattr(hip_ops, "temper_" + k)
    stages = len(res.betas) - 1
    assert res.betas == a.betas and calls == {"move": 1, "move_cov": stages, "moments": stages}
