"""The HIP library's Gamma, Beta, Normal and Bernoulli sites against the CPU oracle, bit for bit, over the whole parameter range
of dist_range_ref.py (shapes 0.01 .. 1e4; test_dist_range_cpu.py pins that oracle against float64): per-site kernels,
importance plans on every kernel route, a scan plan and a generated SMC filter, with shapes entering as scalars, per-particle
columns, launch parameters, literals and earlier draws — so draws that are 0, subnormal or 1, both sides of the `conc < 1`
boost and of m_lgamma's branch at 8 in NEIGHBOURING lanes, and the log-space branch of beta_from_gammas all run on the device.
Then the float64 truth through the device's own log-densities, and the fast-math plans on Gamma and Beta sites."""

import numpy as np
import pytest
import torch

import dist_range_ref as R
from genjax._amd import prng, workloads as W
from genjax._amd.ops import KeyBatch

pytestmark = pytest.mark.gpu

IMPLS = [0, 1]
SIZES = [4099, 70004]  # ragged (a short last row, no quads) / the four-particles-per-lane form


def dev(t, ops):
    return t.to(ops.device()).contiguous()


def same(a, b, what):
    """Bit for bit; a NaN (invalid shapes only: a Gamma draw of 0 used as a shape) on both sides, whatever its sign."""
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype.is_floating_point:
        nan = a.isnan()
        ok = torch.equal(nan, b.isnan()) and torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32))
    else:
        ok = torch.equal(a, b)
    if not ok:
        bad = ((a != b) & ~(a.isnan() & b.isnan()) if a.dtype.is_floating_point else a != b).flatten().nonzero().flatten()
        raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} differ, first at {bad[:5].tolist()}: "
                             f"{a.flatten()[bad[:5]].tolist()} vs {b.flatten()[bad[:5]].tolist()}")


def site_parity(hip_ops, oracle_ops, dist, kb, n, a, b, what, valid=True):
    dv = lambda x: dev(x, hip_ops) if isinstance(x, torch.Tensor) else x  # noqa: E731
    hv, hs = hip_ops.sample_logpdf(dist, kb, n, dv(a), dv(b))
    ov, os_ = oracle_ops.sample_logpdf(dist, kb, n, a, b)
    same(hv, ov, f"{what} value")
    same(hs, os_, f"{what} score")
    hl = hip_ops.logpdf(dist, n, hv, dv(a), dv(b))
    same(hl, oracle_ops.logpdf(dist, n, ov, a, b), f"{what} logpdf")
    same(hl, hs, f"{what} logpdf == fused score")
    if valid:
        assert not bool(hv.isnan().any()) and not bool(hs.isnan().any()), f"{what}: NaN for valid parameters"
    return hv


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", SIZES)
def test_site_ops_on_the_scalar_grid(hip_ops, oracle_ops, impl, n):
    kb = KeyBatch(impl, 1, parent=(31, 32), first=0).with_fold(2)
    for a, r in R.gamma_density_params():
        v = site_parity(hip_ops, oracle_ops, "gamma", kb, n, R.f32(a), R.f32(r), f"gamma({a}, {r})")
        assert bool((v >= 0).all())
    for a, b in R.BETA_PAIRS:
        v = site_parity(hip_ops, oracle_ops, "beta", kb, n, R.f32(a), R.f32(b), f"beta({a}, {b})")
        assert bool(((v >= 0) & (v <= 1)).all())
    for p in R.BERNOULLI_P:
        site_parity(hip_ops, oracle_ops, "bernoulli", kb, n, R.f32(p), None, f"bernoulli({p})")
    for sc in R.NORMAL_SCALES:
        for loc in R.NORMAL_LOCS:
            site_parity(hip_ops, oracle_ops, "normal", kb, n, R.f32(loc), R.f32(sc), f"normal({loc}, {sc})")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("n", SIZES)
def test_site_ops_with_per_particle_shapes(hip_ops, oracle_ops, impl, n):
    """Shapes log-spaced over [0.01, 1e4] with a period of 61 lanes: every wave mixes boost and non-boost lanes, both lgamma
    branches, flushed and ordinary draws."""
    kb = KeyBatch(impl, 1, parent=(33, 34), first=10).with_fold(1)
    sh, a, b, x = R.input_columns(n)
    rate = torch.tensor(R.RATES, dtype=torch.float32)[torch.arange(n) % 3]
    site_parity(hip_ops, oracle_ops, "gamma", kb, n, sh, rate, "gamma, per-particle shapes")
    v = site_parity(hip_ops, oracle_ops, "beta", kb, n, a, b, "beta, per-particle shapes")
    assert bool(((v >= 0) & (v <= 1)).all())
    p = torch.tensor(R.BERNOULLI_P, dtype=torch.float32)[torch.arange(n) % len(R.BERNOULLI_P)]
    site_parity(hip_ops, oracle_ops, "bernoulli", kb, n, p, None, "bernoulli, per-particle p")
    sc = torch.tensor(R.NORMAL_SCALES, dtype=torch.float32)[torch.arange(n) % 5]
    loc = torch.tensor(R.NORMAL_LOCS, dtype=torch.float32)[torch.arange(n) % 3]
    site_parity(hip_ops, oracle_ops, "normal", kb, n, loc, sc, "normal, per-particle scale")


def test_log_densities_against_float64_on_the_device(hip_ops):
    R.check_logpdf_grid(hip_ops)


# ---- importance plans ----------------------------------------------------------------------------------------------------------

ROUTES = [("specialized", 0), ("specialized", 1), ("pair", 1), ("interpreter", 0), ("interpreter", 1)]


@pytest.fixture(params=ROUTES, ids=[f"{m}-impl{i}" for m, i in ROUTES])
def route(request, monkeypatch):
    """The routes of test_gpu_parity_abi.plan_mode, per generator: the specialised kernel (Philox: four particles per lane
    where n allows), two particles per lane (GJX_JIT_FORM chooses among the Philox kernels only: Threefry has the one kernel
    of 'specialized'), and the site-table interpreter."""
    mode, impl = request.param
    monkeypatch.setenv("GJX_PLAN_JIT", "0" if mode == "interpreter" else "1")
    if mode == "pair":
        monkeypatch.setenv("GJX_JIT_FORM", "pair")
    else:
        monkeypatch.delenv("GJX_JIT_FORM", raising=False)
    return mode, impl


_ORACLE = {}


def oracle_importance(oracle_ops, kind, impl, n, row):
    """The oracle's pass (computed once per case, shared between the routes and the fast-math test, never modified)."""
    k = (kind, impl, n, row)
    if k not in _ORACLE:
        sites, dts = R.importance_sites(kind)
        plan = oracle_ops.plan_create(sites)
        plan.set_params(list(R.PARAM_ROWS[row]))
        kb = W.importance_particle_keys(prng.key(50 + row, impl), n)
        vals, score, logw, mp, rows = oracle_ops.importance_run(plan, kb, n, R.input_columns(n), dts, want_rows=True)
        _ORACLE[k] = vals + [score, logw, mp, rows.e, rows.s]
    return _ORACLE[k]


def hip_importance(hip_ops, plan, kind, impl, n, row):
    _, dts = R.importance_sites(kind)
    plan.set_params(list(R.PARAM_ROWS[row]))
    kb = W.importance_particle_keys(prng.key(50 + row, impl), n)
    vals, score, logw, mp, rows = hip_ops.importance_run(plan, kb, n, [dev(c, hip_ops) for c in R.input_columns(n)], dts, want_rows=True)
    return vals + [score, logw, mp, rows.e, rows.s]


OUTPUTS = ["score", "logw", "row maxima", "row anchors", "row sums"]


@pytest.mark.parametrize("kind", R.IMPORTANCE_KINDS)
def test_importance_plans(hip_ops, oracle_ops, kind, route):
    """Every output the parity fuzz compares — values, score, log-weights, row maxima, row anchors, row sums.  One compiled
    kernel per (plan, route) serves the whole grid: shapes are columns and launch parameters."""
    plan_mode, impl = route
    sites, dts = R.importance_sites(kind)
    plan = hip_ops.plan_create(sites)
    for n in SIZES:
        for row in range(len(R.PARAM_ROWS) if kind == "inputs" else 1):
            got = hip_importance(hip_ops, plan, kind, impl, n, row)
            want = oracle_importance(oracle_ops, kind, impl, n, row)
            names = [f"value column {i}" for i in range(len(dts))] + OUTPUTS
            for g, w, nm in zip(got, want, names):
                same(g, w, f"{kind} {plan_mode} impl {impl} n {n} params {R.PARAM_ROWS[row]}: {nm}")
            if kind != "site_shape":  # (there a Gamma draw of 0 is a shape: Beta(0, b) is invalid, NaN on both sides)
                for g in got[:len(dts)]:
                    assert not bool(g.isnan().any())
                beta = got[1]
                assert bool(((beta >= 0) & (beta <= 1)).all())


# ---- a scan plan and a generated SMC filter: Gamma(0.05, .) and Beta(0.05, 0.05) feed the carry -----------------------------------

T_STEPS = 4


def _obs():
    return np.random.default_rng(5).uniform(-1, 1, (T_STEPS, 1)).astype(np.float32)


@pytest.mark.parametrize("impl", IMPLS)
def test_scan_plan(hip_ops, oracle_ops, impl):
    outs = {}
    for n in SIZES:
        kb = W.importance_particle_keys(prng.key(60, impl), n)
        for ops in (hip_ops, oracle_ops):
            plan = ops.scan_plan_create(R.carry_sites(False), R.carry_next(), 1)
            o = ops.scan_run(plan, kb, n, T_STEPS, _obs(), [0.5, 0.25], [torch.float32, torch.float32])
            outs[ops is hip_ops] = o["values"] + o["carry"] + [o["score"], o["logw"], o["max_partials"], o["rows"].e, o["rows"].s]
        for i, (g, w) in enumerate(zip(outs[True], outs[False])):
            same(g, w, f"scan output {i}, impl {impl}, n {n}")
        for g in outs[True][:4]:
            assert not bool(g.isnan().any())
        assert bool(((outs[True][1] >= 0) & (outs[True][1] <= 1)).all())


@pytest.mark.parametrize("ess", [0.0, 0.5])
@pytest.mark.parametrize("impl", IMPLS)
def test_generated_smc_filter(hip_ops, oracle_ops, impl, ess):
    sk, rk = W.smc_key_schedule(prng.key(61, impl), T_STEPS)
    for n in SIZES:
        outs = []
        for ops in (hip_ops, oracle_ops):
            plan = ops.smc_plan_create(R.carry_sites(True), R.carry_sites(False), R.carry_next(), R.carry_next(), 1)
            r = ops.smc_run_plan(plan, impl, n, sk, rk, _obs(), True, ess_threshold=ess, want_flags=True)
            outs.append([r[0], r[1], *r[2], r[3], r[4]] + ([r[5]] if r[5] is not None else []))
        for i, (g, w) in enumerate(zip(*outs)):
            same(g, w, f"smc output {i}, impl {impl}, n {n}, ess {ess}")
        state = outs[0][2:4]
        assert not bool(state[0].isnan().any()) and bool(((state[1] >= 0) & (state[1] <= 1)).all())


# ---- fast math ------------------------------------------------------------------------------------------------------------------

SUBNORMAL_CAP = 0.005


@pytest.mark.parametrize("form", ["pair", "quad", "one"])
def test_fast_math_on_gamma_and_beta_sites(hip_ops, oracle_ops, form, monkeypatch):
    """GJX_PLAN_FAST_MATH on the 'inputs' plan, under the contract of test_importance_fast_math_tolerance: scores and
    log-weights within 1e-5 relative of the oracle, values within 1e-5 relative or 2e-6 absolute, the same particles decided.
    Where the oracle's draw is 0 or 1 the fast plan draws the same value, and where the oracle's score or log-weight is
    infinite the fast plan's is the same infinity.  Particles one of whose oracle draws is SUBNORMAL are left out of the
    tolerance (the hardware log flushes a subnormal argument): their share is capped at 0.5 %.  Counted on the oracle it is
    1.0e-4 of the 70004 particles (7) and none of the 4099."""
    monkeypatch.setenv("GJX_PLAN_JIT", "1")
    monkeypatch.setenv("GJX_JIT_FORM", form)
    sites, dts = R.importance_sites("inputs")
    plan = hip_ops.plan_create(sites, fast_math=True)
    tiny = float(np.finfo(np.float32).tiny)
    for n in SIZES:
        got = [t.cpu() for t in hip_importance(hip_ops, plan, "inputs", 1, n, 0)]
        want = oracle_importance(oracle_ops, "inputs", 1, n, 0)
        nv = len(dts)
        sub = torch.zeros(n, dtype=torch.bool)
        for w, dt in zip(want[:nv], dts):
            if dt == torch.float32:
                sub |= (w != 0) & (w.abs() < tiny)
        share = float(sub.double().mean())
        print(f"form {form} n {n}: subnormal share {share:.3g}")
        assert share <= SUBNORMAL_CAP
        keep = ~sub
        for i, (g, w, dt) in enumerate(zip(got[:nv], want[:nv], dts)):
            if dt != torch.float32:
                assert torch.equal(g, w), f"column {i}: other particles decided"
                continue
            edge = (w == 0) | (w == 1)
            assert torch.equal(g[edge], w[edge]), f"column {i}: a draw of 0 or 1"
            err = (g.double() - w.double()).abs()[keep]
            ok = (err <= 1e-5 * w.double().abs()[keep]) | (err <= 2e-6)
            print(f"  column {i}: max abs deviation {float(err.max()):.3g}")
            assert bool(ok.all()), f"column {i}: max abs deviation {float(err.max()):.3g}"
        for g, w, nm in zip(got[nv:nv + 2], want[nv:nv + 2], OUTPUTS):
            inf = ~w.isfinite()
            same(g[inf], w[inf], f"{nm} where the oracle's is not finite")
            fin = keep & ~inf
            rel = ((g.double() - w.double()).abs()[fin] / w.double().abs()[fin].clamp_min(1e-30))
            worst = int(rel.argmax())
            print(f"  {nm}: max relative deviation {float(rel.max()):.3g} ({float(g[fin][worst])!r} vs {float(w[fin][worst])!r})")
            assert float(rel.max()) <= 1e-5, f"{nm}: max relative deviation {float(rel.max()):.3g}"
