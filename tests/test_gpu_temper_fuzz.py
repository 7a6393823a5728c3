"""The tempered kernels held to float64 on the GPU (tests/temper_fuzz.py): random bodies and the fixed `interleaved` body —
latents declared after plated sites, several plated sites, a scalar observed site next to them, a plated Beta, a plated
Gamma with a data-dependent rate, a plate's value read as data — through gjx_temper_move (assess and K = 3 sweeps) and
gjx_temper_pointwise: bit for bit against the replay built from the tracer's table, AND within the derived tolerance of the
float64 evaluation of the body's own source text, which shares nothing with the lowering.  Stage 0 from temper.prior_table is
bit-equal to the oracle's, and a conjugate two-plate regression whose second latent lies between the plates runs end to end
against its closed form."""

import time

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import pointwise_ref as W
import temper_fuzz as F
import temper_ref as R
from genjax._amd import prng, temper
from genjax._amd.plan import PlanUnsupported, _make_plan
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC

pytestmark = pytest.mark.gpu

NS = (1, 257, 1000)
DS = (1, 2, 63, 64, 65, 257)  # a lone row, remainders of any unroll or 64-row chunk, one past a 256-row staging chunk
SEEDS = (21, 22, 23, 24)
BODIES = 8                    # per (seed, generator): see test_random_bodies
SCALE = {"normal": 0.3, "gamma": 0.2, "beta": 0.1}
IMPL = {0: "threefry", 1: "philox"}


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same(a, b):
    """Integer views, tolerance 0 — except that a NaN equals a NaN (its payload is the platform's, not the specification's);
    without a NaN on either side this is bit equality."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).cuda() for c in cols]


def _ancestors(n, rng):
    a = rng.integers(0, max(1, n // 2), n).astype(np.int64)  # repeats
    wild = np.array([-1, n, n + 5, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)  # out-of-range words: they clamp to n - 1
    a[rng.permutation(n)[:len(wild)]] = wild
    return a.astype(np.int32)


def _lower(hip_ops, src, args, obs, n=64):
    """-> (tracer, plan): lowered on the HIP backend from device tensors; the plan knows no length (data is set per case)."""
    with use_ops(hip_ops):
        tracer = temper.lower(F.target_of(src, args, obs, device="cuda"), n)
        plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
    if tracer.params:
        plan.set_params(tracer.params)
    return tracer, plan


def _rows(args, obs, D):
    """The first D rows of a case's columns."""
    cut = lambda v: v[:D] if isinstance(v, np.ndarray) else v  # noqa: E731
    return tuple(cut(a) for a in args), {k: cut(v) for k, v in obs.items()}


def _replay(oracle_ops, tracer, data):
    return P.Assess(oracle_ops, tracer, data) if data else R.Assess(oracle_ops, tracer)


def _assess_case(hip_ops, plan, assess, cols, impls, ref, case, times=None):
    """K = 0, recompute = 1: the GPU's (lp, ll) bit-equal to the replay's and within the derived tolerance of float64.
    `times` (a list): the seconds of every launch, its results read back, are appended."""
    lp_ref, ll_ref = assess(cols)
    worst = 0.0
    for impl in impls:
        t0 = time.time()
        x, lp, ll, acc = hip_ops.temper_move(plan, genjax.random.key(3, IMPL[impl]), _dev(cols), None, None, 0.37, 0, None, recompute=True)
        lp, ll = lp.cpu().numpy(), ll.cpu().numpy()
        if times is not None:
            times.append(time.time() - t0)
        assert all(_same(a.cpu().numpy(), b) for a, b in zip(x, cols)), case
        assert _same(lp, lp_ref), (case, impl, lp[:4], lp_ref[:4])
        assert _same(ll, ll_ref), (case, impl, ll[:4], ll_ref[:4])
        assert int(acc.sum()) == 0
        if ref is not None:
            worst = max(worst, F.check64(lp, what="lp", ref=ref, context=str(case)), F.check64(ll, what="ll", ref=ref, context=str(case)))
    return worst, lp_ref, ll_ref


def _sweep_case(hip_ops, oracle_ops, plan, assess, cols, scales, impl, seed, case, grids=(0,)):
    """K = 3 sweeps through an ancestors column with repeats and out-of-range words: temper_ref.move_ref's, bit for bit."""
    n, K, beta = len(cols[0]), 3, 0.37
    rng = np.random.default_rng(seed)
    lp0, ll0 = assess(cols)
    anc = _ancestors(n, rng)
    key = genjax.random.key(1000 + seed, IMPL[impl])
    ref = R.move_ref(oracle_ops, assess, key, cols, lp0, ll0, beta, K, scales, ancestors=anc)
    assert 0 < int(ref[3].sum()) < n * K, case  # the replay accepts some proposals and rejects some
    for wg in grids:
        x, lp, ll, acc = hip_ops.temper_move(plan, key, _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(), beta, K,
                                             scales, ancestors=torch.from_numpy(anc).cuda(), max_workgroups=wg)
        assert np.array_equal(acc.cpu().numpy(), ref[3]), (case, wg)
        assert all(_same(a.cpu().numpy(), b) for a, b in zip(x, ref[0])), (case, wg)
        assert _same(lp.cpu().numpy(), ref[1]) and _same(ll.cpu().numpy(), ref[2]), (case, wg)


def _pointwise_case(got, t, case, min_share=0.0):
    """got float64 [4, D] against the float64 reductions of the replay's terms t [D, n], at pointwise_ref's tolerances, on the
    rows whose terms are finite and spread less than LSE_MAX_SPREAD -> the share of such rows."""
    ref = W.reduce64(t)
    b1, b2 = W.moment_bounds(t)
    rows = np.flatnonzero(np.isfinite(t).all(axis=1) & (W.spread(t) < W.LSE_MAX_SPREAD))
    share = len(rows) / t.shape[0]
    assert share >= min_share, (case, share)
    assert np.array_equal(got[3], ref[3]), case
    if len(rows):
        with np.errstate(invalid="ignore"):  # (rows left out of `rows` may hold infinities)
            e0, e1, e2 = (np.abs(got[k] - ref[k])[rows] for k in range(3))
        assert np.all(e0 <= W.LSE_TOL), (case, e0.max())
        assert np.all(e1 <= b1[rows]) and np.all(e2 <= b2[rows]), case
    return share


# ---- random bodies ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("seed", SEEDS)
def test_random_bodies(hip_ops, oracle_ops, seed, impl):
    """BODIES = 8 random bodies per (seed, generator) — the first of the seed's stream that lower and whose references (the
    wide population's and the centred one's, at both sizes) are conditioned; the shares of the others are asserted on 200 bodies
    by tests/test_temper_fuzz_cpu.py — at n = 257 and at BOTH D = 65 and D = 2 (a body without a plated site has no rows: once):
    assess bit-equal to the replay and within the derived tolerance of float64; K = 3 sweeps bit-equal to temper_ref.move_ref
    with the plated assess; for plated bodies the pointwise outputs at pointwise_ref's tolerances on a centred population, and
    that population's terms within the derived tolerance of float64.
    Each body costs one compilation of its move kernel per generator and one of its pointwise kernel.  Measured on an MI355X
    machine: a body's first move launch, compilation included and the replay not, 0.20 to 0.50 s; a whole test of eight bodies
    2.1 to 4.8 s, under the 10 s a test may take: BODIES = 8.  The times of a run are printed."""
    n, sizes = 257, (65, 2)
    rng = np.random.default_rng(seed)
    done, attempts, worst, refused, t_launch, n_terms = 0, 0, 0.0, [], [], 0
    while done < BODIES and attempts < 3 * BODIES:
        attempts += 1
        src, sites = F.random_tempered_model(rng)
        args, obs = F.random_inputs(rng, sites, max(sizes))
        latents = F.latent_columns(rng, sites, n)
        centred = F.latent_columns(rng, sites, n, centred=True)
        plated = any(role == "plated" for _, role, _ in sites)
        Ds = sizes if plated else sizes[:1]
        refs = {D: F.Reference(src, latents, _rows(args, obs, D)[1], _rows(args, obs, D)[0]) for D in Ds}
        crefs = {D: F.Reference(src, centred, _rows(args, obs, D)[1], _rows(args, obs, D)[0]) for D in Ds} if plated else {}
        reasons = sum((r.reasons for r in list(refs.values()) + list(crefs.values())), [])
        if reasons:
            refused.append("dropped: " + "; ".join(reasons))
            continue
        try:
            tracer, plan = _lower(hip_ops, src, args, obs)
        except PlanUnsupported as e:
            refused.append(f"unlowered: {e}")
            continue
        assert [m["addr"] for m in tracer.meta] == [s[0] for s in sites] and bool(tracer.data) == plated
        cols, ccols = F.columns_of(tracer, latents), F.columns_of(tracer, centred)
        scales = [SCALE[k] for _, role, k in sites if role == "latent"]
        for D in Ds:
            case = f"seed {seed} body {attempts} impl {impl} D {D}\n{src}\nargs {args[3:]}"
            data = F.data_of(tracer, D)
            if data:
                plan.set_data(_dev(data))
            assess = _replay(oracle_ops, tracer, data)
            times = []
            w, _, _ = _assess_case(hip_ops, plan, assess, cols, (impl,), refs[D], case, times=times)
            if D == Ds[0]:
                t_launch += times  # (the first launch of the body under this generator: its compilation)
            worst = max(worst, w)
            _sweep_case(hip_ops, oracle_ops, plan, assess, cols, scales, impl, seed, case)
            if plated:
                t = W.terms(assess, ccols)
                got = hip_ops.temper_pointwise(plan, _dev(ccols)).cpu().numpy()
                _pointwise_case(got, t, case, min_share=0.9)
                worst = max(worst, F.check64(t, what="terms", ref=crefs[D], context=case))
                n_terms += 1
        done += 1
    print(f"seed {seed} {IMPL[impl]}: {done} bodies of {attempts} generated; {n_terms} pointwise tables compared with float64; worst err / tol "
          f"{worst:.3f}; first move launch of a body (compilation included) {min(t_launch, default=0):.2f} .. {max(t_launch, default=0):.2f} s")
    for r in refused:
        print("  ", r)
    assert done == BODIES


# ---- the interleaved body --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interleaved(hip_ops):
    rng = np.random.default_rng(77)
    args, obs = F.random_inputs(rng, F.INTERLEAVED_SITES, max(DS))
    tracer, plan = _lower(hip_ops, F.INTERLEAVED, args, obs)
    assert [m["addr"] for m in tracer.meta] == [s[0] for s in F.INTERLEAVED_SITES] and len(tracer.sites) == 9
    return dict(args=args, obs=obs, tracer=tracer, plan=plan, scales=[SCALE[k] for _, role, k in F.INTERLEAVED_SITES if role == "latent"])


def _interleaved_case(c, oracle_ops, D, inf_row=False):
    """Data of D rows set on the plan -> (the replay's assess, the data columns).  `inf_row`: one +inf value in y1's column —
    set on the plan's data after the lowering, so the column 1 + y1 * y1 (computed when the body was traced) stays finite."""
    data = F.data_of(c["tracer"], D)
    if inf_row:
        k = next(i for i, col in enumerate(data) if np.array_equal(col, c["obs"]["y1"][:D]))
        data[k][D // 2] = np.inf
    c["plan"].set_data(_dev(data))
    return P.Assess(oracle_ops, c["tracer"], data), data


def test_interleaved_assess(hip_ops, oracle_ops, interleaved):
    """n in {1, 257, 1000} x D in {1, 2, 63, 64, 65, 257}, both generators: bit-equal to the replay and within the derived
    tolerance of float64."""
    c, rng, worst = interleaved, np.random.default_rng(31), 0.0
    for D in DS:
        assess, _ = _interleaved_case(c, oracle_ops, D)
        args, obs = _rows(c["args"], c["obs"], D)
        for n in NS:
            latents = F.latent_columns(rng, F.INTERLEAVED_SITES, n)
            ref = F.Reference(F.INTERLEAVED, latents, obs, args)
            assert ref.kept or n == 1, (n, D, ref.reasons)
            w, _, _ = _assess_case(hip_ops, c["plan"], assess, F.columns_of(c["tracer"], latents), (0, 1), ref, ("interleaved", n, D))
            worst = max(worst, w)
    print(f"interleaved assess: worst err / tol {worst:.3f}")


@pytest.mark.parametrize("impl", [0, 1])
def test_interleaved_sweeps(hip_ops, oracle_ops, interleaved, impl):
    """K = 3 sweeps at n = 257, D = 65, whatever the grid."""
    c = interleaved
    assess, _ = _interleaved_case(c, oracle_ops, 65)
    latents = F.latent_columns(np.random.default_rng(32), F.INTERLEAVED_SITES, 257)
    _sweep_case(hip_ops, oracle_ops, c["plan"], assess, F.columns_of(c["tracer"], latents), c["scales"], impl, 5, ("interleaved", impl), grids=(0, 1, 7))


def test_interleaved_pointwise(hip_ops, oracle_ops, interleaved):
    """The four plated sites' terms summed in f32 in table order, reduced over the particles: against float64 reductions of the
    replay's terms, and those terms within the derived tolerance of float64."""
    c, rng, worst = interleaved, np.random.default_rng(33), 0.0
    for D in DS:
        assess, _ = _interleaved_case(c, oracle_ops, D)
        args, obs = _rows(c["args"], c["obs"], D)
        for n in NS:
            latents = F.latent_columns(rng, F.INTERLEAVED_SITES, n, centred=True)
            cols = F.columns_of(c["tracer"], latents)
            t = W.terms(assess, cols)
            assert t.shape == (D, n)
            got = hip_ops.temper_pointwise(c["plan"], _dev(cols)).cpu().numpy()
            _pointwise_case(got, t, ("interleaved", n, D), min_share=0.9)
            ref = F.Reference(F.INTERLEAVED, latents, obs, args)
            worst = max(worst, F.check64(t, what="terms", ref=ref, context=str((n, D))))
    print(f"interleaved pointwise terms: worst err / tol {worst:.3f}")


def test_interleaved_inf_row(hip_ops, oracle_ops, interleaved):
    """One +inf observed value in y1: ll = -inf for every particle, that row's lse -inf and count 0."""
    c, n, D = interleaved, 257, 65
    assess, _ = _interleaved_case(c, oracle_ops, D, inf_row=True)
    latents = F.latent_columns(np.random.default_rng(34), F.INTERLEAVED_SITES, n, centred=True)
    cols = F.columns_of(c["tracer"], latents)
    _, lp_ref, ll_ref = _assess_case(hip_ops, c["plan"], assess, cols, (0, 1), None, "inf_row")
    assert np.isfinite(lp_ref).all() and np.isneginf(ll_ref).all()
    t = W.terms(assess, cols)
    r = D // 2
    assert np.isneginf(t[r]).all() and np.isfinite(np.delete(t, r, axis=0)).all()
    got = hip_ops.temper_pointwise(c["plan"], _dev(cols)).cpu().numpy()
    assert got[0][r] == -np.inf and got[3][r] == 0.0 and got[1][r] == -np.inf and got[2][r] == np.inf
    assert _pointwise_case(got, t, "inf_row") == (D - 1) / D


def test_interleaved_outside_support(hip_ops, oracle_ops, interleaved):
    """Every fourth Gamma / Beta latent value outside its support: lp = -inf there, exactly as float64 has it; the NaN terms
    (a negative Gamma shape) reach s1 and s2 of their rows and not the lse or the count."""
    c, n, D = interleaved, 1000, 65
    assess, _ = _interleaved_case(c, oracle_ops, D)
    args, obs = _rows(c["args"], c["obs"], D)
    latents = F.latent_columns(np.random.default_rng(35), F.INTERLEAVED_SITES, n, outside=True)
    ok = F.inside(F.INTERLEAVED_SITES, latents)
    cols = F.columns_of(c["tracer"], latents)
    ref = F.Reference(F.INTERLEAVED, latents, obs, args, live=ok)
    assert ref.kept, ref.reasons
    worst, lp_ref, _ = _assess_case(hip_ops, c["plan"], assess, cols, (0, 1), ref, "outside")
    assert (~ok).sum() >= n // 4 and np.all(np.isneginf(lp_ref[~ok]) | np.isnan(lp_ref[~ok])) and np.isneginf(lp_ref).sum() >= n // 8
    assert np.isfinite(lp_ref[ok]).all()
    t = W.terms(assess, cols)
    bad = np.isnan(t)
    assert bad.any() and not bad[:, ok].any()
    got = hip_ops.temper_pointwise(c["plan"], _dev(cols)).cpu().numpy()
    nan_rows = bad.any(axis=1)
    assert np.array_equal(np.isnan(got[1]), nan_rows) and np.array_equal(np.isnan(got[2]), nan_rows)
    live = np.where(t > -np.inf, t, -np.inf)  # (false on NaN: those entries leave)
    lref = W.reduce64(live)
    assert np.array_equal(got[3], lref[3]) and np.array_equal(got[3], n - (bad | np.isneginf(t)).sum(axis=1))
    rows = W.spread(live) < W.LSE_MAX_SPREAD
    assert rows.mean() >= 0.9 and np.all(np.abs(got[0] - lref[0])[rows] <= W.LSE_TOL)
    print(f"outside support: worst err / tol {worst:.3f}; rows with NaN terms {int(nan_rows.sum())} of {D}")


# ---- stage 0 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1])
def test_stage0_parity(hip_ops, oracle_ops, interleaved, impl):
    """The prior_table plan of `interleaved` through the importance kernel as TemperedSMC.run calls it: every latent column
    bit-equal to the oracle's on the same table and keys (its distribution is checked in tests/test_temper_fuzz_cpu.py)."""
    tr = interleaved["tracer"]
    pt = temper.prior_table(tr)
    key = genjax.random.key(2026, IMPL[impl])
    for n in (257, 20000):
        out = []
        for ops in (hip_ops, oracle_ops):
            with use_ops(ops):
                plan = _make_plan(pt)
                vals = ops.importance_run(plan, prng.split_lazy(prng.fold_in(key, 0), n), n, [], [torch.float32] * tr.n_out,
                                          want_score=False, want_max_partials=False)[0]
            out.append([v.cpu().numpy().copy() for v in vals])
        assert len(out[0]) == len(out[1]) == 4
        for k, (a, b) in enumerate(zip(*out)):
            assert not np.isnan(b).any() and np.array_equal(_bits(a), _bits(b)), (n, impl, k)


# ---- end to end through the renumbering path --------------------------------------------------------------------------------
def test_end_to_end_two_plate_regression(hip_ops):
    """w ~ N(0, 2); y1 ~ N(w xs, 0.2) plated; b ~ N(0, 2) declared BETWEEN the plates; y2 ~ N(w zs + b, 0.3) plated; D = 200,
    n = 4096, K = 2: two runs from one key are bit-equal; log Z and the posterior means and deviations of (w, b) within FOUR
    TIMES the spread of the float64 restatement on this model (tests/plate_ref.py: measured on the CPU over 24 seeds)."""
    model = P.two_plate()
    xs, zs, y1, y2 = P.two_plate_data()
    with use_ops(hip_ops):
        alg = TemperedSMC(F.target_of(P.TWO_PLATE, (xs, zs), {"y1": y1, "y2": y2}, device="cuda"), 4096, n_moves=2)
        key = genjax.random.key(2027, "philox")
        a, b = alg.run(key), alg.run(key)
    assert a.log_marginal_likelihood == b.log_marginal_likelihood and a.betas == b.betas and a.accept_rate == b.accept_rate
    assert torch.equal(a.lp, b.lp) and torch.equal(a.ll, b.ll) and all(torch.equal(u, v) for u, v in zip(a.columns, b.columns))
    sd = np.sqrt(np.diag(model.post_cov))
    w, bb = a.choices["w"].double(), a.choices["b"].double()
    em = [(w.mean().item() - model.post_mean[0]) / sd[0], (bb.mean().item() - model.post_mean[1]) / sd[1]]
    es = [w.std().item() / sd[0] - 1.0, bb.std().item() / sd[1] - 1.0]
    ez = a.log_marginal_likelihood - model.log_z
    print(f"stages {len(a.betas) - 1}, accept {a.accept_rate}")
    print(f"log Z-hat {a.log_marginal_likelihood:.4f} against {model.log_z:.4f} (error {ez:+.4f}, bound {P.E2E_FACTOR * P.TWO_PLATE_SPREAD_LOG_Z:.4f}); "
          f"mean errors / sd {em[0]:+.4f} {em[1]:+.4f}; sd errors {es[0]:+.4f} {es[1]:+.4f}")
    assert a.betas[0] == 0.0 and a.betas[-1] == 1.0 and all(y > x for x, y in zip(a.betas, a.betas[1:]))
    assert abs(ez) <= P.E2E_FACTOR * P.TWO_PLATE_SPREAD_LOG_Z
    assert all(abs(e) <= P.E2E_FACTOR * s for e, s in zip(em, P.TWO_PLATE_SPREAD_MEAN))
    assert all(abs(e) <= P.E2E_FACTOR * s for e, s in zip(es, P.TWO_PLATE_SPREAD_SD))
