"""PSIS-LOO on the GPU (include/gjx_psis.h): the selected tail bit for bit against np.sort under the header's key, the body sum
within the bound of an f32 exponential, the fit and the estimate held to the float64 numpy restatement (tests/psis_ref.py) at a
measured multiple of reordering noise, rows that are not smoothed, non-finite entries, k-hat on both sides of the scale,
determinism, and the public call end to end against the closed-form leave-one-out of the conjugate regression."""

import math

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import pointwise_ref as W
import psis_ref as S
from genjax import ChoiceMap, Target
from genjax._amd import temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PSISLOO, PointwiseLikelihood, TemperedSMC

pytestmark = pytest.mark.gpu

MODELS = P.MODELS + ("two_plate",)
# (model, n, D, population): n = 4096 (M = 192, sixteen chunks), 4099 (M = 193, a short last chunk), 25 (M = 5, one chunk: the
# stored histogram); D = 5 (a partial row block), 64, 300 (75 row blocks)
CASES = [(name, 4096, 64, "centred") for name in MODELS] + [
    ("normal", 4099, 5, "centred"), ("normal", 25, 300, "centred"), ("logistic", 25, 5, "centred"),
    ("normal", 4096, 300, "dup"), ("two_plate", 4099, 64, "dup"), ("gamma_rate", 25, 64, "dup"),
]


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


def _f32(t):
    return t.detach().to(torch.float32).numpy().copy()


def lower_all(ops):
    """Per model: (tracer, plan, order) lowered once, from 20 rows — the plan knows no length: data of any D is set per case.
    `order`: the plan's data columns as positions in the case's (arguments, then observed values)."""
    import temper_fuzz as F

    out = {}
    with use_ops(ops):
        for name in MODELS:
            if name == "two_plate":
                given = P.two_plate_data(20, 0)
                target = F.target_of(P.TWO_PLATE, given[:2], {"y1": given[2], "y2": given[3]})
            else:
                target, given = P.target(name, 20)
                given = [_f32(t) for t in given]
            tracer = temper.lower(target, 64)
            order = [next(k for k, g in enumerate(given) if np.array_equal(g, c)) for c in F.data_of(tracer)]
            plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            if tracer.params:
                plan.set_params(tracer.params)
            out[name] = (tracer, plan, order)
    return out


def case_data(lowered, name, D):
    """The case's data columns in the plan's column order, f32 numpy [D]."""
    if name == "two_plate":
        given = [np.ascontiguousarray(c) for c in P.two_plate_data(D, 1)]
    else:
        given = [_f32(t)[:D] for t in P.target(name, max(D, 2), seed=1)[1]]
    return [given[k] for k in lowered[name][2]]


def population(name, n, kind, rng, width=0.1):
    """centred: pointwise_ref.centred_columns (both signs, several exponents per row); dup: 1500 distinct particles (fewer
    below n = 1500) resampled to n, so that the cutoff is tied; same: n copies of one particle."""
    base = "normal" if name == "two_plate" else name
    if kind == "centred":
        return W.centred_columns(base, n, rng, width)
    m = 1 if kind == "same" else min(1500, max(n // 3, 2))
    cols = W.centred_columns(base, m, rng, width)
    idx = rng.integers(0, m, n)
    return [np.ascontiguousarray(c[idx]) for c in cols]


@pytest.fixture(scope="module")
def lowered(hip_ops):
    return lower_all(hip_ops)


def _run(hip_ops, oracle_ops, lowered, name, D, cols, data=None, M=None):
    """-> (out [7, D], tail [D, M + 1] from the GPU, the oracle's terms t [D, n], M); two calls, equal bits.  `M`: a tail
    length of the caller's choice (tests/test_gpu_psis_shapes.py) in place of the package's rule."""
    tracer, plan, _ = lowered[name]
    data = case_data(lowered, name, D) if data is None else data
    plan.set_data(_dev(data))
    n = len(cols[0])
    if M is None:
        M = S.tail_len(n)
        assert M == int(hip_ops.lib.call("gjx_psis_tail_len", n, 1.0))
    t = W.terms(P.Assess(oracle_ops, tracer, data), cols)
    assert t.shape == (D, n)
    dev = _dev(cols)
    out, tail = hip_ops.temper_psis(plan, dev, M, want_tail=True)
    out2, tail2 = hip_ops.temper_psis(plan, dev, M, want_tail=True)
    assert out.shape == (7, D) and out.dtype == torch.float64 and tail.shape == (D, M + 1) and tail.dtype == torch.float32
    assert torch.equal(out.view(torch.int64), out2.view(torch.int64)) and torch.equal(tail.view(torch.int32), tail2.view(torch.int32))
    only, none = hip_ops.temper_psis(plan, dev, M)
    assert none is None and torch.equal(only.view(torch.int64), out.view(torch.int64))
    return out.cpu().numpy(), tail.cpu().numpy(), t, M


def _check(out, tail, t, M, case, tol=None):
    """The GPU's outputs against the reference on the terms t.  The fit is float64 arithmetic on bit-identical inputs: the
    reference's is evaluated on the tail (equal bit for bit) and on the GPU's OWN body sum, which has its own bound.
    `tol`: psis_ref.TOL, or the table measured for the caller's cases (psis_ref.TOL_LARGE)."""
    tol = S.TOL if tol is None else tol
    n = t.shape[1]
    ref = S.psis(t, M)
    # (value for value where both are numbers, as before; key for key — the header's order: every NaN one key, -0 below +0 —
    # so that a tail that HOLDS NaNs compares too; the device returns a NaN as 0x7FFFFFFF)
    nan = np.isnan(ref["tail"])
    assert np.array_equal(tail[~nan], ref["tail"][~nan]) and np.array_equal(S.keys(tail), S.keys(ref["tail"])), case
    assert np.all(tail.view(np.uint32)[nan] == 0x7FFFFFFF), case
    assert np.array_equal(out[3], ref["s"], equal_nan=True) and np.array_equal(out[4], ref["tT"], equal_nan=True), case
    assert np.array_equal(out[6], ref["bad"]), case
    eb = np.abs(out[5] - ref["B"])
    assert np.all(eb <= ref["B_bound"]), (case, eb.max())
    bad = ref["bad"] > 0
    assert np.all(np.isposinf(out[1][bad])) and np.isnan(out[2][bad]).all() and np.isnan(out[0][bad]).all(), case
    worst = dict(khat=0.0, sigma=0.0, elpd=0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for d in np.flatnonzero(~bad):
            f = S.fit(ref["tail"][d], n, out[5][d])
            if math.isinf(f["khat"]):
                assert out[1][d] == math.inf and math.isnan(out[2][d]), (case, d)
            else:
                assert math.isfinite(out[1][d]) and math.isfinite(out[2][d]), (case, d)  # (max() below would pass a NaN over)
                worst["khat"] = max(worst["khat"], abs(out[1][d] - f["khat"]))
                worst["sigma"] = max(worst["sigma"], abs(out[2][d] - f["sigma"]) / abs(f["sigma"]))
            assert math.isfinite(out[0][d]) == math.isfinite(f["elpd"]), (case, d)
            worst["elpd"] = max(worst["elpd"], abs(out[0][d] - f["elpd"]))
    print(case, f"M {M}; B err / bound {np.max(eb / np.maximum(ref['B_bound'], 1e-300)):.3g}; khat err {worst['khat']:.3g} (tol {tol['khat']:.3g}); "
          f"sigma rel err {worst['sigma']:.3g} (tol {tol['sigma']:.3g}); elpd err {worst['elpd']:.3g} (tol {tol['elpd']:.3g}); "
          f"khat {np.nanmin(out[1]):.3f} .. {np.max(out[1]):.3f}")
    for q in worst:
        assert worst[q] <= tol[q], (case, q, worst[q])
    return ref


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_psis_pin(hip_ops, oracle_ops, lowered, case):
    name, n, D, kind = case
    cols = population(name, n, kind, np.random.default_rng(31))
    out, tail, t, M = _run(hip_ops, oracle_ops, lowered, name, D, cols)
    assert np.isfinite(t).all()
    ref = _check(out, tail, t, M, case)
    if kind == "dup" and n > 25:  # (the cutoff is tied on some row: the resampled population has copies)
        k = S.keys(t)
        assert any((k[d] == S.keys(ref["tail"][d, M:])[0]).sum() > 1 for d in range(D)), case


def test_identical_particles(hip_ops, oracle_ops, lowered):
    """n copies of one particle: nothing to smooth — khat = +inf on every row and elpd_loo is the row's one term."""
    cols = population("normal", 4096, "same", np.random.default_rng(32))
    out, tail, t, M = _run(hip_ops, oracle_ops, lowered, "normal", 5, cols)
    _check(out, tail, t, M, "same")
    assert np.all(np.isposinf(out[1])) and np.isnan(out[2]).all() and np.array_equal(out[5], np.full(5, 4096.0 - M))
    assert np.all(np.abs(out[0] - t[:, 0].astype(np.float64)) <= S.TOL["elpd"])


def test_non_finite_entries(hip_ops, oracle_ops, lowered):
    """`hetero` with every fourth Gamma latent outside its support: NaN terms on every row — bad > 0, khat = +inf, a NaN
    elpd_loo, and the selection still exact (the NaNs sort last)."""
    cols = P.columns("hetero", 4096, np.random.default_rng(33), outside=True)
    out, tail, t, M = _run(hip_ops, oracle_ops, lowered, "hetero", 64, cols)
    assert np.isnan(t).any(axis=1).all()
    ref = _check(out, tail, t, M, "outside")
    assert np.all(ref["bad"] > 0) and np.array_equal(out[6], (~np.isfinite(t)).sum(axis=1).astype(np.float64))
    assert np.isnan(out[0]).all() and np.all(np.isposinf(out[1]))


@pytest.mark.parametrize("which", ["high", "low"])
def test_khat_range(hip_ops, oracle_ops, lowered, which):
    """The two cases psis_ref chose on the CPU: a row moved by fifteen noise deviations (reference khat above 0.7) and a
    population far narrower than the noise (a negative reference khat)."""
    cols, data = S.khat_case(which, case_data(lowered, "normal", 64), population)
    out, tail, t, M = _run(hip_ops, oracle_ops, lowered, "normal", 64, cols, data)
    ref = _check(out, tail, t, M, which)
    if which == "high":
        assert ref["khat"][S.HIGH_K["row"]] > 0.7 and out[1][S.HIGH_K["row"]] > 0.7
    else:
        assert ref["khat"].min() < 0.0 and out[1].min() < 0.0


def test_end_to_end(hip_ops):
    """TemperedSMC with covariance proposals on the conjugate regression with 40 rows, n = 4096, then loo(res): elpd within
    FOUR TIMES the spread psis_ref records of the closed-form leave-one-out sum, p_loo within the same relative margin of the
    float64 numpy value on the same columns, no row above the k-hat threshold."""
    model = P.conjugate(40)
    n = 4096
    xs, ys = torch.tensor(model.xs, dtype=torch.float32), torch.tensor(model.ys, dtype=torch.float32)
    target = Target(P.bodies()["normal"], (xs, model.noise), ChoiceMap.d({"y": ys}))
    with use_ops(hip_ops):
        alg = TemperedSMC(target, n, n_moves=2, proposal="covariance")
        res = alg.run(genjax.random.key(12, "philox"))
        loo = alg.loo(res)
        assert isinstance(loo, PSISLOO) and isinstance(loo.pointwise, PointwiseLikelihood) and loo.tail_len == S.tail_len(n) == 192
        assert loo.elpd_loo.shape == loo.khat.shape == loo.sigma.shape == loo.bad.shape == (40,) and loo.elpd_loo.dtype == torch.float64
        assert loo.elpd_loo.is_cuda and torch.equal(alg.loo(res.columns).elpd_loo, loo.elpd_loo)  # a list of columns is the same call
        assert torch.equal(loo.pointwise.lppd, alg.pointwise(res).lppd) and torch.equal(loo.bad, torch.zeros_like(loo.bad))
        with pytest.raises(ValueError, match="no tail to fit"):
            alg.loo([c[:24] for c in res.columns])
    exact = S.closed_form_loo(model).sum()
    bound = S.E2E_FACTOR * S.E2E_SPREAD_ELPD
    cols = [c.cpu().numpy() for c in res.columns]
    ref = S.loo_f64(model, cols)
    p_ref = ((W.reduce64(W.terms_f64(model, cols))[0] - math.log(n)) - ref["elpd"]).sum()
    rel = bound / abs(exact)
    print(f"elpd {loo.elpd:.5f} against {exact:.5f} (error {loo.elpd - exact:+.5f}, bound {bound:.5f}); p_loo {loo.p_loo:.6f} against {p_ref:.6f} "
          f"(relative error {(loo.p_loo - p_ref) / p_ref:+.3g}, margin {rel:.3g}); largest khat {float(loo.khat.max()):.3f}, threshold "
          f"{loo.khat_threshold:.3f}; se {loo.se:.4f}")
    assert abs(loo.elpd - exact) <= bound
    assert abs(loo.p_loo - p_ref) <= rel * abs(p_ref)
    assert loo.n_high == 0 and loo.khat_threshold == 0.7 and loo.looic == -2.0 * loo.elpd and math.isfinite(loo.se)
