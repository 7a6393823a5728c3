"""Tempered SMC without a GPU: include/gjx_temper.h as a header of its own (libgjx_hip.so exports it, the oracle does not;
bound through abi.PLAN_HEADERS), the lowering of three models and its refusals, the C-side validation before any launch,
the generated move kernel compiled for gfx950 offline, and the float64 restatement of tests/temper_ref.py."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import genjax
import temper_ref as R
from genjax import ChoiceMap, Target, flip, gen, normal
from genjax._amd import abi, temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)

INVALID, WORKSPACE = -1, -3
SYMBOLS = {"gjx_temper_version", "gjx_temper_plan_create", "gjx_temper_plan_destroy", "gjx_temper_plan_set_params",
           "gjx_temper_plan_n_latents", "gjx_temper_plan_source", "gjx_temper_plan_compile_check", "gjx_temper_move",
           "gjx_temper_ladder_blocks", "gjx_temper_ladder_workspace_bytes", "gjx_temper_ess_ladder"}


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    with use_ops(ops):
        out = {}
        for name, target in R.models().items():
            tracer = temper.lower(target, 64)
            out[name] = (target, tracer, ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer)))
        return out


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.PLAN_HEADERS["temper"]
    assert h in abi.all_optional_headers() and "temper" not in abi.OPTIONAL_HEADERS and "temper" not in abi.EXTENSION_HEADERS
    syms = header_symbols("gjx_temper.h")
    assert h.header == "gjx_temper.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.TEMPER_PROTOTYPES and h.version == abi.TEMPER_ABI_VERSION and h.unavailable is abi.TemperUnavailable
    assert issubclass(abi.TemperUnavailable, abi.HeaderUnavailable) and abi.TemperUnavailable.header == "gjx_temper.h"
    assert ops.lib.has_temper and ops.lib.has["temper"] and not oracle_ops.lib.has_temper
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_temper_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.TEMPER_ABI_VERSION
    txt = open(__file__.replace("tests/test_temper_cpu.py", "include/gjx_temper.h")).read()
    for name, value in (("MAX_LATENTS", abi.TEMPER_MAX_LATENTS), ("MAX_MOVES", abi.TEMPER_MAX_MOVES), ("MAX_LADDER", abi.TEMPER_MAX_LADDER)):
        assert f"#define GJX_TEMPER_{name} {value}\n" in txt


def test_oracle_bound_ops_refuse(oracle_ops):
    target = R.models()["regression"]
    with use_ops(oracle_ops):
        with pytest.raises(abi.TemperUnavailable, match="gjx_temper"):
            TemperedSMC(target, 64).run(genjax.random.key(1))
    with pytest.raises(abi.TemperUnavailable, match="gjx_temper_plan_create"):
        oracle_ops.temper_plan_create([])
    with pytest.raises(abi.TemperUnavailable, match="gjx_temper_ess_ladder"):
        oracle_ops.temper_ess_ladder(torch.zeros(8), [0.5])
    with pytest.raises(abi.TemperUnavailable, match="gjx_temper_move"):
        oracle_ops.temper_move(None, genjax.random.key(1), [torch.zeros(8)], None, None, 0.0, 0)
    with pytest.raises(abi.TemperUnavailable):
        oracle_ops.lib.call("gjx_temper_ladder_blocks", 8)


def test_lowering_of_three_models(lowered):
    _, tr, plan = lowered["regression"]
    assert plan.n_latents == 2 and [m["addr"] for m in tr.meta if m["obs"] is None] == ["w", "b"]
    assert len(tr.sites) == 22 and all(s.dist == abi.DIST_NORMAL for s in tr.sites)
    assert all(s.observed == 1 and s.arg[0].kind == abi.ARG_EXPR and s.obs.kind == abi.ARG_PARAM for s in tr.sites[2:])
    assert len(tr.params) == 21  # the noise and the twenty observations: launch parameters, not source
    _, tr, plan = lowered["gamma_normal"]
    assert plan.n_latents == 2 and [s.dist for s in tr.sites[:2]] == [abi.DIST_GAMMA, abi.DIST_NORMAL]
    assert all(s.observed == 1 and s.arg[1].kind == abi.ARG_EXPR for s in tr.sites[2:])
    _, tr, plan = lowered["beta_bernoulli"]
    assert plan.n_latents == 1 and [(s.dist, s.observed) for s in tr.sites] == [(abi.DIST_BETA, 0), (abi.DIST_BERNOULLI, 1)]


def test_source_holds_no_parameter_or_observation(ops, lowered):  # noqa: F811
    reg = R.Regression()
    base = R.models()["regression"]
    other = Target(base.p, ([float(x) for x in reg.xs], 0.25), ChoiceMap.d({("y", i): float(3.0 * y + 1.0) for i, y in enumerate(reg.ys)}))
    with use_ops(ops):
        tr = temper.lower(other, 64)
        plan2 = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
    for impl in (0, 1):
        src = lowered["regression"][2].source(impl)
        assert src == plan2.source(impl)
        assert "gjx_temper_move_kernel" in src and "tm_assess(" in src and "__shared__" not in src and "__syncthreads" not in src
        assert "GJX_BM_LDS" not in src


def test_lowering_refusals_name_the_address(ops):  # noqa: F811
    @gen
    def int_latent():
        z = flip(0.3) @ "z"
        normal(0.0, 1.0) @ "x"
        normal(0.5, 1.0) @ "y"
        return z

    @gen
    def inner():
        return normal(0.0, 1.0) @ "u"

    @gen
    def nested():
        u = inner() @ "sub"
        normal(u, 1.0) @ "y"

    @gen
    def vector_site():
        x = normal(torch.zeros(3), 1.0) @ "vec"
        normal(0.0, 1.0) @ "y"
        return x

    @gen
    def plain():
        x = normal(0.0, 1.0) @ "x"
        normal(x, 1.0) @ "y"

    with use_ops(ops):
        for model, chm, word in ((int_latent, {"y": 0.1}, "'z'"), (nested, {"y": 0.1}, "'sub'"), (vector_site, {"y": 0.1}, "'vec'"),
                                 (plain, {}, "'x'"), (plain, {"x": 0.2, "y": 0.1}, "'y'")):
            with pytest.raises(PlanUnsupported, match=word):
                temper.lower(Target(model, (), ChoiceMap.d(chm)), 64)
        with pytest.raises(PlanUnsupported, match="no observed site"):
            temper.lower(Target(plain, (), ChoiceMap.d({})), 64)
        with pytest.raises(PlanUnsupported, match="no latent site"):
            temper.lower(Target(plain, (), ChoiceMap.d({"x": 0.2, "y": 0.1})), 64)


def _site(dist, observed, a0=0.0, a1=1.0, obs=0.0):
    s = abi.Site()
    s.dist, s.observed, s.out_col = dist, observed, -1
    s.arg[0] = abi.Arg(abi.ARG_CONST, 0, 0.0, a0, None)
    s.arg[1] = abi.Arg(abi.ARG_CONST, 0, 0.0, a1, None)
    s.obs = abi.Arg(abi.ARG_CONST, 0, 0.0, obs, None)
    return s


def test_plan_create_validation(ops):  # noqa: F811
    lib = ops.lib

    def rc(sites, flags=0, n=None):
        arr = (abi.Site * max(1, len(sites)))(*sites)
        h = C.c_void_p()
        r = lib._gjx_temper_plan_create(arr, len(sites) if n is None else n, flags, C.byref(h))
        if r == 0:
            lib.call("gjx_temper_plan_destroy", h)
        return r

    lat, obs = _site(abi.DIST_NORMAL, 0), _site(abi.DIST_NORMAL, 1)
    assert rc([lat, obs]) == 0 and rc([_site(abi.DIST_GAMMA, 0, 2.0), _site(abi.DIST_BETA, 0, 2.0, 2.0), _site(abi.DIST_BERNOULLI, 1, 0.5)]) == 0
    assert rc([lat, obs], flags=1) == INVALID and rc([lat, obs], n=0) == INVALID and rc([lat, obs], n=abi.MAX_SITES + 1) == INVALID
    assert lib._gjx_temper_plan_create(None, 2, 0, C.byref(C.c_void_p())) == INVALID
    assert rc([lat]) == INVALID and rc([obs]) == INVALID  # no observed site / no latent site
    assert rc([_site(abi.DIST_BERNOULLI, 0, 0.5), obs]) == INVALID  # an integer-valued latent
    assert rc([lat, _site(abi.DIST_NORMAL, 2)]) == INVALID and rc([lat, _site(abi.DIST_NORMAL, 3)]) == INVALID  # observed > 1
    assert rc([lat] * abi.TEMPER_MAX_LATENTS + [obs]) == 0 and rc([lat] * (abi.TEMPER_MAX_LATENTS + 1) + [obs]) == INVALID
    bad = _site(abi.DIST_NORMAL, 1)
    bad.arg[0] = abi.Arg(abi.ARG_SITE, 5, 1.0, 0.0, None)  # a reference to a later site
    assert rc([lat, bad]) == INVALID
    assert lib.call("gjx_temper_plan_n_latents", None) == INVALID


def test_move_and_ladder_validation(ops, lowered):  # noqa: F811
    lib, plan = ops.lib, lowered["regression"][2]
    plan.set_params(lowered["regression"][1].params)
    scales = (C.c_float * 2)(0.1, 0.1)

    def io(**kw):
        o = abi.TemperIO()
        o.impl, o.n_moves, o.recompute, o.beta, o.n = 1, 2, 0, 0.5, 8
        for l in range(2):
            o.x_in[l], o.x_out[l] = 0x1000, 0x2000
        o.lp_in = o.ll_in = 0x3000
        o.lp_out = o.ll_out = 0x4000
        o.scales = scales
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    rc = lambda o: lib._gjx_temper_move(plan.handle, C.byref(o) if o is not None else None, None)
    assert rc(None) == INVALID and lib._gjx_temper_move(None, C.byref(io()), None) == INVALID
    for kw in (dict(n=0), dict(n=1 << 31), dict(impl=2), dict(impl=0, key_lane=3), dict(n_moves=-1), dict(n_moves=abi.TEMPER_MAX_MOVES + 1),
               dict(lp_out=None), dict(ll_out=None), dict(lp_in=None), dict(ll_in=None), dict(scales=None), dict(n_input_cols=-1),
               dict(n_input_cols=17), dict(n_input_cols=1)):
        assert rc(io(**kw)) == INVALID, kw
    o = io()
    o.x_in[1] = None
    assert rc(o) == INVALID
    o = io()
    o.x_out[0] = None
    assert rc(o) == INVALID
    # the parameters of the table have to be set first
    tr = lowered["regression"][1]
    fresh = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
    assert lib._gjx_temper_move(fresh.handle, C.byref(io()), None) == INVALID
    assert lib._gjx_temper_plan_set_params(fresh.handle, None, 0) == INVALID  # fewer than the table reads
    for fn in ("_gjx_temper_plan_compile_check",):
        assert getattr(lib, fn)(None, 0) == INVALID and getattr(lib, fn)(plan.handle, 2) == INVALID

    # the ladder
    assert lib.call("gjx_temper_ladder_blocks", 0) == 0 and lib.call("gjx_temper_ladder_blocks", 1) == 1
    assert lib.call("gjx_temper_ladder_blocks", 1000) == 4 and lib.call("gjx_temper_ladder_blocks", 10 ** 6) == 256
    wb = lambda n, g: lib.call("gjx_temper_ladder_workspace_bytes", n, g)
    assert wb(0, 4) == 0 and wb(1 << 31, 4) == 0 and wb(8, 0) == 0 and wb(8, abi.TEMPER_MAX_LADDER + 1) == 0
    assert 0 < wb(1000, 32) < wb(10 ** 6, 32) < wb(10 ** 6, 64)
    d = (C.c_float * 4)(0.0, 0.1, 0.5, 1.0)
    lad = lambda ll=0x1000, n=8, dl=d, g=4, out=0x2000, ws=0x8000, nb=1 << 20: lib._gjx_temper_ess_ladder(
        C.c_void_p(ll), n, dl, g, C.c_void_p(out), C.c_void_p(ws), nb, None)
    assert lad(ll=None) == INVALID and lad(dl=None) == INVALID and lad(out=None) == INVALID and lad(n=0) == INVALID
    assert lad(n=1 << 31) == INVALID and lad(g=0) == INVALID and lad(g=abi.TEMPER_MAX_LADDER + 1) == INVALID and lad(ws=0x8004) == INVALID
    assert lad(dl=(C.c_float * 4)(0.0, -0.1, 0.5, 1.0)) == INVALID and lad(dl=(C.c_float * 4)(0.0, float("nan"), 0.5, 1.0)) == INVALID
    assert lad(dl=(C.c_float * 4)(0.0, float("inf"), 0.5, 1.0)) == INVALID
    assert lad(ws=None) == WORKSPACE and lad(nb=wb(8, 4) - 1) == WORKSPACE


@pytest.mark.parametrize("name", ["regression", "gamma_normal", "beta_bernoulli"])
def test_move_kernels_compile_for_gfx950(lowered, name):
    plan = lowered[name][2]
    for impl in (0, 1):
        assert plan.compile_check(impl) == 0, (name, impl)


def test_regression_move_kernel_has_no_scratch(lowered, tmp_path):
    plan = lowered["regression"][2]
    for impl in (0, 1):
        metas = kernel_notes(plan.source(impl), tmp_path, f"temper_regression_{impl}")
        k = metas["gjx_temper_move_kernel"]
        print("temper move kernel, regression, impl", impl, k)
        assert k["private_segment_fixed_size"] == 0 and k["agpr_count"] == 0 and k["vgpr_count"] <= 128


def test_schedule_rule_is_the_documented_one():
    d = temper.ladder_deltas(0.25)
    assert d.dtype == np.float32 and len(d) == temper.LADDER and d[-1] == np.float32(0.75) and d[0] == np.float32(0.75 * 2.0 ** -31)
    f = temper.ladder_deltas(0.25, d[10], d[11])
    assert f[0] == d[10] and np.all(np.diff(f) > 0) and f[-1] < d[11]
    calls = []

    def ess_fn(deltas):  # ESS falls with the step: 100 / (1 + 1000 delta)
        calls.append(np.asarray(deltas))
        return 100.0 / (1.0 + 1000.0 * np.asarray(deltas, dtype=np.float64))

    nb, e = temper.next_beta(0.25, 50.0, ess_fn)  # ESS >= 50 <=> delta <= 1e-3
    assert len(calls) == 2 and 0.25 < nb <= np.float32(0.25) + np.float32(1e-3) and e >= 50.0
    assert nb > 0.25 + 0.9e-3  # within one fine rung (1 / 32 of a factor-two bracket) of the largest admissible step
    calls.clear()
    assert temper.next_beta(0.25, 0.01, ess_fn) == (1.0, 100.0 / 751.0) and len(calls) == 1  # straight to 1
    assert temper.next_beta(0.25, 1000.0, lambda d: np.zeros(len(d)))[0] > 0.25  # no candidate qualifies: the smallest step


def test_restatement_with_fixed_betas_is_unbiased():
    """mean(Z-hat / Z) of the float64 restatement with a FIXED five-point schedule (and a fixed proposal scale: a scale taken
    from the population would make the move kernel depend on the particles as the adaptive schedule does) on the
    regression with m = 4 points, n = 8 particles, K = 1: within 4 standard errors of 1."""
    model = R.Regression(m=4, noise=0.1)
    betas = [0.0, 0.02, 0.1, 0.35, 1.0]
    S = 3000
    z = np.array([math.exp(R.tempered_f64(model, 8, 1, 0.5, np.random.default_rng(5000 + s), betas=betas, scale=0.2)["log_z"] - model.log_z)
                  for s in range(S)])
    se = z.std(ddof=1) / math.sqrt(S)
    print(f"mean Z-hat / Z = {z.mean():.4f}, standard error {se:.4f} over {S} seeds")
    assert abs(z.mean() - 1.0) <= 4.0 * se


def test_restatement_recovers_the_closed_form():
    """One adaptive run of the restatement at n = 4096, K = 2: 7 to 8 stages, means within 0.25 posterior deviations."""
    model = R.Regression()
    r = R.tempered_f64(model, 4096, 2, 0.5, np.random.default_rng(1000))
    sd = np.sqrt(np.diag(model.post_cov))
    assert 6 <= len(r["betas"]) - 1 <= 9 and r["betas"][-1] == 1.0 and np.all(np.diff(r["betas"]) > 0)
    assert abs(r["w"].mean() - model.post_mean[0]) < 0.25 * sd[0] and abs(r["b"].mean() - model.post_mean[1]) < 0.25 * sd[1]
    assert abs(r["log_z"] - model.log_z) < 5 * 0.083  # (profiles/temper_summary.md: the RMS error over 64 seeds)
