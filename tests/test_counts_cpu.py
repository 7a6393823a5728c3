"""The count families without a GPU (include/gjx_counts.h): the header in its slot of the binding tables, the lowering of
Poisson and negative-binomial regressions (the log k! column directly after the observed one), the refusals, the five
generated sources compiled for gfx950 offline with their register counts, tables without a count site unchanged, and the
references of tests/counts_ref.py against the scipy fixture and against each other."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import counts_ref as K
from genjax import ChoiceMap, Target, gamma, gen, negative_binomial, normal, poisson
from genjax._amd import abi, temper
from genjax._amd.ops import TemperPlan
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import ImportanceK
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)
from test_plate_cpu import _data, _plated, _site, _smc_tables

INVALID = -1
SYMBOLS = {"gjx_counts_version", "gjx_logpdf_poisson", "gjx_logpdf_negative_binomial", "gjx_sample_logpdf_poisson",
           "gjx_sample_logpdf_negative_binomial", "gjx_temper_plan_create_counts"}


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
    normal(w * xs, 0.5) @ "z"
    poisson(log_rate=w * xs) @ "y"
    poisson(3.0 * w * w + 1.0) @ "c"  # a scalar observed count site


XS = torch.linspace(-1.0, 1.0, 20)
YS = torch.arange(20, dtype=torch.float32) % 7
CASES = {"pois_rate": (pois_rate, {"y": YS}), "pois_log": (pois_log, {"y": YS}), "negbin": (negbin, {"y": YS}),
         "mixed": (mixed, {"y": YS, "z": 2.0 * XS, "c": 4})}


def target(name):
    m, con = CASES[name]
    return Target(m, (XS,), ChoiceMap.from_mapping(list(con.items())))


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    out = {}
    with use_ops(ops):
        for name in CASES:
            tr = temper.lower(target(name), 64)
            out[name] = (tr, ops.temper_plan_create(tr.sites, keep=(tr.keep, tr)))
    return out


def _prog(arg):
    assert arg.kind == abi.ARG_EXPR
    return [(o.op, o.ref) for o in (abi.ExprOp * arg.ref).from_address(arg.table)]


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.PLAN_HEADERS["counts"]
    keys = list(abi.PLAN_HEADERS)
    # the one slot that keeps what the other suites pin: between "temper" and "psis"
    assert keys.index("counts") == keys.index("temper") + 1 == keys.index("psis") - 1
    assert keys[-3:] == ["plate", "predictive", "pointwise"] and keys.index("psis") == keys.index("plate") - 1
    assert list(abi.MOVE_HEADERS) == ["temper_cov"] and h in abi.all_optional_headers()
    assert all("counts" not in t for t in (abi.OPTIONAL_HEADERS, abi.EXTENSION_HEADERS, abi.MOVE_HEADERS))
    syms = header_symbols("gjx_counts.h")
    assert h.header == "gjx_counts.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.COUNTS_PROTOTYPES and h.version == abi.COUNTS_ABI_VERSION and h.unavailable is abi.CountsUnavailable
    assert issubclass(abi.CountsUnavailable, abi.HeaderUnavailable) and abi.CountsUnavailable.header == "gjx_counts.h"
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    assert not (syms & header_symbols("gjx.h"))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_counts and ops.lib.has["counts"] and not oracle_ops.lib.has_counts
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_counts_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.COUNTS_ABI_VERSION
    txt = open(__file__.replace("tests/test_counts_cpu.py", "include/gjx_counts.h")).read()
    assert f"GJX_COUNTS_VERSION_MAJOR {major.value}" in txt and f"GJX_COUNTS_VERSION_MINOR {minor.value}" in txt
    assert f"GJX_DIST_POISSON {abi.DIST_POISSON} " in txt and f"GJX_DIST_NEGATIVE_BINOMIAL {abi.DIST_NEGATIVE_BINOMIAL} " in txt
    assert f"GJX_COUNTS_MAX_OBSERVED {abi.COUNTS_MAX_OBSERVED} " in txt and abi.COUNTS_MAX_OBSERVED == K.MAX_OBSERVED == 2 ** 24
    assert abi.COUNT_DISTS == (5, 6) and poisson.dist_id == 5 and negative_binomial.dist_id == 6
    assert poisson.value_dtype == negative_binomial.value_dtype == torch.int32
    with pytest.raises(abi.CountsUnavailable, match="gjx_logpdf_poisson"):
        oracle_ops.lib.call("gjx_logpdf_poisson", None, 0, abi.F32(None, 1.0), None, 0, None)


def test_lowering(lowered):
    for name in ("pois_rate", "pois_log"):
        tr, plan = lowered[name]
        assert plan.n_latents == 2 and plan.plated and [m["addr"] for m in tr.meta] == ["w", "b", "y"]
        y = tr.sites[2]
        assert (y.dist, y.observed) == (abi.DIST_POISSON, abi.SITE_PLATED)
        # rate = exp(w * xs + b), written either way: ONE program
        assert _prog(y.arg[0]) == [(abi.EXPR_SITE, 0), (abi.EXPR_DATA, 0), (abi.EXPR_MUL, 0), (abi.EXPR_SITE, 1), (abi.EXPR_ADD, 0), (abi.EXPR_EXP, 0)]
        # the observed column, then its log k! column: float32 of the float64 lgamma(k + 1)
        assert (y.obs.kind, y.obs.ref, y.obs.scale, y.obs.offset) == (abi.ARG_DATA, 1, 1.0, 0.0)
        assert len(tr.data) == 3 and tr.lf_cols == {2: 1} and tr.data_rows == 20 and torch.equal(tr.data[1], YS)
        assert torch.equal(tr.data[2], torch.lgamma(YS.double() + 1.0).float()) and tr.data[2].dtype == torch.float32
        assert tr.meta[2]["is_int"] and tr.meta[2]["plated"] and tr.meta[2]["dtype"] == torch.int32
    tr, plan = lowered["negbin"]
    y = tr.sites[2]
    assert [(s.dist, s.observed) for s in tr.sites] == [(abi.DIST_NORMAL, 0), (abi.DIST_GAMMA, 0), (abi.DIST_NEGATIVE_BINOMIAL, abi.SITE_PLATED)]
    assert (y.arg[0].kind, y.arg[0].ref) == (abi.ARG_SITE, 1)  # total_count: the Gamma latent
    assert _prog(y.arg[1]) == [(abi.EXPR_CONST, 0), (abi.EXPR_SITE, 0), (abi.EXPR_DATA, 0), (abi.EXPR_MUL, 0), (abi.EXPR_NEG, 0),
                               (abi.EXPR_EXP, 0), (abi.EXPR_CONST, 0), (abi.EXPR_ADD, 0), (abi.EXPR_DIV, 0)]  # 1 / (exp(-(w xs)) + 1)
    assert tr.lf_cols == {2: 1}
    tr, plan = lowered["mixed"]
    assert [(s.dist, s.observed) for s in tr.sites] == [(0, 0), (0, abi.SITE_PLATED), (abi.DIST_POISSON, abi.SITE_PLATED), (abi.DIST_POISSON, 1)]
    assert plan.n_plated == 2 and len(tr.data) == 4 and tr.lf_cols == {3: 2} and tr.sites[2].obs.ref == 2 and tr.sites[1].obs.ref == 1
    c = tr.sites[3]  # the scalar observed count site: its value a launch parameter, its rate a program
    assert c.obs.kind == abi.ARG_PARAM and tr.params[c.obs.ref] == 4.0 and c.arg[0].kind == abi.ARG_EXPR
    # the table that draws stage 0 leaves out the plated sites AND the observed count site (the importance plans know no id 5)
    assert [(s.dist, s.observed) for s in temper.prior_table(tr).sites] == [(0, 0)]


def test_the_log_factorial_column_is_recomputed_at_every_run(ops):  # noqa: F811
    ys = YS.clone()
    with use_ops(ops):
        tr = temper.lower(Target(pois_log, (XS,), ChoiceMap.d({"y": ys})), 64)
    ys[3] = 11.0  # in place, after the lowering: the upload reads the tensor as it is now
    cols = tr.data_columns(torch.device("cpu"))
    assert cols[1][3] == 11.0 and cols[2][3] == np.float32(math.lgamma(12.0)) and all(c.dtype == torch.float32 for c in cols)
    ys[4] = 2.0 ** 24 + 2
    with pytest.raises(PlanUnsupported, match="above 2\\^24"):
        tr.data_columns(torch.device("cpu"))


def test_sixteen_columns_are_counted_with_the_log_factorial_column(ops):  # noqa: F811
    @gen
    def many(*cols):
        w = normal(0.0, 1.0) @ "w"
        for k, c in enumerate(cols[:-1]):
            normal(w * c, 1.0) @ ("z", k)
        poisson(log_rate=w * cols[-1]) @ "ycount"

    def tgt(n_x):  # n_x argument columns: 2 (n_x - 1) columns of the Normal sites, then x, y and log y!
        cols = tuple(torch.linspace(0.0, 1.0, 8) + k for k in range(n_x))
        con = [(("z", k), torch.zeros(8) + k) for k in range(n_x - 1)] + [("ycount", torch.ones(8))]
        return Target(many, cols, ChoiceMap.from_mapping(con))

    with use_ops(ops):
        tr = temper.lower(tgt(7), 64)  # 12 + 3 = 15 columns
        assert len(tr.data) == 15 and tr.lf_cols == {14: 13}
        assert ops.temper_plan_create(tr.sites, keep=(tr.keep, tr)).n_plated == 7
        with pytest.raises(PlanUnsupported, match="17 data columns .at most 16. at address 'ycount'"):
            temper.lower(tgt(8), 64)  # 14 + 3


def test_lowering_refusals_name_the_address(ops):  # noqa: F811
    @gen
    def count_latent(xs):
        w = normal(0.0, 1.0) @ "w"
        k = poisson(3.0) @ "klat"
        normal(w * xs, 1.0) @ "y"
        return k

    @gen
    def scalar_value(xs):
        w = normal(0.0, 1.0) @ "w"
        poisson(log_rate=w * xs) @ "yscalar"

    @gen
    def big_scalar():
        lam = gamma(2.0, 1.0) @ "lam"
        poisson(lam) @ "ybig"

    with use_ops(ops):
        with pytest.raises(PlanUnsupported, match="count-valued latent at address 'klat'"):
            temper.lower(Target(count_latent, (XS,), ChoiceMap.d({"y": YS})), 64)
        with pytest.raises(PlanUnsupported, match="address 'yscalar'.*1-D tensor of the same length"):
            temper.lower(Target(scalar_value, (XS,), ChoiceMap.d({"yscalar": 3})), 64)
        with pytest.raises(PlanUnsupported, match="observed count of 16777218 at address 'ybig' is above 2\\^24"):
            temper.lower(Target(big_scalar, (), ChoiceMap.d({"ybig": 2 ** 24 + 2})), 64)
        big = YS.clone()
        big[5] = 2.0 ** 24 + 2
        with pytest.raises(PlanUnsupported, match="observed count of 16777218 at address 'y' is above 2\\^24"):
            temper.lower(Target(pois_log, (XS,), ChoiceMap.d({"y": big})), 64)
        with pytest.raises(ValueError, match="above 2\\^24"):
            poisson.logpdf(2 ** 24 + 2, 3.0)
        assert temper.lower(Target(big_scalar, (), ChoiceMap.d({"ybig": 2 ** 24})), 64).sites[1].dist == abi.DIST_POISSON


def _create(ops, name, sites):  # noqa: F811
    arr = (abi.Site * len(sites))(*sites)
    h = C.c_void_p()
    r = getattr(ops.lib, "_" + name)(arr, len(sites), 0, C.byref(h))
    if r == 0:
        ops.lib.call("gjx_temper_plan_destroy", h)
    return r


def test_creator_validation(ops):  # noqa: F811
    keep = []
    lat = _site(abi.DIST_NORMAL, 0)
    counts = lambda *s: _create(ops, "gjx_temper_plan_create_counts", [lat, *s])  # noqa: E731
    for dist, a0, a1 in ((abi.DIST_POISSON, 2.0, 0.0), (abi.DIST_NEGATIVE_BINOMIAL, 2.0, 0.5)):
        assert counts(_site(dist, 1, a0, a1, 3.0)) == 0                      # a scalar observed count site
        assert counts(_plated(dist, obs=_data(0))) == 0                      # a plated one: columns 0 and 1
        assert counts(_plated(dist, obs=_data(abi.PLATE_MAX_COLS - 2))) == 0
        assert counts(_plated(dist, obs=_data(abi.PLATE_MAX_COLS - 1))) == INVALID  # no room for the log k! column
        assert counts(_plated(dist, obs=_data(0, 2.0))) == INVALID and counts(_plated(dist, obs=_data(0, 1.0, 1.0))) == INVALID  # scaled, shifted
        prog = abi.expr_arg([(abi.EXPR_DATA, 0, 0.0), (abi.EXPR_CONST, 0, 1.0), (abi.EXPR_ADD, 0, 0.0)], keep)
        assert counts(_plated(dist, obs=prog)) == INVALID                    # a program as the observed value
        assert counts(_plated(abi.DIST_NORMAL, obs=prog)) == 0               # (which a Normal plated site may have)
        assert counts(_site(dist, 0, a0, a1)) == INVALID                     # a count-valued latent
        assert _create(ops, "gjx_temper_plan_create_counts", [_site(dist, 1, a0, a1, 3.0)]) == INVALID  # no latent at all
    assert counts(_site(7, 1, 2.0, 0.5, 3.0)) == INVALID and counts(_site(-1, 1)) == INVALID
    # set_data must be given the log k! column
    arr = (abi.Site * 2)(lat, _plated(abi.DIST_POISSON, obs=_data(1)))
    h = C.c_void_p()
    ops.lib.call("gjx_temper_plan_create_counts", arr, 2, 0, C.byref(h))
    cols = (C.c_void_p * 3)(0x1000, 0x2000, 0x3000)
    assert ops.lib._gjx_temper_plan_set_data(h, cols, 2, 8) == INVALID and ops.lib._gjx_temper_plan_set_data(h, cols, 3, 8) == 0
    ops.lib.call("gjx_temper_plan_destroy", h)


def test_every_old_creator_refuses_the_two_ids(ops):  # noqa: F811
    def status(fn):
        try:
            fn()
            return 0
        except abi.GjxError as e:
            return e.code

    lat = _site(abi.DIST_NORMAL, 0)

    def backsim(v):
        arr = (abi.Site * 1)(v)
        h = C.c_void_p()
        r = ops.lib._gjx_backsim_plan_create(arr, 1, 1, 1, 0, C.byref(h))
        if r == 0:
            ops.lib.call("gjx_backsim_plan_destroy", h)
        return r

    creators = {
        "gjx_plan_create_ex": lambda v: status(lambda: ops.plan_create([lat, v])),
        "gjx_plan_create_scoped": lambda v: status(lambda: ops.plan_create([lat, v], scopes=[(0, 1, 2)])),
        "gjx_smc_plan_create": lambda v: status(lambda: ops.smc_plan_create(*_smc_tables(v), 1)),
        "gjx_smc_plan_create_scoped": lambda v: status(lambda: ops.smc_plan_create(*_smc_tables(v), 1, step_scopes=[(0, 1, 2)])),
        "gjx_smc_plan_create_guided": lambda v: status(lambda: ops.smc_plan_create(*_smc_tables(v), 1, guided=True)),
        "gjx_smc_plan_create_params": lambda v: status(lambda: ops.smc_plan_create(*_smc_tables(v), 1, n_params=1)),
        "gjx_scan_plan_create": lambda v: status(lambda: ops.scan_plan_create(_smc_tables(v)[1], _smc_tables(v)[3], 1)),
        "gjx_scan_plan_create_scoped": lambda v: status(lambda: ops.scan_plan_create(_smc_tables(v)[1], _smc_tables(v)[3], 1, scopes=[(0, 1, 2)])),
        "gjx_backsim_plan_create": backsim,
        "gjx_temper_plan_create": lambda v: _create(ops, "gjx_temper_plan_create", [lat, v]),
        "gjx_temper_plan_create_plated": lambda v: _create(ops, "gjx_temper_plan_create_plated", [lat, v]),
    }
    for cname, create in creators.items():
        assert create(_site(abi.DIST_NORMAL, 1)) == 0, cname
        for dist in abi.COUNT_DISTS:
            for observed in (0, 1):
                assert create(_site(dist, observed, 2.0, 0.5, 3.0)) == INVALID, (cname, dist, observed)
    for dist in abi.COUNT_DISTS:
        assert _create(ops, "gjx_temper_plan_create_plated", [lat, _plated(dist)]) == INVALID


def test_tables_without_a_count_site_keep_their_sources(ops):  # noqa: F811
    """Through the new creator a table without a count site gives the plan, and the five sources, the plated creator gives."""
    import plate_ref as P

    with use_ops(ops):
        for name in ("normal", "logistic"):
            tr = temper.lower(P.target(name, 20)[0], 64)
            a = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))  # (no count site: gjx_temper_plan_create_plated)
            arr = (abi.Site * len(tr.sites))(*tr.sites)
            h = C.c_void_p()
            ops.lib.call("gjx_temper_plan_create_counts", arr, len(tr.sites), 0, C.byref(h))
            b = TemperPlan(ops, h, a.n_latents)
            assert a.pointwise_source() == b.pointwise_source() and a.psis_source() == b.psis_source()
            for impl in (0, 1):
                assert a.source(impl) == b.source(impl) and a.cov_source(impl) == b.cov_source(impl)
                assert a.predictive_source(impl) == b.predictive_source(impl)
                assert "poisson" not in a.source(impl) and "vk" not in a.source(impl)


@pytest.mark.parametrize("name", list(CASES))
def test_generated_kernels_compile_for_gfx950(lowered, tmp_path, name):
    """The five sources of a plan with a count site — move, covariance move and predictive under both ciphers, pointwise, PSIS —
    through the library's helper; registers and scratch recorded, no scratch anywhere."""
    tr, plan = lowered[name]
    assert plan.pointwise_compile_check() == 0 and plan.psis_compile_check() == 0
    kernels = [("pointwise", plan.pointwise_source(), "gjx_pointwise_kernel"), ("psis", plan.psis_source(), "gjx_psis_kernel")]
    for impl in (0, 1):
        assert plan.compile_check(impl) == 0 and plan.cov_compile_check(impl) == 0 and plan.predictive_compile_check(impl) == 0
        kernels += [(f"move_{impl}", plan.source(impl), "gjx_temper_move_kernel"), (f"cov_{impl}", plan.cov_source(impl), "gjx_temper_move_cov_kernel"),
                    (f"predictive_{impl}", plan.predictive_source(impl), "gjx_predictive_kernel")]
    lf = tr.sites[2].obs.ref + 1
    for kind, src, entry in kernels:
        k = kernel_notes(src, tmp_path, f"counts_{name}_{kind}")[entry]
        print(name, kind, k)
        assert k["private_segment_fixed_size"] == 0 and k["agpr_count"] == 0, (name, kind, k)  # (no scratch, no spill to AGPRs)
        fam = "negative_binomial" if name == "negbin" else "poisson"
        if kind.startswith("predictive"):  # a draw, and the observed value as rint(data) itself
            assert f"{fam}_draw<{kind[-1]}>" in src and "!= 0 ? 1.0f : 0.0f" not in src
        else:  # log k! is read, never evaluated, at a plated site
            assert f"logpdf_{fam}_lf(vk2, " in src and f", dc{lf}" in src
            assert ("logpdf_poisson(vk3, a0_3)" in src) == (name == "mixed" and not kind.startswith(("pointwise", "psis")))


def test_fused_importance_falls_back_to_the_per_site_route(ops):  # noqa: F811
    """plan.PlanTracer knows no count family: a body with a count site raises PlanUnsupported there, which every caller of the
    fused plan answers with the per-site route."""
    from genjax._amd import plan

    @gen
    def body():
        lam = gamma(3.0, 1.5) @ "lam"
        poisson(lam) @ "k"

    assert id(poisson) not in plan._DIST_IDS and id(negative_binomial) not in plan._DIST_IDS
    with use_ops(ops):
        assert plan._trace(body, ChoiceMap.d({"k": 4}), 64, ()) is None
    assert isinstance(ImportanceK(Target(body, (), ChoiceMap.d({"k": 4})), k_particles=10), ImportanceK)
    assert poisson.canonical_args((2.0,), {}) == (("rate", 2.0),) and poisson.canonical_args((), {"log_rate": 0.5}) == (("log_rate", 0.5),)
    assert negative_binomial.canonical_args((3.0,), {"logits": 0.1}) == (3.0, ("logits", 0.1))
    assert negative_binomial.canonical_args((3.0, 0.4), {}) == (3.0, ("probs", 0.4))
    with pytest.raises(TypeError):
        poisson.canonical_args((), {"scale": 1.0})
    with pytest.raises(TypeError):
        negative_binomial.canonical_args((3.0,), {})


# ---- the references against the fixture and against each other ----------------------------------------------------------------
def test_golden_fixture_covers_the_grid():
    g = K.golden()
    assert [c["rate"] for c in g["poisson"]] == [K.f32(r) for r in K.POISSON_RATES] and {9.99, 10.0, 10.01} <= set(K.POISSON_RATES)
    assert [(c["total_count"], c["probs"]) for c in g["negative_binomial"]] == [(K.f32(t), K.f32(p)) for t in K.NB_TOTALS for p in K.NB_PROBS]
    assert min(K.NB_TOTALS) == 0.05 and max(K.NB_TOTALS) == 1e4 and min(K.NB_PROBS) == 1e-3 and max(K.NB_PROBS) == 0.999
    for c in g["poisson"] + g["negative_binomial"]:
        assert c["k"][:2] == [0.0, 1.0] and len(c["k"]) == len(c["logpmf"]) and all(k == int(k) and 0 <= k <= K.MAX_OBSERVED for k in c["k"])
        assert all(math.isfinite(v) for v in c["logpmf"])
    # float64 of this file's own formulas reproduces scipy's values
    for c in g["poisson"]:
        want = np.array(c["logpmf"])
        assert np.all(np.abs(K.poisson_logpmf(c["k"], c["rate"]) - want) <= 1e-9 * (1.0 + np.abs(want)))
    for c in g["negative_binomial"]:
        want = np.array(c["logpmf"])
        assert np.all(np.abs(K.nb_logpmf(c["k"], c["total_count"], c["probs"]) - want) <= 1e-8 * (1.0 + np.abs(want)))


def test_f32_restatement_holds_the_tolerances():
    """The header's formulas in numpy float32 against the fixture: inside the tolerances with room (0.040 / 0.033 of them)."""
    g = K.golden()
    worst = {"poisson": 0.0, "negative_binomial": 0.0}
    for c in g["poisson"]:
        k = np.array(c["k"])
        r = np.abs(K.poisson_logpmf32(k, c["rate"]).astype(np.float64) - np.array(c["logpmf"])) / K.poisson_tolerance(k, c["rate"])
        worst["poisson"] = max(worst["poisson"], float(r.max()))
    for c in g["negative_binomial"]:
        k = np.array(c["k"])
        r = np.abs(K.nb_logpmf32(k, c["total_count"], c["probs"]).astype(np.float64) - np.array(c["logpmf"])) / K.nb_tolerance(k, c["total_count"], c["probs"])
        worst["negative_binomial"] = max(worst["negative_binomial"], float(r.max()))
    print("largest error / tolerance of the numpy-f32 restatement", worst)
    assert worst["poisson"] <= 0.05 and worst["negative_binomial"] <= 0.05


def test_replay_draws_the_law():
    """The float64 replay of the header's rule is a Poisson sampler: over the host ciphers' words its mean and variance are the
    rate's, on both branches and under both ciphers (six standard errors)."""
    n = 40000
    for impl in (0, 1):
        for rate in (0.0, 0.7, 9.99, 10.0, 37.0, 2500.0):
            x = K.poisson_replay(K.Streams(impl, (7, 8), 3, n, 2), 0, rate).astype(np.float64)
            assert x.min() >= 0 and abs(x.mean() - rate) <= 6.0 * math.sqrt(rate / n) + 1e-12, (impl, rate, x.mean())
            assert abs(x.var() - rate) <= 6.0 * rate * math.sqrt(2.0 / n) + 6.0 * math.sqrt(rate / n) + 1e-12, (impl, rate, x.var())
    assert np.array_equal(K.poisson_replay(K.Streams(0, (7, 8), 0, 3, 1), 0, np.array([-1.0, np.nan, 2.0 ** 31])), [-1, -1, 1 << 30])


def test_recorded_noise_is_reproducible():
    got = K.nb_moment_rms(seeds=24)
    for case_, (rm, rv) in K.NB_MOMENT_RMS.items():
        assert math.isclose(got[case_][0], rm, rel_tol=1e-9) and math.isclose(got[case_][1], rv, rel_tol=1e-9)
    model = K.GammaPoisson()
    assert model.D == 200 and math.isclose(model.post_mean, (model.a + model.S) / (model.b + model.D))
    # two seeds outside the 24: the restated sampler and exact draws land within the end-to-end bounds
    for s in (9100, 9101):
        rng = np.random.default_rng(s)
        st = K.e2e_statistics(model, K.tempered_f64(model, K.E2E_N, 2, 0.5, rng)["lam"], rng)
        st["log_z"] = K.tempered_f64(model, K.E2E_N, 2, 0.5, np.random.default_rng(s + 7))["log_z"] - model.log_z
        print(s, st)
        assert abs(st["log_z"]) <= K.E2E_FACTOR * K.E2E_RMS["log_z"]
        ex = K.e2e_statistics(model, model.exact_draws(K.E2E_N, rng), rng)
        assert all(abs(ex[k]) <= K.E2E_FACTOR * K.E2E_RMS[k] for k in ex), ex
