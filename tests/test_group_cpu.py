"""Grouped latents of a tempered plan without a GPU: include/gjx_group.h as a header of its own, the lowering of
`dist.repeat(n=G)` and `a[g]` to grouped sites, GROUP operands and offsets, every refusal with its address, the C-side
validation before any launch, the generated move kernels compiled for gfx950 offline (no scratch), tables without a grouped
site unchanged, and the references of tests/group_ref.py against each other."""

import ctypes as C

import numpy as np
import pytest
import torch

import genjax
import group_ref as GR
import temper_ref as R
from genjax import ChoiceMap, Target, categorical, flip, gamma, gen, normal, poisson
from genjax._amd import abi, temper
from genjax._amd.ops import TemperPlan
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)
from test_plate_cpu import _data, _plated, _site

INVALID = -1
SYMBOLS = {"gjx_group_version", "gjx_temper_plan_create_grouped", "gjx_temper_plan_set_groups", "gjx_temper_plan_n_grouped",
           "gjx_temper_move_grouped"}
SIZES = GR.LAYOUTS[5]


def _lower(ops, name, sizes=SIZES, seed=0):  # noqa: F811
    with use_ops(ops):
        target, g, off = GR.target(name, sizes, seed)
        tracer = temper.lower(target, 64)
        return target, tracer, ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer)), g, off


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    return {name: _lower(ops, name) for name in GR.MODELS}


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.PLAN_HEADERS["group"]
    assert h in abi.all_optional_headers() and all("group" not in t for t in (abi.OPTIONAL_HEADERS, abi.EXTENSION_HEADERS, abi.MOVE_HEADERS))
    syms = header_symbols("gjx_group.h")
    assert h.header == "gjx_group.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.GROUP_PROTOTYPES and h.version == abi.GROUP_ABI_VERSION and h.unavailable is abi.GroupUnavailable
    assert issubclass(abi.GroupUnavailable, abi.HeaderUnavailable) and abi.GroupUnavailable.header == "gjx_group.h"
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    assert not (syms & header_symbols("gjx.h"))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_group and ops.lib.has["group"] and not oracle_ops.lib.has_group
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_group_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.GROUP_ABI_VERSION
    txt = open(__file__.replace("tests/test_group_cpu.py", "include/gjx_group.h")).read()
    for name, value in (("GJX_SITE_GROUPED", abi.SITE_GROUPED), ("GJX_ARG_GROUP", abi.ARG_GROUP), ("GJX_EXPR_GROUP", abi.EXPR_GROUP),
                        ("GJX_GROUP_MAX_SITES", abi.GROUP_MAX_SITES), ("GJX_GROUP_MAX_GROUPS", abi.GROUP_MAX_GROUPS),
                        ("GJX_GROUP_VERSION_MAJOR", major.value), ("GJX_GROUP_VERSION_MINOR", minor.value)):
        assert f"#define {name} {value}" in txt
    # the next free values
    assert abi.SITE_GROUPED == abi.SITE_PLATED + 1 and abi.ARG_GROUP == abi.ARG_DATA + 1 and abi.EXPR_GROUP == abi.EXPR_DATA + 1
    assert "GROUP" not in open(__file__.replace("tests/test_group_cpu.py", "include/gjx.h")).read()
    with use_ops(oracle_ops):
        with pytest.raises(abi.HeaderUnavailable, match="gjx_temper|gjx_group"):
            TemperedSMC(GR.target("intercept", SIZES)[0], 64).run(genjax.random.key(1))
    with pytest.raises(abi.GroupUnavailable, match="gjx_temper_move_grouped"):
        oracle_ops.lib.call("gjx_temper_move_grouped", None, None, None)


def _prog(arg):
    assert arg.kind == abi.ARG_EXPR
    return [(o.op, o.ref) for o in (abi.ExprOp * arg.ref).from_address(arg.table)]


def test_lowering(lowered):
    _, tr, plan, g, off = lowered["intercept"]
    assert plan.n_latents == 2 and plan.n_grouped == 1 and plan.plated and [m["addr"] for m in tr.meta] == ["mu", "b", "a", "y"]
    assert [(s.dist, s.observed) for s in tr.sites] == [(abi.DIST_NORMAL, 0)] * 2 + [(abi.DIST_NORMAL, abi.SITE_GROUPED),
                                                                                         (abi.DIST_NORMAL, abi.SITE_PLATED)]
    a, y = tr.sites[2], tr.sites[3]
    assert (a.arg[0].kind, a.arg[0].ref, a.arg[0].scale, a.arg[0].offset) == (abi.ARG_SITE, 0, 1.0, 0.0) and a.arg[1].kind == abi.ARG_CONST
    # a[g] + b * xs: the grouped value is a program leaf; the group tensor is NOT a data column
    assert _prog(y.arg[0]) == [(abi.EXPR_GROUP, 0), (abi.EXPR_SITE, 1), (abi.EXPR_DATA, 0), (abi.EXPR_MUL, 0), (abi.EXPR_ADD, 0)]
    assert len(tr.data) == 2 and tr.data_rows == len(g) == 13 and tr.n_groups == 5 and tr.n_grouped == 1
    assert tr.group.dtype == torch.int64 and torch.equal(tr.group, torch.from_numpy(g))
    assert tr.meta[2]["grouped"] and tr.meta[2]["obs"] is None and not tr.meta[3].get("grouped")
    # the offsets: empty groups are legal (the first and the last here)
    o = tr.group_offsets()
    assert o.dtype == torch.int32 and o.tolist() == off.tolist() == [0, 0, 3, 4, 13, 13]
    # stage 0 draws the scalars alone
    pt = temper.prior_table(tr)
    assert [(s.dist, s.observed, s.out_col) for s in pt.sites] == [(abi.DIST_NORMAL, 0, 0), (abi.DIST_NORMAL, 0, 1)]
    _, tr, plan, _, _ = lowered["slope"]
    assert plan.n_grouped == 2 and [s.observed for s in tr.sites] == [0, 0, abi.SITE_GROUPED, abi.SITE_GROUPED, abi.SITE_PLATED]
    assert _prog(tr.sites[4].arg[0]) == [(abi.EXPR_GROUP, 0), (abi.EXPR_GROUP, 1), (abi.EXPR_DATA, 0), (abi.EXPR_MUL, 0), (abi.EXPR_ADD, 0)]
    assert tr.sites[3].arg[0].kind == abi.ARG_SITE and tr.sites[3].arg[0].ref == 1
    _, tr, plan, _, _ = lowered["gamma"]
    # s[g] itself as the scale: the affine operand
    s = tr.sites[2]
    assert (tr.sites[1].dist, tr.sites[1].observed) == (abi.DIST_GAMMA, abi.SITE_GROUPED)
    assert (s.arg[1].kind, s.arg[1].ref, s.arg[1].scale, s.arg[1].offset) == (abi.ARG_GROUP, 0, 1.0, 0.0)
    _, tr, plan, _, _ = lowered["flat"]
    assert [s.observed for s in tr.sites] == [0, abi.SITE_PLATED, 0, abi.SITE_GROUPED, 1, abi.SITE_PLATED] and plan.n_latents == 2


def test_group_tensor_is_read_again_at_every_run(ops):  # noqa: F811
    with use_ops(ops):
        target, g, _ = GR.target("intercept", SIZES)
        tr = temper.lower(target, 64)
        gt = target.args[1]
        gt[3] = 1  # (in place: the row moves to group 1; still sorted)
        assert tr.group_offsets().tolist() == [0, 0, 4, 4, 13, 13]
        gt[0] = 4
        with pytest.raises(PlanUnsupported, match="'a'.*not sorted"):
            tr.group_offsets()


def test_lowering_refusals_name_the_address(ops):  # noqa: F811
    G = 3
    xs, ys = torch.linspace(0.0, 1.0, 8), torch.zeros(8)
    g = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2])
    g2 = g.clone()

    def model(fn):
        return gen(fn)

    def unsorted(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a_unsorted"
        normal(a[g] + xs, 1.0) @ "y"

    def reads_data(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu * xs, 1.0).repeat(n=G) @ "a_data"
        normal(a[g], 1.0) @ "y"

    def reads_group(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a"
        c = normal(a[g], 1.0).repeat(n=G) @ "c_chain"
        normal(c[g] + xs, 1.0) @ "y"

    def whole(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a_whole"
        normal(a, 1.0) @ "y"

    def arithmetic(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a_arith"
        normal(2.0 * a, 1.0) @ "y"

    def scalar_site(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a"
        normal(a[g], 1.0) @ "y_scalar"

    def float_index(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a_float"
        normal(a[xs], 1.0) @ "y"

    def two_tensors(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a"
        c = normal(mu, 1.0).repeat(n=G) @ "c_other"
        normal(a[g] + c[g2] * xs, 1.0) @ "y"

    def two_sizes(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a"
        c = normal(mu, 1.0).repeat(n=G + 1) @ "c_size"
        normal(a[g] + c[g] * xs, 1.0) @ "y"

    def count_site(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        k = poisson(3.0).repeat(n=G) @ "k_count"
        normal(mu + xs, 1.0) @ "y"

    def flip_site(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        k = flip(0.5).repeat(n=G) @ "k_flip"
        normal(mu + xs, 1.0) @ "y"

    def cat_site(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        k = categorical(logits=torch.zeros(3)).repeat(n=G) @ "k_cat"
        normal(mu + xs, 1.0) @ "y"

    def observed(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a_obs"
        normal(a[g] + xs, 1.0) @ "y"

    def unread(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a_unread"
        normal(mu + xs, 1.0) @ "y"

    def no_scalar(xs, g):
        a = normal(0.0, 1.0).repeat(n=G) @ "a"
        normal(a[g] + xs, 1.0) @ "y"

    def too_many(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        vals = [normal(mu, 1.0).repeat(n=G) @ ("a", k) for k in range(abi.GROUP_MAX_SITES + 1)]
        normal(vals[0][g] + xs, 1.0) @ "y"

    def short_plate(xs, g):
        mu = normal(0.0, 1.0) @ "mu"
        a = normal(mu, 1.0).repeat(n=G) @ "a_short"
        normal(a[g[:5]] + xs, 1.0) @ "y"

    cases = ((unsorted, torch.tensor([0, 1, 0, 1, 1, 2, 2, 2]), {"y": ys}, "'a_unsorted'.*not sorted"),
             (unsorted, torch.tensor([0, 0, 0, 1, 1, 2, 2, 3]), {"y": ys}, "'a_unsorted'.*outside 0 .. 2"),
             (unsorted, torch.tensor([-1, 0, 0, 1, 1, 2, 2, 2]), {"y": ys}, "'a_unsorted'.*outside 0 .. 2"),
             (reads_data, g, {"y": ys}, "'a_data'.*reads data"),
             (reads_group, g, {"y": ys}, "'c_chain'.*reads a grouped latent"),
             (whole, g, {"y": ys}, "'y'.*'a_whole' whole"),
             (arithmetic, g, {"y": ys}, "'a_arith'.*indexing by the group tensor"),
             (scalar_site, g, {"y_scalar": 0.5}, "'y_scalar'"),
             (float_index, g, {"y": ys}, "'a_float'.*1-D integer"),
             (two_tensors, g, {"y": ys}, "'c_other'.*another group tensor"),
             (two_sizes, g, {"y": ys}, "'c_size'.*G = 4.*G = 3"),
             (count_site, g, {"y": ys}, "'k_count'.*normal, gamma or beta"),
             (flip_site, g, {"y": ys}, "'k_flip'.*normal, gamma or beta"),
             (cat_site, g, {"y": ys}, "'k_cat'.*normal, gamma or beta"),
             (observed, g, {"y": ys, "a_obs": torch.zeros(G)}, "'a_obs'.*observed"),
             (unread, g, {"y": ys}, "'a_unread'.*read by no plated site"),
             (no_scalar, g, {"y": ys}, "no scalar latent"),
             (too_many, g, {"y": ys}, r"more than 4 grouped sites.*\('a', 4\)"),
             (short_plate, g, {"y": ys}, "'a_short'|'y'"))
    with use_ops(ops):
        for fn, gt, chm, word in cases:
            with pytest.raises(PlanUnsupported, match=word):
                temper.lower(Target(model(fn), (xs, gt), ChoiceMap.d(chm)), 64)
        target = GR.target("intercept", SIZES)[0]
        key = genjax.random.key(1)
        with pytest.raises(PlanUnsupported, match="covariance.*'a'"):
            TemperedSMC(target, 64, proposal="covariance")._state()
        alg = TemperedSMC(target, 64)
        cols = [torch.zeros(64), torch.zeros(64)]
        for what, call in (("run_smc", lambda: alg.run_smc(key)), ("pointwise", lambda: alg.pointwise(cols)),
                           ("loo", lambda: alg.loo(cols)), ("predictive", lambda: alg.predictive(cols, key))):
            with pytest.raises(PlanUnsupported, match=f"{what}.*'a'"):
                call()


def _grouped(dist=abi.DIST_NORMAL, a0=None, a1=None):
    s = _site(dist, abi.SITE_GROUPED)
    if a0 is not None:
        s.arg[0] = a0
    if a1 is not None:
        s.arg[1] = a1
    return s


def _grp(ref, scale=1.0, offset=0.0):
    return abi.Arg(abi.ARG_GROUP, ref, scale, offset, None)


def test_creator_validation(ops):  # noqa: F811
    lib, keep = ops.lib, []

    def rc(sites, flags=0, fn="_gjx_temper_plan_create_grouped"):
        arr = (abi.Site * max(1, len(sites)))(*sites)
        h = C.c_void_p()
        r = getattr(lib, fn)(arr, len(sites), flags, C.byref(h))
        if r == 0:
            lib.call("gjx_temper_plan_destroy", h)
        return r

    lat, obs = _site(abi.DIST_NORMAL, 0), _site(abi.DIST_NORMAL, 1)
    site0 = abi.Arg(abi.ARG_SITE, 0, 1.0, 0.0, None)
    prog = lambda *ops_: abi.expr_arg([(o, r, 0.0) for o, r in ops_], keep)
    reader = _plated(a0=_grp(0))
    assert rc([lat, _grouped(a0=site0), reader]) == 0
    assert rc([lat, _grouped(), _grouped(abi.DIST_GAMMA, a0=abi.Arg(abi.ARG_CONST, 0, 0.0, 2.0, None)),
               _plated(a0=prog((abi.EXPR_GROUP, 0), (abi.EXPR_GROUP, 1), (abi.EXPR_DATA, 1), (abi.EXPR_MUL, 0), (abi.EXPR_ADD, 0)))]) == 0
    assert rc([lat, obs, _plated(), _grouped(), _plated(a0=_data(1), a1=_grp(0, 2.0, 0.5))]) == 0
    # every other creator refuses the mode and both operand kinds
    for fn in ("_gjx_temper_plan_create", "_gjx_temper_plan_create_plated", "_gjx_temper_plan_create_counts"):
        assert rc([lat, _grouped(a0=site0), reader], fn=fn) == INVALID, fn
        assert rc([lat, reader], fn=fn) == INVALID, fn
        assert rc([lat, _plated(a0=prog((abi.EXPR_GROUP, 0)))], fn=fn) == INVALID, fn
    # whatever the plated creator refuses
    assert rc([lat, _grouped(), reader], flags=1) == INVALID and rc([_grouped(), reader]) == INVALID  # (no scalar latent)
    assert lib._gjx_temper_plan_create_grouped(None, 2, 0, C.byref(C.c_void_p())) == INVALID
    # more than four grouped sites; an integer-valued or count-valued grouped site
    assert rc([lat] + [_grouped()] * 4 + [reader]) == 0 and rc([lat] + [_grouped()] * 5 + [reader]) == INVALID
    for dist in (abi.DIST_BERNOULLI, abi.DIST_CATEGORICAL, abi.DIST_POISSON, abi.DIST_NEGATIVE_BINOMIAL):
        assert rc([lat, _grouped(dist, a0=abi.Arg(abi.ARG_CONST, 0, 0.0, 0.5, None)), reader]) == INVALID, dist
    # a grouped site's argument reads data / a grouped value / a site that is no scalar latent
    assert rc([lat, _grouped(a0=_data(0)), reader]) == INVALID
    assert rc([lat, _grouped(), _grouped(a0=_grp(0)), reader]) == INVALID
    assert rc([lat, _grouped(a0=prog((abi.EXPR_GROUP, 0))), reader]) == INVALID
    assert rc([lat, obs, _grouped(a0=abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None)), reader]) == INVALID
    assert rc([lat, _grouped(), _grouped(a0=abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None)), reader]) == INVALID
    # a GROUP operand outside a0 / a1 of a plated site; a ref not below the grouped sites before it
    bad_lat, bad_obs = _site(abi.DIST_NORMAL, 0), _site(abi.DIST_NORMAL, 1)
    bad_lat.arg[0], bad_obs.arg[0] = _grp(0), _grp(0)
    assert rc([lat, _grouped(), bad_lat, reader]) == INVALID and rc([lat, _grouped(), bad_obs, reader]) == INVALID
    assert rc([lat, _grouped(), _plated(a0=_grp(0), obs=_grp(0))]) == INVALID
    assert rc([lat, _grouped(), _plated(a0=_grp(1))]) == INVALID and rc([lat, _grouped(), _plated(a0=_grp(-1))]) == INVALID
    assert rc([lat, reader, _grouped()]) == INVALID  # (read before its site)
    assert rc([lat, _grouped(), _plated(a0=prog((abi.EXPR_GROUP, 1)))]) == INVALID
    # a grouped site that no plated site reads; a per-particle input column
    assert rc([lat, _grouped(), _plated()]) == INVALID
    inp = _site(abi.DIST_NORMAL, 0)
    inp.arg[0] = abi.Arg(abi.ARG_INPUT, 0, 1.0, 0.0, None)
    assert rc([inp, _grouped(), reader]) == INVALID


def test_setters_and_move_validation(ops, lowered):  # noqa: F811
    lib = ops.lib
    _, tr, plan, _, _ = lowered["intercept"]
    flat_plan = _lower_plain(ops)
    p, fake = plan.handle, 0x1000
    assert lib._gjx_temper_plan_n_grouped(p) == 1 and lib._gjx_temper_plan_n_grouped(flat_plan.handle) == 0
    assert lib._gjx_temper_plan_n_grouped(None) == INVALID
    assert lib._gjx_temper_plan_set_groups(None, fake, 3) == INVALID and lib._gjx_temper_plan_set_groups(p, None, 3) == INVALID
    assert lib._gjx_temper_plan_set_groups(p, fake, 0) == INVALID and lib._gjx_temper_plan_set_groups(p, fake, 1 << 24) == INVALID
    assert lib._gjx_temper_plan_set_groups(flat_plan.handle, fake, 3) == INVALID  # no grouped site

    def io(**kw):
        g = abi.GroupIO()
        g.t.impl, g.t.n_moves, g.t.recompute, g.t.n = 1, 1, 1, 64
        g.t.scales = (C.c_float * 2)(0.1, 0.1)
        for l in range(2):
            g.t.x_in[l] = g.t.x_out[l] = fake
        g.t.lp_out = g.t.ll_out = fake
        g.z_in[0] = g.z_out[0] = g.z_scales[0] = fake
        for k, v in kw.items():
            if k.startswith("t_"):
                setattr(g.t, k[2:], v)
            elif k in ("z_in", "z_out", "z_scales"):
                getattr(g, k)[0] = v
            else:
                setattr(g, k, v)
        return g

    move = lambda g, plan_=p: lib._gjx_temper_move_grouped(plan_, C.byref(g), None)
    tplan = plan.set_params(tr.params) if tr.params else plan
    assert move(io()) == INVALID  # a grouped plan without groups or data: nothing is launched
    assert lib._gjx_temper_plan_set_groups(p, fake, 5) == 0
    assert move(io()) == INVALID  # ... still without data
    assert lib._gjx_temper_plan_set_data(p, (C.c_void_p * 2)(fake, fake), 2, 13) == 0
    assert lib._gjx_temper_move_grouped(None, C.byref(io()), None) == INVALID and lib._gjx_temper_move_grouped(p, None, None) == INVALID
    for bad in (io(z_out=None), io(z_in=None), io(z_scales=None), io(t_n=0), io(t_n=1 << 31), io(t_impl=2), io(t_n_moves=257), io(t_lp_out=None),
                io(t_recompute=0), io(t_impl=0, init=1, init_key_lane=1), io(t_impl=0, t_key_lane=1)):
        assert move(bad) == INVALID
    # the entry points of the other headers refuse a grouped plan, and the grouped move refuses a plan without grouped sites
    t = io().t
    assert lib._gjx_temper_move(p, C.byref(t), None) == INVALID
    assert lib._gjx_temper_move_cov(p, C.byref(t), fake, None) == INVALID
    assert lib._gjx_pointwise_compile_check(p) == INVALID and lib._gjx_psis_compile_check(p) == INVALID
    assert lib._gjx_predictive_compile_check(p, 0) == INVALID and lib._gjx_temper_cov_compile_check(p, 0) == INVALID
    assert move(io(), flat_plan.handle) == INVALID
    del tplan


def _lower_plain(ops):  # noqa: F811
    import plate_ref as P

    with use_ops(ops):
        tr = temper.lower(P.target("normal", 20)[0], 64)
        return ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))


def test_tables_without_grouped_sites_keep_their_plan_and_source(ops):  # noqa: F811
    """A table without a grouped site gives, through the new creator, the plan and the source of the plated creator."""
    import plate_ref as P

    with use_ops(ops):
        tables = [temper.lower(R.models()["regression"], 64)] + [temper.lower(P.target(name, 20)[0], 64) for name in P.MODELS]
        for tr in tables:
            a = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
            arr = (abi.Site * len(tr.sites))(*tr.sites)
            h = C.c_void_p()
            ops.lib.call("gjx_temper_plan_create_grouped", arr, len(tr.sites), 0, C.byref(h))
            b = TemperPlan(ops, h, a.n_latents)
            assert ops.lib._gjx_temper_plan_n_grouped(h) == 0
            for impl in (0, 1):
                src = a.source(impl)
                assert src == b.source(impl) and "GroupArgs" not in src and "gz_" not in src
                assert a.cov_source(impl) == b.cov_source(impl)


def test_source_holds_no_length_no_group_count_and_no_data_value(ops, lowered):  # noqa: F811
    other = _lower(ops, "intercept", GR.LAYOUTS[17], seed=4)  # another data set, another g, another D — and another G
    for impl in (0, 1):
        src = lowered["intercept"][2].source(impl)
        assert src == other[2].source(impl)
        assert "gjx_temper_move_grouped_kernel" in src and "GroupArgs ga" in src and "(GroupOff)ga.off" in src and "ga.G" in src
        assert "__shared__" not in src and "__syncthreads" not in src and "GJX_BM_LDS" not in src
        assert "gjx_temper_move_kernel" not in src


def test_kernels_compile_for_gfx950_without_scratch(ops, lowered, tmp_path):  # noqa: F811
    for name in GR.MODELS:
        plan = lowered[name][2]
        for impl in (0, 1):
            assert plan.compile_check(impl) == 0, (name, impl)
            notes = kernel_notes(plan.source(impl), tmp_path, f"group_{name}_{impl}")["gjx_temper_move_grouped_kernel"]
            print(f"group kernel {name} impl {impl}: {notes}")
            assert notes["private_segment_fixed_size"] == 0, (name, impl, notes)
            assert notes["vgpr_count"] + notes.get("agpr_count", 0) <= 128, (name, impl, notes)  # four waves per SIMD or more


def test_replay_agrees_with_the_float64_restatement(oracle_ops):
    """assess of the replay (f32 terms, the header's sum order) against the float64 closed-form densities of
    group_ref.Intercepts at the same f32 inputs.  The floor: every f32 term of magnitude |t| carries a relative error of a few
    2^-24 from its own arithmetic (three operations and the rounding of a[g] + b x); the float64 sums add none, and the two
    final roundings half an ulp of the totals each."""
    sizes = GR.LAYOUTS[5]
    target, g, off = GR.target("intercept", sizes)
    with use_ops(oracle_ops):
        tr = _trace_only(target)
    xs, ys = tr.data[0].numpy(), tr.data[1].numpy()
    model = GR.Intercepts(xs, g, ys, len(sizes))
    rng = np.random.default_rng(11)
    x, z = GR.columns("intercept", len(sizes), 96, rng)
    assess = GR.Assess(oracle_ops, tr, [xs, ys], off)
    lp, ll = assess(x, z)
    lp64, ll64 = model.assess(x[0].astype(np.float64), x[1].astype(np.float64), z[0].astype(np.float64))
    # per particle: the sum of the terms' magnitudes bounds what their roundings can add up to
    D, G = len(g), len(sizes)
    mag_ll = sum(np.abs(model.acc(x[1].astype(np.float64), z[0][k].astype(np.float64), k)) for k in range(G)) + D * 3.0
    mag_lp = np.abs(lp64) + (2 + G) * 3.0
    eps = 2.0 ** -24
    assert np.all(np.abs(lp - lp64) <= 8 * eps * mag_lp), np.abs(lp - lp64).max()
    assert np.all(np.abs(ll - ll64) <= 8 * eps * mag_ll), np.abs(ll - ll64).max()


def _trace_only(target):
    return temper.lower(target, 64)


def test_closed_form_and_recorded_spreads():
    """The closed form against brute-force quadrature-free checks, and the constants the end-to-end GPU test is held to:
    one seed of the float64 restatement lies within E2E_FACTOR spreads (the 24-seed measurement is profiles/group_summary.md's)."""
    m = GR.e2e_model()
    assert m.D == 200 and m.G == 8 and len(m.post_mean) == 10 and np.all(m.post_sd > 0)
    # the posterior mean maximises lp + ll: its gradient vanishes there (central differences in float64)
    th = m.post_mean
    f = lambda t: float(sum(m.assess(np.array([t[0]]), np.array([t[1]]), t[2:, None])).sum())
    for k in range(len(th)):
        e = np.zeros_like(th)
        e[k] = 1e-4
        assert abs(f(th + e) - f(th - e)) / 2e-4 < 1e-5 * (1.0 + abs(f(th))), k
    # log Z = log p(theta*, y) - log p(theta* | y) at the posterior mean (the candidate's identity)
    _, logdet = np.linalg.slogdet(m.post_cov)
    assert abs(m.log_z - (f(th) + 0.5 * (len(th) * np.log(2 * np.pi) + logdet))) < 1e-8 * abs(m.log_z)
    assert GR.SPREAD_LOG_Z > 0 and len(GR.SPREAD_MEAN) == 2 + m.G and all(0 < s < 0.2 for s in GR.SPREAD_MEAN) and GR.E2E_FACTOR == 4.0
    ez, em = GR.restatement_errors(m, 8192, 2, [GR.E2E_SEEDS[0]])
    assert abs(ez[0]) <= GR.E2E_FACTOR * GR.SPREAD_LOG_Z and np.all(np.abs(em[0]) <= GR.E2E_FACTOR * np.asarray(GR.SPREAD_MEAN))
