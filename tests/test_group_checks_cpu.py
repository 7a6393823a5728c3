"""The check kernels of a plan with grouped latents without a GPU: include/gjx_group_checks.h as a header of its own, its
generated sources compiled for gfx950 offline (no scratch, no length, no data value), the C-side validation before any
launch, flat plans' sources unchanged against hashes recorded before the header existed, the Python layer's refusals, and
the float64 closed-form measurement behind the end-to-end tolerances."""

import ctypes as C
import re

import numpy as np
import pytest
import torch

import genjax
import group_checks_ref as GC
import group_ref as GR
from genjax import Target
from genjax._amd import abi, temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SYMBOLS = {"gjx_group_checks_version", "gjx_temper_pointwise_grouped", "gjx_temper_psis_grouped", "gjx_temper_predictive_grouped",
           "gjx_group_checks_source", "gjx_group_checks_compile_check"}
SIZES = GR.LAYOUTS[5]
KERNELS = (("pointwise", 0), ("psis", 0), ("predictive", 0), ("predictive", 1))
ENTRY = {"pointwise": "gjx_pointwise_grouped_kernel", "psis": "gjx_psis_grouped_kernel", "predictive": "gjx_predictive_grouped_kernel"}


def _lower(ops, name, sizes=SIZES, seed=0):  # noqa: F811
    with use_ops(ops):
        target, g, off = GR.target(name, sizes, seed)
        tracer = temper.lower(target, 64)
        return target, tracer, ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer)), g, off


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    return {name: _lower(ops, name) for name in GR.MODELS}


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.PLAN_HEADERS["group_checks"]
    keys = list(abi.PLAN_HEADERS)
    assert keys.index("group_checks") == keys.index("group") + 1 == keys.index("temper") - 1
    assert h in abi.all_optional_headers() and all("group_checks" not in t for t in (abi.OPTIONAL_HEADERS, abi.EXTENSION_HEADERS, abi.MOVE_HEADERS))
    assert len(abi.all_optional_headers()) == 15  # (with gjx.h: sixteen)
    syms = header_symbols("gjx_group_checks.h")
    assert h.header == "gjx_group_checks.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.GROUP_CHECKS_PROTOTYPES and h.version == abi.GROUP_CHECKS_ABI_VERSION == (0, 1)
    assert h.unavailable is abi.GroupChecksUnavailable and issubclass(abi.GroupChecksUnavailable, abi.HeaderUnavailable)
    assert abi.GroupChecksUnavailable.header == "gjx_group_checks.h"
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes)), other.header
    assert not (syms & header_symbols("gjx.h"))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_group_checks and ops.lib.has["group_checks"] and not oracle_ops.lib.has_group_checks
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_group_checks_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.GROUP_CHECKS_ABI_VERSION
    txt = open(__file__.replace("tests/test_group_checks_cpu.py", "include/gjx_group_checks.h")).read()
    for name, value in (("GJX_GROUP_CHECKS_VERSION_MAJOR", major.value), ("GJX_GROUP_CHECKS_VERSION_MINOR", minor.value)):
        assert f"#define {name} {value}" in txt
    assert C.sizeof(abi.GroupCols) == 8 * abi.GROUP_MAX_SITES
    with pytest.raises(abi.GroupChecksUnavailable, match="gjx_temper_pointwise_grouped"):
        oracle_ops.lib.call("gjx_temper_pointwise_grouped", None, None, None, None)


def test_sources_compile_for_gfx950_without_scratch(ops, lowered, tmp_path):  # noqa: F811
    """All three kernels over the four models, both generators for the predictive one: a source that compiles, reports no
    scratch, and holds neither G, n, n_rows nor a data value — it is the source of another data set, group layout and G."""
    others = {name: _lower(ops, name, GR.LAYOUTS[17], seed=4) for name in GR.MODELS}
    for name in GR.MODELS:
        plan, tr = lowered[name][2], lowered[name][1]
        assert plan.n_grouped == GR.GROUPED[name]
        for kern, impl in KERNELS:
            src = plan.group_checks_source(kern, impl)
            assert plan.group_checks_compile_check(kern, impl) == 0, (name, kern, impl)
            assert src == others[name][2].group_checks_source(kern, impl), (name, kern, impl)
            assert ENTRY[kern] + "(" in src and "GroupCols gc" in src and "group_of_row((GroupOff)gc.off, gc.G, d" in src
            assert "gjx_" + kern + "_kernel" not in src and "asm" not in src
            assert ("__shared__" in src) == (kern == "psis") and ("predictive_pass_key<%d>" % impl in src) == (kern == "predictive")
            # neither a length nor a data value: the source is that of another G, D and data set (above), and no f32 value of
            # the data columns appears as a literal
            data_bits = {"0x%08xu" % int(v) for c in tr.data for v in c.numpy().astype(np.float32).view(np.uint32)}
            lits = set(re.findall(r"0x[0-9a-f]{8}u", src))
            assert not (lits & (data_bits - {"0x00000000u", "0x3f800000u"})), (name, kern)
            notes = kernel_notes(src, tmp_path, f"gc_{name}_{kern}_{impl}")[ENTRY[kern]]
            print(f"group check kernel {name} {kern} impl {impl}: {notes}")
            assert notes["private_segment_fixed_size"] == 0, (name, kern, impl, notes)
            assert notes["vgpr_count"] + notes.get("agpr_count", 0) <= 128, (name, kern, impl, notes)  # four waves per SIMD or more
        # impl is read for the predictive kernel only
        assert plan.group_checks_source("pointwise", 7) == plan.group_checks_source("pointwise", 0)
        assert plan.group_checks_source("predictive", 0) != plan.group_checks_source("predictive", 1)
    # the term is ONE function text in the pointwise and the PSIS kernel
    term = lambda src, nm: src.split(nm + "(", 1)[1].split("\n}\n", 1)[0]
    for name in GR.MODELS:
        plan = lowered[name][2]
        assert term(plan.group_checks_source("pointwise"), "float pw_term") == term(plan.group_checks_source("psis"), "float ps_term")


def test_flat_sources_are_unchanged(ops):  # noqa: F811
    """The generated sources of flat plans — move, covariance move, pointwise, predictive and PSIS, both generators — hash to
    what they hashed to before the grouped modes of the generators existed (tests/golden/flat_temper_sources.json)."""
    golden, got = GC.flat_golden(), GC.flat_source_hashes(ops)
    assert len(golden) == 40 and set(golden) == set(got)
    assert got == golden, sorted(k for k in golden if got[k] != golden[k])
    for plan in GC.flat_plans(ops).values():
        for src in (plan.pointwise_source(), plan.psis_source(), plan.predictive_source(1)):
            assert "GroupCols" not in src and "gz_" not in src and "group_of_row" not in src


def test_abi_refusals(ops, lowered, monkeypatch):  # noqa: F811
    lib = ops.lib
    _, tr, plan, _, _ = _lower(ops, "intercept")
    p, fake, n, D, M = plan.handle, 0x1000, 4096, 13, 192
    monkeypatch.setenv("GJX_PLAN_JIT", "0")  # whatever passes validation stops at GJX_ERR_UNSUPPORTED: nothing is launched

    def cols(z0=0x7000):
        c = abi.GroupCols()
        c.z[0] = z0
        return c

    def fill(o, need, **kw):
        o.n, o.out, o.ws, o.ws_bytes = n, 0x4000, 0x8000, need
        for l in range(2):
            o.x[l] = fake * (l + 1)
        for k, v in kw.items():
            if k in ("x0", "x1"):
                o.x[int(k[1])] = v
            else:
                setattr(o, k, v)
        return o

    pw_io = lambda **kw: fill(abi.PointwiseIO(), int(lib.call("gjx_pointwise_workspace_bytes", n, D)), **kw)
    ps_io = lambda **kw: fill(abi.PsisIO(), int(lib.call("gjx_psis_workspace_bytes", n, D, M)), **{"tail_len": M, **kw})
    pd_io = lambda **kw: fill(abi.PredictiveIO(), int(lib.call("gjx_predictive_workspace_bytes", n, D, 1)), **kw)
    key = ops._keys(genjax.random.key(3, "philox").literal(), 1)
    ref = lambda v: C.byref(v) if v is not None else None
    pw = lambda io, c, plan_=p: lib._gjx_temper_pointwise_grouped(plan_, ref(io), ref(c), None)
    ps = lambda io, c, plan_=p: lib._gjx_temper_psis_grouped(plan_, ref(io), ref(c), None)
    pd = lambda io, c, plan_=p, k=key: lib._gjx_temper_predictive_grouped(plan_, ref(k), ref(io), ref(c), None)
    calls = ((pw, pw_io), (ps, ps_io), (pd, pd_io))
    if tr.params:
        plan.set_params(tr.params)
    for call, io in calls:  # a grouped plan without groups or without data
        assert call(io(), cols()) == INVALID
    assert lib._gjx_temper_plan_set_groups(p, fake, 5) == 0
    for call, io in calls:
        assert call(io(), cols()) == INVALID
    assert lib._gjx_temper_plan_set_data(p, (C.c_void_p * 2)(fake, fake), 2, D) == 0
    for call, io in calls:
        assert call(io(), cols()) == UNSUPPORTED  # valid: only the switched-off compiler stops it
        assert call(io(), None) == INVALID and call(io(), cols(None)) == INVALID and call(None, cols()) == INVALID
        assert call(io(), cols(), None) == INVALID
        # whatever the flat entry point refuses
        for bad in (io(n=0), io(n=1 << 31), io(out=None), io(x0=None), io(x1=None), io(ws=0x8004)):
            assert call(bad, cols()) == INVALID
        assert call(io(ws=None), cols()) == WORKSPACE and call(io(ws_bytes=8), cols()) == WORKSPACE
    for bad in (ps_io(tail_len=4), ps_io(tail_len=4096), ps_io(tail_len=n)):
        assert ps(bad, cols()) == INVALID
    assert pd(pd_io(draw_stride=1), cols()) == INVALID and pd(pd_io(), cols(), k=None) == INVALID
    batch = ops._keys(genjax.random.key(3, "philox").literal().with_fold(0), 1)
    assert pd(pd_io(), cols(), k=batch) == INVALID
    assert pd(pd_io(draws=0x9000, draw_stride=7), cols()) == UNSUPPORTED
    # a plan without grouped sites goes to the flat entry points, and a grouped plan does not
    import plate_ref as P

    with use_ops(ops):
        t2 = temper.lower(P.target("normal", 20)[0], 64)
        flat = ops.temper_plan_create(t2.sites, keep=(t2.keep, t2))
        if t2.params:
            flat.set_params(t2.params)
    assert lib._gjx_temper_plan_set_data(flat.handle, (C.c_void_p * 2)(fake, fake), 2, D) == 0
    for call, io in calls:
        assert call(io(), cols(), flat.handle) == INVALID
    assert lib._gjx_temper_pointwise(flat.handle, C.byref(pw_io()), None) == UNSUPPORTED
    assert lib._gjx_temper_pointwise(p, C.byref(pw_io()), None) == INVALID and lib._gjx_temper_psis(p, C.byref(ps_io()), None) == INVALID
    assert lib._gjx_temper_predictive(p, C.byref(key), C.byref(pd_io()), None) == INVALID
    need = C.c_size_t()
    assert lib._gjx_pointwise_source(p, None, 0, C.byref(need)) == INVALID and lib._gjx_psis_source(p, None, 0, C.byref(need)) == INVALID
    assert lib._gjx_predictive_source(p, 1, None, 0, C.byref(need)) == INVALID
    # source / compile_check: the kernel and, for the predictive kernel, the generator
    for k, impl in ((-1, 0), (3, 0), (2, 2), (2, -1)):
        assert lib._gjx_group_checks_source(p, k, impl, None, 0, C.byref(need)) == INVALID
        assert lib._gjx_group_checks_compile_check(p, k, impl) == INVALID
    for k in (0, 1, 2):
        assert lib._gjx_group_checks_source(None, k, 0, None, 0, C.byref(need)) == INVALID
        assert lib._gjx_group_checks_source(flat.handle, k, 0, None, 0, C.byref(need)) == INVALID
        assert lib._gjx_group_checks_compile_check(flat.handle, k, 0) == INVALID
        assert lib._gjx_group_checks_source(p, k, 0, None, 0, C.byref(need)) == 0 and need.value > 1000


def test_python_refusals(ops):  # noqa: F811
    """Before anything is uploaded or launched: the scalar columns alone, [G, n] columns of the wrong G or n, and held-out
    targets whose group tensor is unsorted, out of range or of another G."""
    with use_ops(ops):
        target, g, _ = GR.target("intercept", SIZES)
        key = genjax.random.key(1)
        alg = TemperedSMC(target, 64)
        scalars = [torch.zeros(64), torch.zeros(64)]
        for what, call in (("pointwise", lambda c: alg.pointwise(c)), ("loo", lambda c: alg.loo(c)),
                           ("predictive", lambda c: alg.predictive(c, key))):
            with pytest.raises(PlanUnsupported, match=f"{what}.*\\[G, n\\] column.*'a'.*missing"):
                call(scalars)
            with pytest.raises(ValueError, match=f"{what}.*'a'.*\\[5, 64\\].*\\(4, 64\\)"):
                call(scalars[:1] + [scalars[1], torch.zeros(4, 64)])  # the wrong G
            with pytest.raises(ValueError, match=f"{what}.*'a'.*\\[5, 64\\].*\\(5, 63\\)"):
                call(scalars + [torch.zeros(5, 63)])  # the wrong n
            with pytest.raises(ValueError, match=f"{what}.*'a'.*\\[5, 64\\]"):
                call(scalars + [torch.zeros(64)])  # not [G, n] at all
            with pytest.raises(ValueError, match=f"{what}.*3 latent columns expected"):
                call(scalars + [torch.zeros(5, 64)] * 2)
        with pytest.raises(PlanUnsupported, match="run_smc.*'a'"):
            alg.run_smc(key)
        with pytest.raises(PlanUnsupported, match="covariance.*'a'"):
            TemperedSMC(target, 64, proposal="covariance")._state()
        # held-out targets
        cols = scalars + [torch.zeros(5, 64)]
        xs, ys = target.args[0], target.constraint
        held = lambda gt, body=target.p: Target(body, (xs, gt), ys)
        unsorted = torch.from_numpy(g.copy())
        unsorted[0] = 4
        outside = torch.from_numpy(g.copy())
        outside[-1] = 5
        for what, call in (("pointwise", lambda t: alg.pointwise(cols, target=t)), ("predictive", lambda t: alg.predictive(cols, key, target=t))):
            with pytest.raises(ValueError, match=f"{what}.*'a'.*not sorted"):
                call(held(unsorted))
            with pytest.raises(ValueError, match=f"{what}.*'a'.*outside 0 .. 4.*never fitted"):
                call(held(outside))
            with pytest.raises(ValueError, match=f"{what}.*G = 6.*'a'.*G = 5"):
                call(held(torch.from_numpy(g), GR.body("intercept", 6)))
        # args= with a group that was never fitted
        with pytest.raises(ValueError, match="predictive.*outside 0 .. 4.*never fitted"):
            alg.predictive(cols, key, args=(xs, outside))


def test_references_agree(oracle_ops):
    """group_checks_ref.terms against the float64 closed-form densities of group_ref.Intercepts at the same f32 inputs (a few
    2^-24 of each term's magnitude: its own three operations and the rounding of a[g] + b x), g(d) against np.repeat, and
    the populations' spread below the condition of the lse tolerance on every layout."""
    import pointwise_ref as W

    for G, sizes in GC.LAYOUTS.items():
        off = np.concatenate([[0], np.cumsum(sizes)])
        assert np.array_equal(GC.group_of_rows(off, GC.ROWS[G]), GR.group_column(sizes)), G
    assert GC.ROWS == {1: 9, 2: 9, 5: 13, 17: 52, 7: 401}
    sizes = GR.LAYOUTS[17]
    target, g, off = GR.target("intercept", sizes)
    with use_ops(oracle_ops):
        tr = temper.lower(target, 64)
    xs, ys = tr.data[0].numpy(), tr.data[1].numpy()
    x, z = GC.centred_columns("intercept", sizes, 37, np.random.default_rng(3))
    t = GC.terms(GR.Assess(oracle_ops, tr, [xs, ys], off), x, z)
    m = GR.Intercepts(xs, g, ys, len(sizes))
    t64 = GC.terms_f64(m, x[1], z[0])
    assert t.shape == t64.shape == (52, 37) and np.all(np.abs(t - t64) <= 8 * 2.0 ** -24 * (np.abs(t64) + 3.0))
    assert W.spread(t).max() < W.LSE_MAX_SPREAD / 4
    # the generating values are the data's: residuals of the centred population stay within a few noise deviations
    assert np.abs(ys[:, None] - (z[0][g] + x[1][None, :] * xs[:, None])).max() < 6 * 0.5


def test_closed_form_and_recorded_spreads():
    """The closed forms against each other and the recorded constants against a fresh measurement on two seeds (each within
    the 24-seed range group_checks_ref records, by construction of that range)."""
    m = GR.e2e_model()
    mean, V = GC.closed_form(m)
    assert mean.shape == V.shape == (200,) and np.all(V > m.noise ** 2)
    # leave-one-out densities lie below the full-data ones in total (a row's own evidence is gone) and close to them
    lppd, loo = GC.closed_form_lppd(m), GC.closed_form_loo(m)
    assert loo.sum() < lppd.sum() and abs(loo.sum() - lppd.sum()) < 0.1 * abs(lppd.sum())
    # one row by brute force: the posterior refitted without it
    d = 17
    keep = np.arange(m.D) != d
    sub = GR.Intercepts(m.xs[keep].astype(np.float32), m.g[keep], m.ys[keep].astype(np.float32), m.G)
    assert abs(GC.closed_form_lppd(sub, m.xs[d:d + 1], m.g[d:d + 1], m.ys[d:d + 1])[0] - loo[d]) < 1e-9
    assert GC.E2E_FACTOR == 4.0 and GC.E2E_N == 8192 and len(GC.E2E_SEEDS) == 24 and GC.E2E_MAX_KHAT < 0.7
    e = GC.e2e_errors(m, GC.E2E_N, GC.E2E_SEEDS[:2])
    print(e)
    # the measurement itself: the two populations give the recorded values, digit for digit
    assert np.all(np.abs(e - np.array(GC.E2E_FIRST_SEEDS)) <= 1e-5), np.abs(e - np.array(GC.E2E_FIRST_SEEDS)).max()
    lo, hi = np.array(GC.E2E_RANGE).T
    assert np.all(e >= lo - 1e-4) and np.all(e <= hi + 1e-4)
    # the recorded RMS values: each between the smallest and the largest magnitude of its 24 per-seed values, and the two
    # repeated seeds' part of its square sum does not exceed the whole
    recorded = np.array((GC.SPREAD_LPPD_SUM, GC.SPREAD_HELD_SUM, GC.SPREAD_ELPD_SUM, GC.SPREAD_MEAN, GC.SPREAD_VAR, GC.SPREAD_PIT))
    largest = np.maximum(np.abs(lo), np.abs(hi))[:6]
    smallest = np.where(lo[:6] > 0, lo[:6], 0.0)
    assert np.all(recorded <= largest) and np.all(recorded >= smallest)
    assert np.all((e[:, :6] ** 2).sum(axis=0) <= 24 * recorded ** 2 * (1 + 1e-2))
    assert GC.E2E_MAX_KHAT == hi[6]
