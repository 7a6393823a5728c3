"""Pointwise predictive densities of a plated tempered plan without a GPU: include/gjx_pointwise.h as a header of its own,
the generated pointwise kernel compiled for gfx950 offline (one source per plan, no data in it, no scratch), the move
kernels' sources left as they were, the C-side validation before any launch, the chunk rule, the host logic of
PointwiseLikelihood, the refusals of `target=`, and the numpy reference against the closed form of the conjugate regression."""

import ctypes as C
import hashlib
import math

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import pointwise_ref as W
import temper_ref as R
from genjax import ChoiceMap, Target, gen, normal
from genjax._amd import abi, temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PointwiseLikelihood, TemperedSMC
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
SYMBOLS = {"gjx_pointwise_version", "gjx_pointwise_chunks", "gjx_pointwise_workspace_bytes", "gjx_temper_pointwise",
           "gjx_pointwise_source", "gjx_pointwise_compile_check"}

# sha256 of the generated MOVE kernel sources (TemperPlan.source(impl)) of plate_ref.MODELS lowered from 20 rows, generated
# with the build of the commit before the pointwise kernels existed: they add nothing to and change nothing in those sources.
MOVE_SOURCE_SHA256 = {
    ("normal", 0): "65fd151cc0bde5c1c4194225bc2b7ac0b749d2b164b5ffaca0d39e217b2440ce",
    ("normal", 1): "54ea155818ee8bcade0388aa1aa8b6b31024d70f5686151071513603706976bf",
    ("hetero", 0): "f981378f3e4d8a5c812441eeb9f896009f8dfd630116b61cb23a59e2370adca0",
    ("hetero", 1): "62b4e0b20716fd6a1618dcefc3bc4dde5daf8e61637033b8aba9a49035358093",
    ("logistic", 0): "fe5a70112457fb2d43d873d86e33ab902c8e4c70c4501a1d40c908a71ea9e363",
    ("logistic", 1): "6781db23c368582005ae57b71d2d929bd258dda3a079562222e3b1b9768f0eda",
    ("gamma_rate", 0): "6a579cd3ae075bd87a69b48e4cd9e716f143b6fb642ee7acb73601229a5af92b",
    ("gamma_rate", 1): "e5fcb506f98ece7943c96b43c3b375585a7755be558070c401c40940da1361be",
}


def _lower(ops, name, D, seed=0):  # noqa: F811
    with use_ops(ops):
        target, data = P.target(name, D, seed)
        tracer = temper.lower(target, 64)
        return target, tracer, ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer)), data


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    return {name: _lower(ops, name, 20) for name in P.MODELS}


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.PLAN_HEADERS["pointwise"]
    assert list(abi.PLAN_HEADERS)[-1] == "pointwise" and h in abi.all_optional_headers()
    assert "pointwise" not in abi.OPTIONAL_HEADERS and "pointwise" not in abi.EXTENSION_HEADERS
    syms = header_symbols("gjx_pointwise.h")
    assert h.header == "gjx_pointwise.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.POINTWISE_PROTOTYPES and h.version == abi.POINTWISE_ABI_VERSION and h.unavailable is abi.PointwiseUnavailable
    assert issubclass(abi.PointwiseUnavailable, abi.HeaderUnavailable) and abi.PointwiseUnavailable.header == "gjx_pointwise.h"
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    assert not (syms & header_symbols("gjx.h"))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_pointwise and ops.lib.has["pointwise"] and not oracle_ops.lib.has_pointwise
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_pointwise_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.POINTWISE_ABI_VERSION
    txt = open(__file__.replace("tests/test_pointwise_cpu.py", "include/gjx_pointwise.h")).read()
    assert f"GJX_POINTWISE_VERSION_MAJOR {major.value}" in txt and f"GJX_POINTWISE_VERSION_MINOR {minor.value}" in txt
    assert [f for f, _ in abi.PointwiseIO._fields_] == ["n", "x", "out", "ws", "ws_bytes"]
    assert C.sizeof(abi.PointwiseIO) == 8 + 8 * abi.TEMPER_MAX_LATENTS + 3 * 8


def test_oracle_bound_ops_refuse(oracle_ops):
    target, _ = P.target("normal", 20)
    cols = [torch.zeros(8), torch.zeros(8)]
    with use_ops(oracle_ops):
        with pytest.raises(abi.HeaderUnavailable, match="gjx_temper|gjx_plate|gjx_pointwise"):
            TemperedSMC(target, 64).pointwise(cols)
    with pytest.raises(abi.PointwiseUnavailable, match="gjx_temper_pointwise"):
        oracle_ops.lib.call("gjx_temper_pointwise", None, None, None)
    with pytest.raises(abi.PointwiseUnavailable, match="gjx_pointwise_chunks"):
        oracle_ops.lib.call("gjx_pointwise_chunks", 1, 1)


@pytest.mark.parametrize("name", P.MODELS)
def test_pointwise_source(ops, lowered, name):  # noqa: F811
    """One source per plan: it compiles for gfx950, is the same text for D = 20 and D = 1000 and for other data values,
    holds no data value, no LDS, no barrier and no inline assembly, and reads the latent columns through the constant
    address space (scalar loads)."""
    plan, data = lowered[name][2], lowered[name][3]
    src = plan.pointwise_source()
    assert plan.pointwise_compile_check() == 0
    assert src == _lower(ops, name, 1000, seed=3)[2].pointwise_source() == _lower(ops, name, 20, seed=5)[2].pointwise_source()
    assert "gjx_pointwise_kernel(PointwiseArgs a, PlanParams prm, PlanTables tabs, PlateData pd)" in src
    assert "(PlateCol)a.x[0]" in src and "pd.n_rows" in src and "pointwise_take<4>" in src and "pointwise_take<1>" in src
    assert "__shared__" not in src and "__syncthreads" not in src and "asm" not in src and "gjx_temper_move_kernel" not in src
    for t in data:  # no data value as a literal (literals are hex words: gjx_plan_jit.hpp flit)
        for v in t.to(torch.float32).numpy().view(np.uint32):
            assert f"0x{int(v):08x}u" not in src or v in (0, 0x3f800000)


@pytest.mark.parametrize("name", ["normal", "logistic"])
def test_pointwise_kernel_has_no_scratch(lowered, tmp_path, name):
    k = kernel_notes(lowered[name][2].pointwise_source(), tmp_path, f"pointwise_{name}")["gjx_pointwise_kernel"]
    print("pointwise kernel,", name, k)  # (profiles/pointwise_summary.md records these)
    assert k["private_segment_fixed_size"] == 0 and k["agpr_count"] == 0
    assert k["vgpr_count"] <= 128  # four waves per SIMD out of 512 registers


def test_move_sources_are_the_parents(lowered):
    for (name, impl), want in MOVE_SOURCE_SHA256.items():
        assert hashlib.sha256(lowered[name][2].source(impl).encode()).hexdigest() == want, (name, impl)


def test_chunks_and_workspace(ops):  # noqa: F811
    lib = ops.lib
    ch = lambda n, D: int(lib.call("gjx_pointwise_chunks", n, D))
    ws = lambda n, D: int(lib.call("gjx_pointwise_workspace_bytes", n, D))
    rule = lambda n, D: min(-(-n // 256), max(1, -(-2048 // -(-D // 256))))
    cases = [(1, 1), (256, 1), (257, 1), (1000, 513), (10 ** 6, 64), (10 ** 6, 1000), (10 ** 6, 10000), (2 ** 31 - 1, 2 ** 31 - 1),
             (10 ** 6, 256 * 2048), (10 ** 6, 256 * 2048 + 1), (5000, 257)]
    for n, D in cases:
        assert ch(n, D) == rule(n, D) == ch(n, D), (n, D)
        assert ws(n, D) == 40 * ch(n, D) * D, (n, D)
    assert ch(257, 20) == 2 and ch(1000, 20) == 4 and ch(10 ** 6, 1000) == 512 and ch(10 ** 6, 64) == 2048 and ch(10 ** 6, 10000) == 52
    assert ws(10 ** 6, 1000) == 512 * 1000 * 40  # 20 MB
    for n, D in ((0, 5), (5, 0), (1 << 31, 5), (5, 1 << 31)):
        assert ch(n, D) == 0 and ws(n, D) == 0


def test_pointwise_validation(ops, lowered, monkeypatch):  # noqa: F811
    """Every refusal is decided on the host, before anything is compiled or launched (the pointers are never followed)."""
    lib = ops.lib
    _, tr, plan, _ = _lower(ops, "normal", 20, seed=9)  # (a plan of its own: no parameters, no data yet)
    D, n = 20, 1000
    need = int(lib.call("gjx_pointwise_workspace_bytes", n, D))

    def io(**kw):
        o = abi.PointwiseIO()
        o.n, o.out, o.ws, o.ws_bytes = n, 0x4000, 0x8000, need
        for l in range(2):
            o.x[l] = 0x1000 * (l + 1)
        for k, v in kw.items():
            if k == "x0":
                o.x[0] = v
            elif k == "x1":
                o.x[1] = v
            else:
                setattr(o, k, v)
        return o

    call = lambda p, o: lib._gjx_temper_pointwise(p, C.byref(o) if o is not None else None, None)
    monkeypatch.setenv("GJX_PLAN_JIT", "0")  # whatever passes validation stops at GJX_ERR_UNSUPPORTED: nothing is launched
    assert call(plan.handle, io()) == INVALID  # fewer parameters than the table reads (none set)
    plan.set_params(tr.params)
    assert call(plan.handle, io()) == INVALID  # a plated plan without data
    cols = (C.c_void_p * 2)(0x5000, 0x6000)
    assert lib._gjx_temper_plan_set_data(plan.handle, cols, 2, D) == 0
    assert call(plan.handle, io()) == UNSUPPORTED  # valid: only the switched-off compiler stops it
    assert call(None, io()) == INVALID and call(plan.handle, None) == INVALID
    assert call(plan.handle, io(x0=None)) == INVALID and call(plan.handle, io(x1=None)) == INVALID and call(plan.handle, io(out=None)) == INVALID
    assert call(plan.handle, io(n=0)) == INVALID and call(plan.handle, io(n=1 << 31)) == INVALID
    assert call(plan.handle, io(ws=0x8004)) == INVALID  # not 8-byte aligned
    assert call(plan.handle, io(ws=None)) == WORKSPACE and call(plan.handle, io(ws_bytes=need - 1)) == WORKSPACE
    assert call(plan.handle, io(n=(1 << 31) - 1)) == WORKSPACE  # (a larger population needs a larger workspace)
    # a plan without a PLATED site has no pointwise kernel
    with use_ops(ops):
        t2 = temper.lower(R.models()["regression"], 64)
        flat = ops.temper_plan_create(t2.sites, keep=(t2.keep, t2))
        flat.set_params(t2.params)
    assert call(flat.handle, io()) == INVALID and flat.pointwise_compile_check() == INVALID
    assert lib._gjx_pointwise_source(flat.handle, None, 0, C.byref(C.c_size_t())) == INVALID
    assert lib._gjx_pointwise_source(None, None, 0, C.byref(C.c_size_t())) == INVALID and lib._gjx_pointwise_compile_check(None) == INVALID
    with pytest.raises(ValueError, match="no plated site"):
        ops.temper_pointwise(flat, [torch.zeros(4), torch.zeros(4)])


def test_pointwise_likelihood_host_logic():
    n, D = 5, 4
    rng = np.random.default_rng(0)
    t = rng.standard_normal((D, n))
    table = torch.from_numpy(W.reduce64(t))
    pw = PointwiseLikelihood(table, n)
    lppd = np.log(np.exp(t).mean(axis=1))
    var = t.var(axis=1, ddof=1)
    assert np.allclose(pw.lppd.numpy(), lppd, rtol=0, atol=1e-12) and np.allclose(pw.mean.numpy(), t.mean(axis=1), rtol=0, atol=1e-12)
    assert np.allclose(pw.var.numpy(), var, rtol=0, atol=1e-12) and torch.equal(pw.count, torch.full((D,), float(n), dtype=torch.float64))
    assert pw.lppd.dtype == pw.var.dtype == pw.mean.dtype == torch.float64 and pw.lppd.shape == (D,)
    assert math.isclose(pw.log_predictive_density, lppd.sum(), abs_tol=1e-12) and math.isclose(pw.p_waic, var.sum(), abs_tol=1e-12)
    assert math.isclose(pw.elpd_waic, (lppd - var).sum(), abs_tol=1e-12) and pw.waic == -2.0 * pw.elpd_waic
    assert math.isclose(pw.elpd_waic, pw.log_predictive_density - pw.p_waic, abs_tol=1e-12)
    assert math.isclose(pw.elpd_waic_se, math.sqrt(D * np.var(lppd - var, ddof=1)), abs_tol=1e-12)
    # n = 1: no variance to speak of — zeros, WAIC = -2 lppd
    one = PointwiseLikelihood(torch.from_numpy(W.reduce64(t[:, :1])), 1)
    assert torch.equal(one.var, torch.zeros(D, dtype=torch.float64)) and one.p_waic == 0.0
    assert np.allclose(one.lppd.numpy(), t[:, 0], rtol=0, atol=1e-15) and math.isclose(one.waic, -2.0 * t[:, 0].sum(), abs_tol=1e-12)
    # a row no particle gives a density above 0: lppd = -inf there, and it propagates
    t2 = t.copy()
    t2[1] = -np.inf
    dead = PointwiseLikelihood(torch.from_numpy(W.reduce64(t2)), n)
    assert dead.count[1] == 0 and dead.lppd[1] == -math.inf and torch.isfinite(dead.lppd[[0, 2, 3]]).all()
    assert dead.log_predictive_density == -math.inf and math.isnan(dead.var[1].item())  # (-inf) - (-inf)^2 / n
    with pytest.raises(ValueError):
        PointwiseLikelihood(table.float(), n)
    with pytest.raises(ValueError):
        PointwiseLikelihood(table, 0)


def test_target_refusals(ops):  # noqa: F811
    target, _ = P.target("normal", 20)
    cols = [torch.zeros(8), torch.zeros(8)]

    @gen
    def other_names(xs, s):
        w = normal(0.0, 2.0) @ "slope"
        b = normal(0.0, 2.0) @ "b"
        normal(w * xs + b, s) @ "y"

    @gen
    def swapped(xs, s):
        b = normal(0.0, 2.0) @ "b"
        w = normal(0.0, 2.0) @ "w"
        normal(w * xs + b, s) @ "y"

    @gen
    def unplated(s):
        w = normal(0.0, 2.0) @ "w"
        b = normal(0.0, 2.0) @ "b"
        normal(w + b, s) @ "y"

    xs, ys = torch.linspace(0.0, 1.0, 7), torch.ones(7)
    with use_ops(ops):
        alg = TemperedSMC(target, 64)
        with pytest.raises(ValueError, match=r"\['slope', 'b'\].*\['w', 'b'\]"):
            alg.pointwise(cols, target=Target(other_names, (xs, 0.1), ChoiceMap.d({"y": ys})))
        with pytest.raises(ValueError, match=r"\['b', 'w'\].*\['w', 'b'\]"):
            alg.pointwise(cols, target=Target(swapped, (xs, 0.1), ChoiceMap.d({"y": ys})))
        with pytest.raises(PlanUnsupported, match="no plated site.*'y'"):
            alg.pointwise(cols, target=Target(unplated, (0.1,), ChoiceMap.d({"y": 0.5})))
        with pytest.raises(PlanUnsupported, match="no plated site"):
            TemperedSMC(Target(unplated, (0.1,), ChoiceMap.d({"y": 0.5})), 64).pointwise(cols)
        with pytest.raises(ValueError, match="2 latent columns"):
            alg.pointwise(cols[:1])
        with pytest.raises(TypeError):
            alg.pointwise(cols, target="held out")


def test_reference_recovers_the_closed_form():
    """The float64 numpy reference on populations drawn from the exact posterior of the conjugate regression with 500 rows,
    n = 8192: two seeds outside the 24 the spread was measured over land within four times that spread of
    sum_d log N(y_d; x_d' mu, noise^2 + x_d' Sigma x_d)."""
    model = P.conjugate(500)
    err = W.closed_form_errors(model, 8192, (6000, 6001))
    print("sum lppd minus the closed form", err, "bound", W.CLOSED_FORM_FACTOR * W.SPREAD_LPPD_SUM, "closed form", W.closed_form_lppd(model).sum())
    assert np.all(np.abs(err) <= W.CLOSED_FORM_FACTOR * W.SPREAD_LPPD_SUM)
