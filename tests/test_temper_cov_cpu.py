"""The covariance proposal of the tempered sampler without a GPU: include/gjx_temper_cov.h as a header of its own (bound
through abi.MOVE_HEADERS), the C-side validation before any launch, the generated covariance move kernels compiled for gfx950
offline (no value in the source, no scratch), the Cholesky rule of tests/temper_cov_ref.py, the new arguments of TemperedSMC,
and the float64 restatement on the correlated regression that the GPU test's bounds come from."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import genjax
import temper_cov_ref as V
import temper_ref as R
from genjax import ChoiceMap, Target
from genjax._amd import abi, temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)

INVALID, WORKSPACE = -1, -3
SYMBOLS = {"gjx_temper_cov_version", "gjx_temper_moments_workspace_bytes", "gjx_temper_moments", "gjx_temper_move_cov",
           "gjx_temper_cov_source", "gjx_temper_cov_compile_check"}
KERNEL = "gjx_temper_move_cov_kernel"


def _lower(ops, target):  # noqa: F811
    with use_ops(ops):
        tracer = temper.lower(target, 64)
        return tracer, ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    targets = dict(R.models())
    targets["correlated_plated"] = V.correlated_target(plated=True)
    targets["gaussian16"] = V.gaussian_chain_target(16)
    return {name: _lower(ops, t) for name, t in targets.items()}


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.MOVE_HEADERS["temper_cov"]
    assert list(abi.MOVE_HEADERS) == ["temper_cov"] and abi.all_optional_headers()[-1] is h
    assert all("temper_cov" not in t for t in (abi.OPTIONAL_HEADERS, abi.EXTENSION_HEADERS, abi.PLAN_HEADERS))
    assert abi.all_optional_headers()[:-1] == (*abi.OPTIONAL_HEADERS.values(), *abi.EXTENSION_HEADERS.values(), *abi.PLAN_HEADERS.values())
    syms = header_symbols("gjx_temper_cov.h")
    assert h.header == "gjx_temper_cov.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.TEMPER_COV_PROTOTYPES and h.version == abi.TEMPER_COV_ABI_VERSION == (0, 1)
    assert h.unavailable is abi.TemperCovUnavailable and issubclass(abi.TemperCovUnavailable, abi.HeaderUnavailable)
    assert abi.TemperCovUnavailable.header == "gjx_temper_cov.h"
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    assert not (syms & header_symbols("gjx.h"))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_temper_cov and ops.lib.has["temper_cov"] and not oracle_ops.lib.has_temper_cov
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_temper_cov_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.TEMPER_COV_ABI_VERSION
    txt = open(__file__.replace("tests/test_temper_cov_cpu.py", "include/gjx_temper_cov.h")).read()
    assert f"GJX_TEMPER_COV_VERSION_MAJOR {major.value}" in txt and f"GJX_TEMPER_COV_VERSION_MINOR {minor.value}" in txt
    assert [f for f, _ in abi.TemperMomentsIO._fields_] == ["n", "n_latents", "x", "lw", "moments", "factor", "scales", "n_degenerate",
                                                            "ws", "ws_bytes", "max_workgroups"]
    assert C.sizeof(abi.TemperMomentsIO) == 8 + 8 + 8 * abi.TEMPER_MAX_LATENTS + 5 * 8 + 8 + 8 + 8
    import __graft_entry__ as g

    assert "gjx_temper_cov.h" in open(g.__file__).read()


def test_oracle_bound_ops_refuse(oracle_ops):
    with use_ops(oracle_ops):
        with pytest.raises(abi.HeaderUnavailable, match="gjx_temper"):
            TemperedSMC(V.correlated_target(), 64, proposal="covariance").run(genjax.random.key(1))
    with pytest.raises(abi.TemperCovUnavailable, match="gjx_temper_moments"):
        oracle_ops.temper_moments([torch.zeros(8)], None)
    with pytest.raises(abi.TemperCovUnavailable, match="gjx_temper_moments_workspace_bytes"):
        oracle_ops.temper_moments_workspace(8, 2)
    with pytest.raises(abi.TemperCovUnavailable, match="gjx_temper_move_cov"):
        oracle_ops.temper_move_cov(None, genjax.random.key(1), [torch.zeros(8)], None, None, 0.0, 0, torch.zeros(1))
    with pytest.raises(abi.TemperCovUnavailable):
        oracle_ops.lib.call("gjx_temper_cov_compile_check", None, 0)


def test_moments_validation(ops):  # noqa: F811
    """Every refusal is decided on the host, before anything is launched (the pointers are never followed)."""
    lib = ops.lib
    wb = lambda n, L: int(lib.call("gjx_temper_moments_workspace_bytes", n, L))
    assert wb(0, 2) == 0 and wb(1 << 31, 2) == 0 and wb(8, 0) == 0 and wb(8, abi.TEMPER_MAX_LATENTS + 1) == 0
    assert 0 < wb(8, 1) <= wb(1000, 2) < wb(10 ** 6, 2) < wb(10 ** 6, 16)
    # the ticket, the block maxima, W x P float64 block sums: each padded to 256 bytes
    assert wb(10 ** 6, 16) == 256 + 256 * 4 + 256 * 153 * 8 and wb((1 << 31) - 1, 16) == wb(10 ** 6, 16)
    n, L = 1000, 2
    need = wb(n, L)

    def io(**kw):
        o = abi.TemperMomentsIO()
        o.n, o.n_latents, o.lw = n, L, 0x3000
        o.x[0], o.x[1] = 0x1000, 0x2000
        o.moments, o.factor, o.scales, o.n_degenerate = 0x4000, 0x5000, 0x6000, 0x7000
        o.ws, o.ws_bytes = 0x8000, need
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    rc = lambda o: lib._gjx_temper_moments(C.byref(o) if o is not None else None, None)
    assert rc(None) == INVALID
    for kw in (dict(n=0), dict(n=1 << 31), dict(n_latents=0), dict(n_latents=-1), dict(n_latents=abi.TEMPER_MAX_LATENTS + 1),
               dict(moments=None), dict(factor=None), dict(scales=None), dict(n_degenerate=None), dict(ws=0x8004)):
        assert rc(io(**kw)) == INVALID, kw
    o = io()
    o.x[1] = None
    assert rc(o) == INVALID
    assert rc(io(ws=None)) == WORKSPACE and rc(io(ws_bytes=need - 1)) == WORKSPACE and rc(io(ws_bytes=0)) == WORKSPACE
    assert rc(io(n_latents=16, ws_bytes=need)) == INVALID  # (columns 2 .. 15 are NULL)
    o = io(n_latents=3)
    o.x[2] = 0x2800
    assert rc(o) == WORKSPACE  # more latents: the same workspace is too small


def test_move_cov_validation(ops, lowered):  # noqa: F811
    lib = ops.lib
    tracer, plan = lowered["regression"]
    plan.set_params(tracer.params)

    def io(**kw):
        o = abi.TemperIO()
        o.impl, o.n_moves, o.recompute, o.beta, o.n = 1, 2, 0, 0.5, 8
        for l in range(2):
            o.x_in[l], o.x_out[l] = 0x1000, 0x2000
        o.lp_in = o.ll_in = 0x3000
        o.lp_out = o.ll_out = 0x4000
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    F = C.c_void_p(0x5000)
    rc = lambda p, o, f: lib._gjx_temper_move_cov(p, C.byref(o) if o is not None else None, f, None)
    assert rc(plan.handle, io(), None) == INVALID  # a NULL factor: nothing is compiled, nothing launched
    assert rc(None, io(), F) == INVALID and rc(plan.handle, None, F) == INVALID
    for kw in (dict(n=0), dict(n=1 << 31), dict(impl=2), dict(impl=0, key_lane=3), dict(n_moves=-1), dict(n_moves=abi.TEMPER_MAX_MOVES + 1),
               dict(lp_out=None), dict(ll_out=None), dict(lp_in=None), dict(ll_in=None), dict(n_input_cols=-1), dict(n_input_cols=1)):
        assert rc(plan.handle, io(**kw), F) == INVALID, kw
    o = io()
    o.x_in[1] = None
    assert rc(plan.handle, o, F) == INVALID
    fresh = _lower(ops, R.models()["regression"])[1]  # the parameters of the table have to be set first
    assert rc(fresh.handle, io(), F) == INVALID
    assert lib._gjx_temper_cov_compile_check(None, 0) == INVALID and lib._gjx_temper_cov_compile_check(plan.handle, 2) == INVALID
    assert lib._gjx_temper_cov_source(None, 0, None, 0, None) == INVALID
    with pytest.raises(ValueError, match="factor"):
        ops.temper_move_cov(plan, genjax.random.key(1), [torch.zeros(8)] * 2, None, None, 0.0, 0, torch.zeros(2))


@pytest.mark.parametrize("name", ["regression", "gamma_normal", "beta_bernoulli", "correlated_plated", "gaussian16"])
def test_cov_kernels_compile_for_gfx950(lowered, name):
    plan = lowered[name][1]
    for impl in (0, 1):
        assert plan.cov_compile_check(impl) == 0, (name, impl)


def test_cov_source(ops, lowered):  # noqa: F811
    """The covariance kernel is the diagonal kernel with another "propose": the same tm_assess, the factor a pointer read through
    the constant address space, no value of a parameter, an observation or the factor in the text."""
    plan = lowered["regression"][1]
    reg, base = R.Regression(), R.models()["regression"]  # the same body over another noise and other observations
    other = _lower(ops, Target(base.p, ([float(x) for x in reg.xs], 0.25),
                               ChoiceMap.d({("y", i): float(3.0 * y + 1.0) for i, y in enumerate(reg.ys)})))[1]
    for impl in (0, 1):
        src, diag = plan.cov_source(impl), plan.source(impl)
        assert src == other.cov_source(impl)
        assert KERNEL in src and "gjx_temper_move_kernel" not in src and "gjx_temper_move_cov_kernel" not in diag
        assert "const float* factor" in src and "FactorPtr F = (FactorPtr)factor;" in src and "a.scales" not in src
        assert "F[0] * e0" in src and "t1 = t1 + F[2] * e1;" in src and "F[3]" not in src
        assert "__shared__" not in src and "__syncthreads" not in src
        head = lambda s: s.split('extern "C"')[0]
        assert head(src) == head(diag) + "typedef const __attribute__((address_space(4))) float* FactorPtr;\n"
    src16 = lowered["gaussian16"][1].cov_source(1)
    assert "t15 = t15 + F[135] * e15;" in src16 and "F[136]" not in src16
    srcp = lowered["correlated_plated"][1].cov_source(1)
    assert "const float* factor, PlateData pd) {" in srcp  # (PlateData stays the last argument)


@pytest.mark.parametrize("name", ["beta_bernoulli", "regression", "gaussian16"])
def test_cov_kernel_has_no_scratch(lowered, tmp_path, name):
    plan = lowered[name][1]
    for impl in (0, 1):
        k = kernel_notes(plan.cov_source(impl), tmp_path, f"temper_cov_{name}_{impl}")[KERNEL]
        d = kernel_notes(plan.source(impl), tmp_path, f"temper_diag_{name}_{impl}")["gjx_temper_move_kernel"]
        print("covariance move kernel,", name, "impl", impl, k, "| diagonal:", d)  # (profiles/temper_cov_summary.md records these)
        assert k["private_segment_fixed_size"] == 0
        if name == "regression":
            assert k["agpr_count"] == 0 and k["vgpr_count"] <= 128


def test_factor_ref_on_a_random_spd_matrix():
    """F F^T = c^2 S within 1e-6 relative to sqrt(S_ll S_jj): f32 rounding of the factor, 6e-8 per entry, over at most 16 terms."""
    rng = np.random.default_rng(3)
    for L in (1, 2, 5, 16):
        A = rng.standard_normal((L, L + 3))
        S = A @ A.T
        G, ndeg = V.factor_ref(V.pack(S), L)
        F = V.unpack(G.astype(np.float32), L).astype(np.float64)
        c2 = 2.38 ** 2 / L
        err = np.abs(F @ F.T - c2 * S) / (c2 * np.sqrt(np.outer(np.diag(S), np.diag(S))))
        print(f"L = {L}: largest relative error of F F^T {err.max():.2e}")
        assert ndeg == 0 and err.max() <= 1e-6 and np.all(np.diag(F) > 0)


def test_factor_ref_fallbacks():
    rng = np.random.default_rng(4)
    c = 2.38 / math.sqrt(3.0)
    cols = rng.standard_normal((3, 500))
    cols[2] = cols[0]  # a duplicated column
    S = np.cov(cols, bias=True)
    G, ndeg = V.factor_ref(V.pack(S), 3)
    F = V.unpack(G, 3)
    assert ndeg == 1 and F[2, 0] == 0.0 and F[2, 1] == 0.0 and F[2, 2] == c * math.sqrt(S[2, 2]) and F[1, 1] > 0
    cols[2] = 1.5  # a constant column: a zero row, and the latent stays put
    S = np.cov(cols, bias=True)
    assert S[2, 2] == 0.0
    G, ndeg = V.factor_ref(V.pack(S), 3)
    assert ndeg == 1 and np.all(V.unpack(G, 3)[2] == 0.0)
    # a row whose divisor is 0 takes 0 there: a constant column FIRST
    cols[0], cols[2] = 1.5, rng.standard_normal(500)
    G, ndeg = V.factor_ref(V.pack(np.cov(cols, bias=True)), 3)
    F = V.unpack(G, 3)
    assert ndeg == 1 and np.all(F[0] == 0.0) and F[1, 0] == 0.0 and F[2, 0] == 0.0 and F[1, 1] > 0 and F[2, 2] > 0
    for bad in (np.nan, np.inf, -1.0):
        G, ndeg = V.factor_ref([bad], 1)
        assert ndeg == 1 and G[0] == 0.0
    assert V.factor_ref([0.0], 1) == (np.array([0.0]), 1)


def test_moments_ref_matches_numpy():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 400)) + np.array([[10.0], [0.0], [-3.0]])
    lw = -20.0 * rng.chisquare(2, 400) * 0.01
    ws, mean, S = V.moments_ref(x, lw)
    w = np.exp(lw - lw.max())
    assert abs(ws - w.sum()) <= 1e-12 * ws and np.allclose(mean, (x * w).sum(axis=1) / w.sum(), rtol=0, atol=1e-12)
    assert np.allclose(V.unpack(S, 3), np.tril(np.cov(x, aweights=w, bias=True)), rtol=1e-12, atol=1e-14)
    holes = lw.copy()
    holes[::3] = -np.inf
    holes[1::6] = np.nan
    keep = np.isfinite(holes)
    a, b = V.moments_ref(x, holes), V.moments_ref(x[:, keep], holes[keep])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert V.moments_ref(x, np.full(400, -np.inf))[0] == 0.0


def test_temperedsmc_arguments():
    target = V.correlated_target()
    assert TemperedSMC(target, 64).proposal == "diagonal" and TemperedSMC(target, 64, proposal="covariance").proposal == "covariance"
    with pytest.raises(ValueError, match="proposal"):
        TemperedSMC(target, 64, proposal="full")
    with pytest.raises(ValueError, match="proposal"):
        TemperedSMC(target, 64, proposal=None)
    with pytest.raises(ValueError, match="scale"):
        TemperedSMC(target, 64, proposal="covariance", scale=0.1)
    assert TemperedSMC(target, 64, proposal="diagonal", scale=0.1).scale == 0.1


def test_correlated_targets_lower(ops):  # noqa: F811
    tr, plan = _lower(ops, V.correlated_target())
    assert plan.n_latents == 2 and len(tr.sites) == 22
    tr, plan = _lower(ops, V.correlated_target(37, plated=True))
    assert plan.n_latents == 2 and len(tr.sites) == 3 and tr.data_rows == 37 and tr.sites[2].observed == abi.SITE_PLATED
    tr, plan = _lower(ops, V.gaussian_chain_target(5))
    assert plan.n_latents == 5 and len(tr.sites) == 10
    m = V.correlated()
    corr = m.post_cov[0, 1] / math.sqrt(m.post_cov[0, 0] * m.post_cov[1, 1])
    assert -0.995 < corr < -0.99


def test_diagonal_restatement_is_tempered_f64():
    """tempered_cov_f64(proposal="diagonal") makes tempered_f64's draws in tempered_f64's order: the same numbers."""
    m = V.correlated()
    a = R.tempered_f64(m, 512, 2, 0.5, np.random.default_rng(5))
    b = V.tempered_cov_f64(m, 512, 2, 0.5, np.random.default_rng(5), proposal="diagonal")
    assert a["log_z"] == b["log_z"] and a["betas"] == b["betas"] and np.array_equal(a["w"], b["w"]) and np.array_equal(a["b"], b["b"])


def test_restatement_on_the_correlated_regression():
    """The float64 restatement at n = 4096, K = 2, ESS target 0.5 over default_rng(1000 .. 1063): the figures
    profiles/temper_cov_summary.md records and tests/test_gpu_temper_cov.py takes its bounds from.  The covariance proposal
    recovers the closed form within 5 x its RMS error on every seed, and its SMALLEST last-stage acceptance lies above the
    diagonal proposal's LARGEST: the premise of the end-to-end test."""
    model = V.correlated()
    ez, acc, em, vr = V.restatement_figures("covariance")
    dz, dacc, dm, dv = V.restatement_figures("diagonal")
    rms, drms = math.sqrt((ez ** 2).mean()), math.sqrt((dz ** 2).mean())
    print(f"closed form log Z {model.log_z:.4f}")
    print(f"covariance: RMS log Z error {rms:.4f} (from {ez.min():+.3f} to {ez.max():+.3f}), last-stage acceptance "
          f"{acc.min():.4f} / {acc.mean():.4f} / {acc.max():.4f}, variance / truth {vr.min():.2f} .. {vr.max():.2f}, worst mean "
          f"error {np.abs(em).max():.3f} sd")
    print(f"diagonal:   RMS log Z error {drms:.4f} (from {dz.min():+.3f} to {dz.max():+.3f}), last-stage acceptance "
          f"{dacc.min():.4f} / {dacc.mean():.4f} / {dacc.max():.4f}, variance / truth {dv.min():.2f} .. {dv.max():.2f}, worst mean "
          f"error {np.abs(dm).max():.3f} sd")
    assert np.abs(ez).max() <= 5.0 * rms
    assert acc.min() > dacc.max()
    assert np.abs(em).max() < 0.25
    # the constants the GPU test reads are these measurements
    assert abs(rms - V.COV_RMS_LOG_Z) < 5e-5 and abs(drms - V.DIAG_RMS_LOG_Z) < 5e-5
    assert abs(acc.min() - V.COV_MIN_ACCEPT) < 5e-5 and 0.0 <= V.DIAG_MAX_ACCEPT - dacc.max() < 1e-4
