"""include/gjx_plate_loglik.h without a GPU: the header's registration, the rule for R and C, every refusal before a launch,
and the two generated kernels of four models compiled for gfx950 offline."""

import ctypes as C

import pytest

import plate_ref as P
from genjax._amd import abi, temper
from genjax._amd.runtime import use_ops
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)
from test_gpu_counts import case as count_case

INVALID, WORKSPACE, MODELS = -1, -3, ("normal", "logistic", "pois_log", "negbin")


def target_of(name, D):  # plate_ref's regressions, test_gpu_counts' count regressions
    return P.target(name, D, seed=1)[0] if name in P.MODELS else count_case(name, D)[0]


def lower_all(ops, D):  # noqa: F811
    """Per model: (tracer, plan with its parameters set, the D data rows as float32 numpy columns)."""
    out = {}
    with use_ops(ops):
        for name in MODELS:
            tracer = temper.lower(target_of(name, D), 64)
            plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            plan.set_params(tracer.params)
            out[name] = (tracer, plan, [c.numpy() for c in tracer.data_columns("cpu")])
    return out


@pytest.fixture(scope="module")
def lowered(ops):  # noqa: F811
    return lower_all(ops, 20)


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.LOGLIK_HEADERS["plate_loglik"]
    assert header_symbols("gjx_plate_loglik.h") == set(h.prototypes) and not set(h.prototypes) & set(abi.PROTOTYPES)
    assert h not in abi.bound_headers() and abi.library_headers() == (*abi.bound_headers(), h)
    assert ops.lib.has["plate_loglik"] and not oracle_ops.lib.has["plate_loglik"]
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_plate_loglik_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.PLATE_LOGLIK_ABI_VERSION
    with pytest.raises(abi.PlateLoglikUnavailable, match="gjx_plate_loglik"):
        oracle_ops.lib.call("gjx_plate_loglik", None, None, None, 0, None)


@pytest.mark.parametrize("n, D, R, C_want", [
    (4096, 100_000, 0, 64),        # 16 tiles: 64 chunks of 1564 rows
    (65_536, 100_000, 0, 4),       # 256 tiles
    (261_888, 100_000, 0, 2),      # 1023 tiles: the last n with two chunks
    (261_889, 100_000, 0, 1),      # 1024 tiles: the particles fill the device
    (1_000_000, 1_000_000, 0, 1), (1, 37, 0, 1),
    (1, 65, 0, 2),                 # the minimum of 64 rows binds
    (1, 1_000_000, 4, 1021),       # the cap binds: R = 4 is raised to 980
    (1000, 131, 64, 3), (1000, 64, 64, 1), (1000, 65, 64, 2), (255, 5, 4, 2),
])
def test_chunks_and_workspace_follow_the_rule(ops, n, D, R, C_want):  # noqa: F811  (C_want: the header's rule by hand)
    chunks = lambda *a: ops.lib.call("gjx_plate_loglik_chunks", *a)  # noqa: E731
    nbytes = lambda *a: ops.lib.call("gjx_plate_loglik_workspace_bytes", *a)  # noqa: E731
    assert chunks(n, D, R) == C_want and nbytes(n, D, R, 1) == 8 * C_want * n and nbytes(n, D, R, 3) == 24 * C_want * n
    for bad in ((0, D, R), (1 << 31, D, R), (n, 0, R), (n, 1 << 31, R), (n, D, R + 2)):
        assert chunks(*bad) == 0 and nbytes(*bad, 1) == 0
    assert nbytes(n, D, R, 0) == 0 and nbytes(n, D, R, abi.MAX_SITES + 1) == 0


def _io(L=2, n=8, R=0):
    io = abi.PlateLoglikIO()
    io.impl, io.rows_per_chunk, io.n, io.ll_out, io.lp_out = 1, R, n, 0x4000, 0x5000
    for l in range(L):
        io.x_in[l] = 0x1000
    return io


def test_refusals_before_any_launch(ops):  # noqa: F811
    """(Host-side checks: the pointers are never dereferenced and no device is present.)"""
    import group_ref as G
    import temper_ref as R

    lib = ops.lib
    with use_ops(ops):
        tracer = temper.lower(target_of("normal", 20), 64)  # (a plan of its own: neither data nor parameters yet)
        flat = temper.lower(R.models()["regression"], 64)
        grouped = temper.lower(G.target("intercept", (3, 2, 4))[0], 64)
    plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
    call = lambda io, p=plan.handle, ws=0x8000, nb=1 << 20: lib._gjx_plate_loglik(p, C.byref(io) if io else None, ws, nb, None)  # noqa: E731
    assert call(_io()) == INVALID  # a plated plan without data
    lib.call("gjx_temper_plan_set_data", plan.handle, (C.c_void_p * 2)(0x6000, 0x7000), 2, 20)
    assert call(_io()) == INVALID  # ... and without the parameter its table reads
    plan.set_params(tracer.params)
    assert lib.call("gjx_temper_plan_n_plated", plan.handle) == 1 and lib.call("gjx_temper_plan_n_plated", None) == INVALID
    assert call(_io(), p=None) == INVALID and call(None) == INVALID
    for field, value in (("n", 0), ("n", 1 << 31), ("impl", 2), ("impl", -1), ("ll_out", None), ("rows_per_chunk", 6),
                         ("n_input_cols", -1), ("n_input_cols", 17), ("n_input_cols", 1)):
        io = _io()
        setattr(io, field, value)
        assert call(io) == INVALID, field
    assert call(_io(L=1)) == INVALID and call(_io(), ws=0x8004) == INVALID  # a latent column missing; ws misaligned
    assert call(_io(), ws=None) == WORKSPACE and call(_io(), nb=8 * 8 - 1) == WORKSPACE
    assert call(_io(R=4), nb=8 * 8 * 5 - 1) == WORKSPACE  # five chunks of four rows
    for tr in (flat, grouped):  # a plan without plated sites; a grouped plan
        p = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr)).set_params(tr.params)
        assert call(_io(L=p.n_latents), p=p.handle) == INVALID
        assert lib._gjx_plate_loglik_compile_check(p.handle, 0, 1) == INVALID
    assert lib._gjx_plate_loglik_compile_check(plan.handle, 2, 1) == INVALID and lib._gjx_plate_loglik_compile_check(plan.handle, 0, 2) == INVALID


@pytest.mark.parametrize("name", MODELS)
def test_kernels_compile_for_gfx950(lowered, name):
    plan = lowered[name][1]
    for impl in (0, 1):
        for kernel in ("rows", "fold"):
            assert plan.loglik_compile_check(kernel, impl) == 0, (name, kernel, impl)


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("name", ["normal", "pois_log"])
def test_rows_kernel_has_no_scratch(lowered, tmp_path, name, impl):
    k = kernel_notes(lowered[name][1].loglik_source("rows", impl), tmp_path, f"loglik_{name}_{impl}")["gjx_plate_loglik_rows_kernel"]
    print("row-chunk kernel", name, "impl", impl, k)
    assert k["private_segment_fixed_size"] == 0 and k["agpr_count"] == 0 and k["vgpr_count"] <= 64  # eight waves per SIMD
