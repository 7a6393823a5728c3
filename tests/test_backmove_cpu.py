"""The MCMC backward sampler without a GPU: include/gjx_backmove.h as a fifth header (libgjx_hip.so exports it, the oracle
does not; bound through abi.EXTENSION_HEADERS), gjx_backmove_run's validation before any launch, the generated move kernels
compiled for gfx950 offline, and the reference of tests/backmove_ref.py held against trace-back and the exact smoother."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import backmove_ref as M
import backsim_ref as B
import genjax
from genjax._amd import abi, workloads as W
from genjax._amd.abi import GjxError
from genjax._amd.runtime import use_ops
from genjax._amd.smc_plan import build_transition_table
from genjax.inference.smc import BootstrapSMC, GuidedSMC, LinearGaussianSSM, StateSpaceModel
from offline import ROOT, header_symbols, kernel_notes, ops, source_shape  # noqa: F401

Y = [("y",)]
SYMBOLS = {"gjx_backmove_version", "gjx_backmove_plan_source", "gjx_backmove_plan_compile_check", "gjx_backmove_workspace_bytes",
           "gjx_backmove_run"}


def _table(ops, model, addrs=Y):
    with use_ops(ops):
        return build_transition_table(StateSpaceModel(*model), addrs)


# ---- the header and its bindings ---------------------------------------------------------------------------------------
def test_the_fifth_header_is_exported_by_the_hip_library_only(ops, oracle_ops):
    assert len(abi.OPTIONAL_HEADERS) == 3 and list(abi.EXTENSION_HEADERS) == ["backmove"]
    h = abi.EXTENSION_HEADERS["backmove"]
    syms = header_symbols(h.header)
    assert h.header == "gjx_backmove.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.BACKMOVE_PROTOTYPES and h.version == abi.BACKMOVE_ABI_VERSION and h.unavailable is abi.BackmoveUnavailable
    assert not (syms & header_symbols("gjx.h")) and not (syms & set(abi.PROTOTYPES))
    for other in abi.OPTIONAL_HEADERS.values():
        assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_backmove and ops.lib.has["backmove"] and not oracle_ops.lib.has_backmove
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_backmove_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.BACKMOVE_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", h.header)).read()
    assert f"GJX_BACKMOVE_VERSION_MAJOR {major.value}" in hdr and f"GJX_BACKMOVE_VERSION_MINOR {minor.value}" in hdr
    assert f"GJX_BACKMOVE_MAX_MOVES {abi.BACKMOVE_MAX_MOVES}" in hdr
    # gjx_backmove_io = the fields of gjx_backsim_io, then three more
    n = len(abi.BacksimIO._fields_)
    assert abi.BackmoveIO._fields_[:n] == abi.BacksimIO._fields_
    assert [f for f, _ in abi.BackmoveIO._fields_[n:]] == ["ancestors", "anc_stride", "n_moves"]
    for f, _ in abi.BacksimIO._fields_:
        assert getattr(abi.BackmoveIO, f).offset == getattr(abi.BacksimIO, f).offset, f


def test_the_workspace_size_contract(ops):
    wb = lambda T, n, m: ops.lib.call("gjx_backmove_workspace_bytes", T, n, m)
    pad = lambda b: (b + 255) & ~255
    for T, n, m in ((1, 1, 1), (6, 1000, 7), (100, 1_000_000, 1_000_000), (3, 70_000, 300)):
        nt = (n + 1023) // 1024
        # tile maxima, tile masses, the maximum, the CDF, the lineage rows: each padded to 256 bytes
        assert wb(T, n, m) == pad(4 * nt) + pad(8 * nt) + pad(4) + pad(8 * n) + pad(4 * T * m), (T, n, m)
    assert wb(0, 8, 8) == 0 and wb(3, 0, 8) == 0 and wb(3, 8, 0) == 0 and wb(3, 1 << 31, 8) == 0 and wb(3, 8, 1 << 31) == 0


# ---- validation on the host, before any launch -------------------------------------------------------------------------
def _io(T=3, n=8, m=8, K=2):
    """A VALID call description over dummy non-null addresses (the tests below break one thing at a time and never reach a
    launch: the last check before the compiler is the workspace's, which they fail on purpose where nothing else does)."""
    io = abi.BackmoveIO()
    io.n_steps, io.impl, io.n, io.m = T, 1, n, m
    io.cols[0], io.col_stride[0] = 0x2000, n
    io.logw, io.logw_stride = 0x3000, n
    io.obs = 0x7000  # (the user-written LGSSM's table reads one observation column; the rows are read after the last check)
    io.lineage_out, io.lineage_stride = 0x4000, m
    io.paths_out[0], io.paths_stride[0] = 0x5000, m
    io.ancestors, io.anc_stride, io.n_moves = 0x6000, n, K
    return io


def test_invalid_calls_are_refused_before_any_launch(ops):
    INVALID, WORKSPACE = -1, -3
    plan = ops.backsim_plan_create(_table(ops, B.lgssm_model()))
    rc = lambda io, ws=0x8000, nb=0: ops.lib._gjx_backmove_run(plan.handle, C.byref(io) if io is not None else None, C.c_void_p(ws), nb, None)
    # the valid description passes every check up to the workspace's (too small here: nothing is compiled or launched)
    assert rc(_io()) == WORKSPACE and rc(_io(), ws=0, nb=1 << 20) == WORKSPACE
    need = ops.lib.call("gjx_backmove_workspace_bytes", 3, 8, 8)
    assert rc(_io(), nb=need - 1) == WORKSPACE
    assert rc(None) == INVALID and ops.lib._gjx_backmove_run(None, C.byref(_io()), C.c_void_p(0x8000), 0, None) == INVALID
    bad = []
    for field, value in (("n_steps", 0), ("n", 0), ("m", 0), ("n", 1 << 31), ("m", 1 << 31), ("impl", 2), ("impl", -1),
                         ("n_moves", -1), ("n_moves", 257), ("ancestors", None), ("anc_stride", 7), ("anc_stride", 1 << 32),
                         ("logw", None), ("obs", None), ("logw_stride", 7), ("logw_stride", 1 << 32), ("lineage_stride", 7)):
        io = _io()
        setattr(io, field, value)
        bad.append((field, value, rc(io)))
    assert all(r == INVALID for _, _, r in bad), bad
    io = _io(m=1 << 23, K=256)  # m K = 2^31
    assert rc(io) == INVALID
    io = _io(m=(1 << 23) - 1, K=256)  # ... and just below it
    assert rc(io) == WORKSPACE
    io = _io(m=(1 << 31) - 1, K=0)  # K = 0 counts as one draw per path: the leaves
    assert rc(io) == WORKSPACE
    io = _io(); io.impl = 0; io.key_lane = 3  # a lane with THREEFRY
    assert rc(io) == INVALID
    io = _io(); io.cols[0] = None
    assert rc(io) == INVALID
    io = _io(); io.col_stride[0] = 7
    assert rc(io) == INVALID
    io = _io(); io.paths_stride[0] = 7
    assert rc(io) == INVALID
    io = _io(); io.lineage_out = None; io.paths_out[0] = None  # no output at all
    assert rc(io) == INVALID
    io = _io(); io.lineage_out = None  # paths alone: the lineage rows live in the workspace
    assert rc(io) == WORKSPACE
    assert rc(_io(), ws=0x8004, nb=1 << 20) == INVALID  # not 8-byte aligned
    # every state column of the plan is required
    plan2 = ops.backsim_plan_create(_table(ops, B.two_component_model()))
    assert ops.lib._gjx_backmove_run(plan2.handle, C.byref(_io()), C.c_void_p(0x8000), 0, None) == INVALID
    io = _io(); io.cols[1], io.col_stride[1] = 0x2800, 8
    assert ops.lib._gjx_backmove_run(plan2.handle, C.byref(io), C.c_void_p(0x8000), 0, None) == WORKSPACE
    for fn in ("_gjx_backmove_plan_compile_check",):
        assert getattr(ops.lib, fn)(None, 0) == INVALID and getattr(ops.lib, fn)(plan.handle, 2) == INVALID


def test_ops_refuses_bad_tensors_without_a_gpu(ops):
    plan = ops.backsim_plan_create(_table(ops, B.lgssm_model()))
    key = genjax.random.key(1, "philox")
    with pytest.raises(ValueError, match="ancestors"):
        ops.backmove_run(plan, key, [torch.zeros((3, 8))], torch.zeros((3, 8)), torch.zeros((3, 8), dtype=torch.int64), None, 4, 2)


# ---- libraries without the header; results without what the sampler reads -----------------------------------------------
def test_oracle_bound_ops_raise_unavailable(oracle_ops):
    alg = BootstrapSMC(LinearGaussianSSM(), W.lgssm_data(6), 512, record_history=True)
    with use_ops(oracle_ops):
        res = alg.run(genjax.random.key(1, "philox"))
        with pytest.raises(abi.BackmoveUnavailable, match="gjx_backmove") as e:
            alg.backward_simulate(res, genjax.random.key(2, "philox"), n_paths=8, n_moves=2)
        with pytest.raises(abi.BacksimUnavailable):  # n_moves=None is the exact method, unchanged
            alg.backward_simulate(res, genjax.random.key(2, "philox"), n_paths=8)
    assert isinstance(e.value, GjxError) and isinstance(e.value, abi.HeaderUnavailable) and e.value.code == -2
    with pytest.raises(abi.BackmoveUnavailable, match="gjx_backmove_run"):
        oracle_ops.backmove_run(None, genjax.random.key(2), [res.history], res.log_weight_history, res.ancestors, None, 8, 2)
    with pytest.raises(abi.BackmoveUnavailable, match="gjx_backmove_workspace_bytes"):
        oracle_ops.lib.call("gjx_backmove_workspace_bytes", 3, 8, 8)
    with pytest.raises(abi.BackmoveUnavailable):
        oracle_ops.lib.require("backmove", "gjx_backmove_run")


def test_a_result_without_ancestors_or_history_or_a_bad_n_moves_raises(oracle_ops):
    y = W.lgssm_data(4)
    with use_ops(oracle_ops):
        plain = BootstrapSMC(LinearGaussianSSM(), y, 256)
        res = plain.run(genjax.random.key(1))
        with pytest.raises(ValueError, match="record_history"):
            plain.backward_simulate(res, genjax.random.key(2), n_paths=4, n_moves=2)
        hist = BootstrapSMC(LinearGaussianSSM(), y, 256, record_history=True)
        res = hist.run(genjax.random.key(1))
        for bad in (-1, 257, 2.0, True, "2"):
            with pytest.raises(ValueError, match="n_moves"):
                hist.backward_simulate(res, genjax.random.key(2), n_paths=4, n_moves=bad)
        res.ancestors = None
        with pytest.raises(ValueError, match="ancestor"):
            hist.backward_simulate(res, genjax.random.key(2), n_paths=4, n_moves=2)
    assert GuidedSMC.backward_simulate is BootstrapSMC.backward_simulate  # inherited


# ---- offline compilation -------------------------------------------------------------------------------------------------
def test_generated_move_kernels_compile_offline(ops, oracle_ops):
    trans, emit = B.hmm_tables(8)
    tables = dict(lgssm=_table(ops, B.lgssm_model()), two=_table(ops, B.two_component_model()), gamma=_table(ops, B.gamma_model()),
                  increment=_table(ops, B.increment_model(), [("u",), ("d",)]),
                  # (compile-only: the categorical tables are never read, host tensors will do)
                  hmm=_table(oracle_ops, B.hmm_model(trans, emit), [("x",)]))
    for name, t in tables.items():
        plan = ops.backsim_plan_create(t)
        for impl in (0, 1):
            src = plan.move_source(impl)
            assert "gjx_backmove_step_kernel" in src and "gjx_backmove_last_kernel" in src and "trans_lp(" in src
            assert "gjx_backsim_step_kernel" not in src and "gjx_backmove" not in plan.source(impl)  # a module of its own
            # the generator is baked into the source: both entry points instantiate their helpers for it, the other's streams are absent
            entries = src.split('extern "C"')[1:]
            assert src.count("nx_") > 0 and len(entries) == 2 and all(f"<{impl}," in e for e in entries)
            assert f"Stream<{1 - impl}>" not in src
            assert plan.move_compile_check(impl) == 0, (name, impl)
    assert "logpdf_normal_pre(" in ops.backsim_plan_create(tables["lgssm"]).move_source(1)
    assert "logpdf_gamma(" in ops.backsim_plan_create(tables["gamma"]).move_source(1)


def test_generated_move_source_is_the_table_walk_and_two_kernels(ops):
    """The search, the draw, the blocks of moves and the stores are gjx_device.hpp's backmove_* templates.  The two kernels'
    own loops over paths (and the LDS array they hand to backmove_stage) are still generated: moved into a device function
    they compile to other machine code (profiles/fixed_bodies_summary.md), so outside the struct the source holds the two
    entry points and nothing else — one grid-stride loop and one LDS array each, no search loop, no atomic."""
    plan = ops.backsim_plan_create(_table(ops, B.lgssm_model()))
    for impl in (0, 1):
        structs, kernels, rest = source_shape(plan.move_source(impl))
        assert structs == ["GenTrans"] and kernels == ["gjx_backmove_step_kernel", "gjx_backmove_last_kernel"]
        assert "bm_" not in plan.move_source(impl)
        assert rest.startswith("using namespace gjx;\nextern \"C\"") and "__device__" not in rest and "template" not in rest
        assert "while (" not in rest and "atomic" not in rest
        step, last = rest.split('extern "C"')[1:]
        assert step.count("__shared__") == last.count("__shared__") == 1
        assert step.count("for (") == 3 and last.count("for (") == 1  # paths; the next state's D columns; blocks of four moves


def test_philox_lgssm_move_kernel_occupancy(ops, tmp_path):
    plan = ops.backsim_plan_create(_table(ops, B.lgssm_model()))
    metas = kernel_notes(plan.move_source(1), tmp_path, "backmove_lgssm")
    print("PHILOX LGSSM move kernels:", metas)
    assert "gjx_backmove_step_kernel" in metas and "gjx_backmove_last_kernel" in metas
    for meta in metas.values():
        assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0, meta  # no scratch
        assert meta["vgpr_count"] <= 128, meta  # 512 / 128: four resident waves per SIMD — a latency kernel lives on them


# ---- the reference -------------------------------------------------------------------------------------------------------
def test_with_no_moves_the_reference_is_trace_back(oracle_ops):
    y = W.lgssm_data(6)
    alg = BootstrapSMC(LinearGaussianSSM(), y, 1000, record_history=True)
    table = _table(oracle_ops, B.lgssm_model())
    for impl in ("threefry", "philox"):
        with use_ops(oracle_ops):
            res = alg.run(genjax.random.key(3, impl))
        lin, (paths,) = M.backmove_ref(oracle_ops, table, genjax.random.key(4, impl), [res.history], res.log_weight_history, res.ancestors,
                                       None, 300, 0)
        assert torch.equal(lin, M.trace_back(res.ancestors, lin[-1]))
        assert torch.equal(paths, torch.gather(res.history, 1, lin.long()))
        moved, _ = M.backmove_ref(oracle_ops, table, genjax.random.key(4, impl), [res.history], res.log_weight_history, res.ancestors,
                                  None, 300, 3)
        assert torch.equal(moved[-1], lin[-1]) and not torch.equal(moved[:-1], lin[:-1])  # same leaves; the moves do move


N_REF, M_REF, R_REF, T_REF, K_REF = 8192, 512, 16, 8, 4


def test_the_reference_is_a_smoother_lgssm(oracle_ops):
    """The bounds are those of test_backsim_cpu.py::test_the_reference_is_a_smoother_lgssm."""
    y = W.lgssm_data(T_REF)
    alg = BootstrapSMC(LinearGaussianSSM(), y, N_REF, record_history=True)
    table = _table(oracle_ops, B.lgssm_model())
    means, variances = [], []
    for r in range(R_REF):  # a run = a filter of its own and a backward pass over it: the spread holds both errors
        with use_ops(oracle_ops):
            res = alg.run(genjax.random.key(500 + r, "philox"))
        _, (paths,) = M.backmove_ref(oracle_ops, table, genjax.random.key(100 + r, "philox"), [res.history], res.log_weight_history,
                                     res.ancestors, None, M_REF, K_REF)
        p = paths.double().numpy()
        means.append(p.mean(1))
        variances.append(p.var(1))
    means, variances = np.asarray(means), np.asarray(variances)
    ms, ps = B.lgssm_rts(y)
    se = means.std(0, ddof=1) / np.sqrt(R_REF)
    z = (means.mean(0) - ms) / se
    ratio = variances.mean(0) / ps
    print("LGSSM smoothing mean z-scores:", np.round(z, 2), "variance ratios:", np.round(ratio, 3))
    assert np.all(np.abs(z) <= 4.0), z
    assert np.all(np.abs(ratio - 1.0) <= 0.10), ratio
