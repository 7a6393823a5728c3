"""The optional headers next to gjx.h (gjx_paths.h, gjx_guided.h, gjx_backsim.h): libgjx_hip.so exports them, the ctypes
tables cover them, gjx.h and the oracle library know nothing of them.  And include/gjx_paths.h itself: host-side validation
refuses bad calls before any launch (no GPU needed for any of this)."""

import ctypes as C
import os

import pytest
import torch

from genjax._amd import abi
from genjax._amd.abi import GjxError
from genjax._amd.ops import Ops
from offline import ROOT, header_symbols, ops  # noqa: F401


@pytest.fixture(scope="module")
def hip_lib(ops):
    return ops.lib


# per optional header: the symbols it declares, and the constants the binding restates as the header's text has them
HEADERS = dict(
    paths=({"gjx_paths_version", "gjx_paths_workspace_bytes", "gjx_paths_trace"},
           ["GJX_PATHS_MAX_COLS (GJX_SMC_MAX_STATE + 1)", f"GJX_PATHS_LEAVES_ORDERED {abi.PATHS_LEAVES_ORDERED}u"]),
    guided=({"gjx_guided_version", "gjx_smc_plan_create_guided", "gjx_smc_plan_source"},
            [f"GJX_SITE_PROPOSED {abi.SITE_PROPOSED}", f"GJX_SITE_GUIDED {abi.SITE_GUIDED}"]),
    backsim=({"gjx_backsim_version", "gjx_backsim_plan_create", "gjx_backsim_plan_destroy", "gjx_backsim_plan_source",
              "gjx_backsim_plan_compile_check", "gjx_backsim_workspace_bytes", "gjx_backsim_run"},
             [f"GJX_ARG_NEXT {abi.ARG_NEXT}"]))


@pytest.mark.parametrize("key", list(abi.OPTIONAL_HEADERS))
def test_optional_header_is_exported_by_the_hip_library_only(hip_lib, oracle_ops, key):
    h = abi.OPTIONAL_HEADERS[key]
    symbols, constants = HEADERS[key]
    syms = header_symbols(h.header)
    assert syms == set(h.prototypes) == symbols and h.version_fn in syms
    assert h.prototypes is getattr(abi, f"{key.upper()}_PROTOTYPES") and h.version == getattr(abi, f"{key.upper()}_ABI_VERSION")
    assert not (syms & header_symbols("gjx.h")) and not (syms & set(abi.PROTOTYPES))
    for other in abi.OPTIONAL_HEADERS.values():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    for name in syms:
        assert hasattr(hip_lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert getattr(hip_lib, f"has_{key}") and not getattr(oracle_ops.lib, f"has_{key}")
    major, minor = C.c_int(-1), C.c_int(-1)
    hip_lib.call(h.version_fn, C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == h.version
    hdr = open(os.path.join(ROOT, "include", h.header)).read()
    up = key.upper()
    assert f"GJX_{up}_VERSION_MAJOR {major.value}" in hdr and f"GJX_{up}_VERSION_MINOR {minor.value}" in hdr
    for text in constants:
        assert text in hdr, text
    assert abi.PATHS_MAX_COLS == abi.SMC_MAX_STATE + 1
    if key == "backsim":
        assert hip_lib.call("gjx_backsim_workspace_bytes", 100, 1024) == 100 * 1024 * 8


def test_oracle_loads_without_them_and_says_so(oracle_ops):
    assert not oracle_ops.lib.has_paths
    for name in abi.PATHS_PROTOTYPES:
        assert not hasattr(oracle_ops.lib._dll, name)
    anc = torch.zeros((3, 8), dtype=torch.int32)
    with pytest.raises(GjxError, match="gjx_paths_trace") as e:
        oracle_ops.paths_trace(anc, [torch.zeros((3, 8))])
    assert isinstance(e.value, abi.PathsUnavailable) and e.value.code == -2
    with pytest.raises(abi.PathsUnavailable, match="gjx_paths_workspace_bytes"):
        oracle_ops.lib.call("gjx_paths_workspace_bytes", 3, 8, 1)


def test_workspace_bytes(hip_lib):
    wb = lambda T, m, c: hip_lib.call("gjx_paths_workspace_bytes", T, m, c)
    assert wb(100, 1_000_000, 1) == 100 * 3 * 977 * 8 and wb(1, 1, 0) == 8
    assert wb(0, 10, 1) == 0 and wb(3, 0, 1) == 0 and wb(3, 1 << 31, 1) == 0 and wb(3, 10, 6) == 0


def _io(T=3, n=8, m=8, n_cols=1):
    """A VALID call description over dummy non-null addresses (validation happens on the host, before any launch; the
    tests below break one thing at a time and never reach a launch)."""
    io = abi.PathsIO()
    io.n_steps, io.n_cols, io.n, io.m = T, n_cols, n, m
    io.ancestors, io.anc_stride = 0x1000, n
    for c in range(n_cols):
        io.cols[c], io.col_stride[c], io.col_is_f32[c] = 0x2000, n, 1
        io.paths_out[c], io.paths_stride[c] = 0x3000, m
    io.lineage_out, io.lineage_stride = 0x4000, m
    io.ticket = 0x5000
    return io


def _rc(hip_lib, io, ws=0x8000, nb=1 << 20):
    return hip_lib._gjx_paths_trace(C.byref(io) if io is not None else None, C.c_void_p(ws), nb, None)


def test_invalid_calls_are_refused_before_any_launch(hip_lib):
    INVALID, WORKSPACE = -1, -3
    assert _rc(hip_lib, None) == INVALID
    bad = []
    for field, value in (("n_steps", 0), ("n", 0), ("m", 0), ("n", 1 << 31), ("m", 1 << 31), ("n_cols", -1), ("n_cols", 6),
                         ("ancestors", None), ("anc_stride", 7), ("lineage_stride", 7), ("m", 9)):  # (m != n without leaves)
        io = _io()
        setattr(io, field, value)
        bad.append((field, value, _rc(hip_lib, io)))
    assert all(rc == INVALID for _, _, rc in bad), bad
    io = _io(); io.cols[0] = None
    assert _rc(hip_lib, io) == INVALID
    io = _io(); io.col_stride[0] = 7
    assert _rc(hip_lib, io) == INVALID
    io = _io(); io.paths_stride[0] = 7
    assert _rc(hip_lib, io) == INVALID
    io = _io(); io.lineage_out = None; io.paths_out[0] = None  # no output at all
    assert _rc(hip_lib, io) == INVALID
    io = _io(m=4); io.leaves = 0x6000; io.lineage_stride = 3
    assert _rc(hip_lib, io) == INVALID
    # statistics: the ordered flag, the ticket, the workspace
    io = _io(); io.unique_out = 0x7000
    assert _rc(hip_lib, io) == INVALID  # unique_out without GJX_PATHS_LEAVES_ORDERED
    io.flags = abi.PATHS_LEAVES_ORDERED; io.ticket = None
    assert _rc(hip_lib, io) == INVALID
    io.ticket = 0x5000
    assert _rc(hip_lib, io, ws=0) == WORKSPACE
    need = hip_lib.call("gjx_paths_workspace_bytes", 3, 8, 1)
    assert _rc(hip_lib, io, nb=need - 1) == WORKSPACE
    assert _rc(hip_lib, io, ws=0x8004) == INVALID  # not 8-byte aligned
    io = _io(); io.sum_out = 0x7000
    assert _rc(hip_lib, io, nb=need - 1) == WORKSPACE


def test_ops_refuses_bad_tensors_without_a_gpu(hip_lib):
    ops = Ops(hip_lib)
    with pytest.raises(ValueError, match="ancestors"):
        ops.paths_trace(torch.zeros((3, 8), dtype=torch.int64), [])
    with pytest.raises(ValueError, match="ancestors"):
        ops.paths_trace(torch.zeros((3, 8), dtype=torch.int32), [])  # a CPU tensor for the HIP library
