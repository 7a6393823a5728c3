"""Occupancy of the flagship importance kernel, checked without a GPU: the default (quad, PHILOX) kernel generated for
the 10-latent Gaussian model is compiled for gfx950 by the library's own helper and its code object's notes are read.

A SIMD's 512 VGPRs are shared in granules of 8, so an allocation of <= 96 registers is five waves per SIMD, <= 80 six and
<= 72 seven.  The kernel used to allocate 132 (three waves): the fused fold tail was inlined into it (22 registers on
launches that never enter it), twelve 64-bit store addresses were hoisted out of the row loop, and every site's
log-density was computed at the end of the row, which kept all sampled values alive until then."""

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from genjax._amd import workloads as W
from genjax._amd.abi import GjxLib
from genjax._amd.ops import Ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "genjax-chi_amd", "lib")
HIP_LIB = os.path.join(LIB_DIR, "libgjx_hip.so")
JITC = os.path.join(LIB_DIR, "gjx_jitc")
DEVICE_HDR = os.path.join(ROOT, "genjax-chi_amd", "csrc", "gjx_device.hpp")
# gjx_plan_jit.hpp compile_options()
OPTIONS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"]
FUSED_TAIL = 0x100  # include/gjx.h GJX_SOURCE_FUSED_TAIL


def _readelf():
    for cand in ("/opt/rocm/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-readelf"):
        if os.path.exists(cand):
            return cand
    return shutil.which("llvm-readelf")


@pytest.fixture(scope="module")
def ops():
    if not os.path.exists(HIP_LIB) or not os.path.exists(JITC):
        import __graft_entry__ as g

        g.build()
    return Ops(GjxLib(HIP_LIB, "cuda"))  # no compute calls below: plans are host objects


def source_of(ops, plan, impl):
    need = C.c_size_t()
    ops.lib.call("gjx_plan_specialized_source", plan.handle, impl, None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value)
    ops.lib.call("gjx_plan_specialized_source", plan.handle, impl, buf, need.value, None)
    return buf.value.decode()


def kernel_notes(src, tmp_path, name):
    """Compile `src` with the helper the library itself uses; -> the kernel's metadata fields as a dict of ints."""
    readelf = _readelf()
    if readelf is None:
        pytest.skip("llvm-readelf is not installed")
    fsrc, fout, flog = (str(tmp_path / f"{name}.{ext}") for ext in ("hip", "co", "log"))
    with open(fsrc, "w") as f:
        f.write(src)
    r = subprocess.run([JITC, fsrc, DEVICE_HDR, fout, flog, *OPTIONS], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, open(flog).read() if os.path.exists(flog) else r.stderr)
    notes = subprocess.run([readelf, "--notes", fout], capture_output=True, text=True, timeout=60).stdout
    assert "gjx_plan_kernel_philox" in notes, notes[:2000]
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|agpr_count|private_segment_fixed_size|sgpr_count):\s+(\d+)", notes)}


def test_default_quad_kernel_occupancy(ops, tmp_path, monkeypatch):
    monkeypatch.delenv("GJX_JIT_FORM", raising=False)
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = source_of(ops, plan, 1)
    assert "__launch_bounds__(64" in src and "make_uint4(" in src  # the quad form
    assert "lse_tail(" not in src, "the default kernel must not carry the fused fold"
    meta = kernel_notes(src, tmp_path, "quad")
    print("default quad kernel:", meta)
    # the floor the issue sets: five waves per SIMD, within the scratch tolerance plan_compiled applies
    assert meta["vgpr_count"] <= 96 and meta["private_segment_fixed_size"] <= 32, meta
    # the target: six waves or more (<= 80 VGPRs) without scratch; reached: 68 registers = seven waves
    assert meta["vgpr_count"] <= 80 and meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0, meta
    assert meta["vgpr_count"] <= 72, meta


def test_fused_tail_variant_still_compiles(ops, tmp_path, monkeypatch):
    monkeypatch.delenv("GJX_JIT_FORM", raising=False)
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = source_of(ops, plan, 1 | FUSED_TAIL)
    assert src.count("lse_tail(") == 1 and "tail.tickets != nullptr" in src
    meta = kernel_notes(src, tmp_path, "quad_tail")
    print("fused-tail quad kernel:", meta)
    assert meta["private_segment_fixed_size"] <= 32, meta
    # ... and every form of it, through the library's own check (one particle per lane, pairs, quads; both RNG schemes)
    for impl in (0, 1):
        ops.lib.call("gjx_plan_compile_check", plan.handle, impl | FUSED_TAIL)


def test_same_draws_and_operations(ops, monkeypatch):
    """The diet moves WHERE things are computed, not what: the same cipher blocks, transforms and log-densities."""
    monkeypatch.delenv("GJX_JIT_FORM", raising=False)
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    for impl in (1, 1 | FUSED_TAIL):
        src = source_of(ops, plan, impl)
        assert src.count("bm_pair(") == 20 and src.count("logpdf_normal_pre(") == 80 and src.count("kTagPair") == 10
        assert src.count("bm_stage();") == 1 and src.index("bm_stage();") < src.index("for (uint64_t g0")
        assert "__syncthreads" not in src.split("void gjx_plan_kernel_philox")[1]
