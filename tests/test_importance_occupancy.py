"""Occupancy of the flagship importance kernel, checked without a GPU: the default (quad, PHILOX) kernel generated for
the 10-latent Gaussian model is compiled for gfx950 by the library's own helper and its code object's notes are read.

A SIMD's 512 VGPRs are shared in granules of 8, so an allocation of <= 96 registers is five waves per SIMD, <= 80 six and
<= 72 seven.  The kernel used to allocate 132 (three waves): the fused fold tail was inlined into it (22 registers on
launches that never enter it), twelve 64-bit store addresses were hoisted out of the row loop, and every site's
log-density was computed at the end of the row, which kept all sampled values alive until then."""

from genjax._amd import workloads as W
from offline import FUSED_TAIL, importance_source as source_of, kernel_notes, ops  # noqa: F401


def test_default_quad_kernel_occupancy(ops, tmp_path, monkeypatch):
    monkeypatch.delenv("GJX_JIT_FORM", raising=False)
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = source_of(ops, plan, 1)
    assert "__launch_bounds__(64" in src and "make_uint4(" in src  # the quad form
    assert "lse_tail(" not in src, "the default kernel must not carry the fused fold"
    meta = kernel_notes(src, tmp_path, "quad")["gjx_plan_kernel_philox"]
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
    meta = kernel_notes(src, tmp_path, "quad_tail")["gjx_plan_kernel_philox"]
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
