"""The entry of the flagship importance kernel, checked without a GPU.

The generated kernels of the 10-latent Gaussian model take their pass and row from the block indices of a two-dimensional
grid and stage the Box-Muller tables for a workgroup size that is a constant of the source: no division by the rows of a
pass, no read of the block size.  Compiled for gfx950 by the library's own helper with the shipped options
(gjx_plan_jit.hpp compile_options), the default (quad, PHILOX, plain stores) kernel must still fit eight waves per SIMD,
its row loop must keep the arithmetic it had (multiplies, transcendentals, three-input XORs of the cipher), price no
higher in issue cycles (tools/price_kernel.py) and hold fewer scalar instructions than before the change."""

import pytest

from genjax._amd import workloads as W
from offline import FUSED_TAIL, importance_source, ops  # noqa: F401
from test_importance_issue_cost import KERNEL, SHIPPED, WT_STORES, _compile, _notes, _pricer

# the row loop of the default kernel before the change (profiles/philox_xor3_summary.md; reproduced with the shipped options)
PARENT_PRICED_CYCLES = 5599.4
PARENT_SCALAR = 326
VARIANTS = {"default": 0, "one_pass": WT_STORES, "fused_tail": FUSED_TAIL, "one_pass_fused_tail": WT_STORES | FUSED_TAIL}


@pytest.fixture(scope="module")
def built(ops, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("entry")
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = {name: importance_source(ops, plan, 1 | flags) for name, flags in VARIANTS.items()}
    co = {name: _compile(s, tmp, name, SHIPPED) for name, s in src.items()}
    return plan, src, co


def test_source_has_no_row_division_and_no_block_size_read(built):
    _, src, _ = built
    for name, s in src.items():
        assert "/ bt.rows_per_pass" not in s, name
        assert "blockDim.x" not in s, name
        assert "blockIdx.y" in s and "#define GJX_BM_BLOCK 64\n" in s and "bm_stage();" in s, name
        # the table loads are issued in front of the argument anchor and committed to LDS behind it, before the row loop
        assert s.index("bm_issue();") < s.index('asm volatile("" :: "s"(n)') < s.index("bm_loads.bm_stage();") < s.index("for (uint64_t g0"), name
        # the parent key of the pass is loaded with the arguments; which key a pass uses keeps its meaning
        assert "bt.parent[pass][0]" in s and "bt.n_pass > 1 ? bk0 : ks.parent.k0" in s, name
    assert "lse_tail(row_e, row_s, (n + 255) / 256, tail, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y)" in src["fused_tail"]


def test_every_variant_and_form_compiles(ops, built):
    """The four quad variants above compiled; the library's own check also builds the pair and one-particle forms."""
    plan, _, co = built
    for name in VARIANTS:
        meta = _notes(co[name])
        print(name, meta)
        assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0, (name, meta)
    for flags in VARIANTS.values():
        ops.lib.call("gjx_plan_compile_check", plan.handle, 1 | flags)


def test_default_kernel_fits_eight_waves(built):
    _, _, co = built
    meta = _notes(co["default"])
    print("default quad kernel:", meta)
    assert meta["vgpr_count"] <= 64, meta
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["agpr_count"] == 0, meta


def test_row_loop_keeps_its_arithmetic_and_sheds_scalar_work(built):
    _, _, co = built
    r = _pricer().price(co["default"], KERNEL)
    print("row loop:", r["counts"], "priced cycles", r["priced_cycles"])
    assert r["vector_instructions"] > 1000, r  # (the row loop was found: it is still a loop in the code object)
    assert r["counts"]["multiply"] == 168 and r["counts"]["transcendental"] == 20 and r["counts"]["bitop3"] == 186, r["counts"]
    assert r["priced_cycles"] <= PARENT_PRICED_CYCLES, r["priced_cycles"]
    assert r["counts"]["scalar"] < PARENT_SCALAR, r["counts"]
