"""The bit-exact algebraic cuts of the sampler and the Normal log-density (gjx_device.hpp bm_pair, sqrt_pos and the fused
overload of logpdf_normal_pre), checked without a GPU.

tools/check_exact_cuts.cpp holds the sweeps behind the "same bits" claims and must exit 0.  The default flagship kernel
(quad, PHILOX, plain stores) of the 10-latent Gaussian model, compiled for gfx950 by the library's own helper with the
shipped options, must keep its registers and its arithmetic and hold at least 100 fewer simple vector instructions in its
row loop than before the cuts (1514; priced 5592.4 cycles by tools/price_kernel.py).  The generator picks the fused
log-density only where both of its conditions hold: the reciprocal scale a literal power of two, the log-normaliser a
literal."""

import os
import subprocess

import pytest

from genjax._amd import abi, workloads as W
from offline import FUSED_TAIL, ROOT, importance_source, ops  # noqa: F401
from test_importance_issue_cost import KERNEL, SHIPPED, WT_STORES, _compile, _notes, _pricer

PARENT_SIMPLE = 1514
PRICED_CYCLES = 5242.8  # the row loop with the four cuts (below the issue's bound of 5350; the parent's: 5592.4)
VARIANTS = {"default": 0, "one_pass": WT_STORES, "fused_tail": FUSED_TAIL, "one_pass_fused_tail": WT_STORES | FUSED_TAIL}
FUSED = ", NormalExactCuts())"


def test_the_sweeps_find_no_mismatch(tmp_path):
    exe = str(tmp_path / "check_exact_cuts")
    flags = ["-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off"]
    if " fma " in open("/proc/cpuinfo").read():  # (without it fmaf is a library call: the same results, several times slower)
        flags.append("-mfma")
    subprocess.run(["g++", *flags, "-o", exe, os.path.join(ROOT, "tools", "check_exact_cuts.cpp")], check=True, timeout=300)
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, os.cpu_count() or 1)))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    assert "A radius word: 4294967296 words, 0 mismatches" in r.stdout
    assert r.stdout.count("240992364 floats, 0 mismatches") == 5


@pytest.fixture(scope="module")
def built(ops, tmp_path_factory):
    os.environ.pop("GJX_JIT_FORM", None)
    tmp = tmp_path_factory.mktemp("exact_cuts")
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = importance_source(ops, plan, 1)
    return plan, src, _compile(src, tmp, "default", SHIPPED)


def test_default_kernel_keeps_registers_and_arithmetic_and_sheds_simple_instructions(built):
    _, _, co = built
    meta = _notes(co)
    print("default quad kernel:", meta)
    assert meta["vgpr_count"] <= 64 and meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0, meta
    r = _pricer().price(co, KERNEL)
    print("row loop:", r["counts"], "priced cycles", r["priced_cycles"])
    assert r["vector_instructions"] > 1000, r  # (the row loop was found)
    assert r["counts"]["multiply"] == 168 and r["counts"]["transcendental"] == 20 and r["counts"]["bitop3"] == 186, r["counts"]
    assert r["counts"]["simple"] <= PARENT_SIMPLE - 100, r["counts"]
    assert r["priced_cycles"] <= PRICED_CYCLES < 5350, r["priced_cycles"]


def test_every_variant_and_form_compiles(ops, built):
    """The four quad variants, and with each the pair and one-particle forms (the library's check builds every form)."""
    plan, _, _ = built
    for flags in VARIANTS.values():
        ops.lib.call("gjx_plan_compile_check", plan.handle, 1 | flags)


def test_flagship_plan_emits_the_fused_forms(ops, built):
    plan, src, _ = built
    # sigma = 1 latents (rs = 2^0) and sigma = 0.5 observations (rs = 2^1): every one of the 80 log-densities
    assert src.count("logpdf_normal_pre(") == 80 and src.count(FUSED) == 80
    for flags in VARIANTS.values():
        assert importance_source(ops, plan, 1 | flags).count(FUSED) == 80
    for form, per_lane in (("pair", 2), ("one", 1)):
        os.environ["GJX_JIT_FORM"] = form
        try:
            assert importance_source(ops, plan, 1).count(FUSED) == 20 * per_lane, form
        finally:
            del os.environ["GJX_JIT_FORM"]
    assert importance_source(ops, plan, 0).count(FUSED) == 20  # (THREEFRY: one particle per lane)


def _sites(scale_arg):
    """z ~ Normal(0.25, 1); x ~ Normal(z, scale); y ~ Normal(x, scale) observed."""
    c = lambda v: abi.Arg(abi.ARG_CONST, 0, 0.0, v, None)  # noqa: E731
    z = abi.Site(); z.dist, z.observed, z.out_col = abi.DIST_NORMAL, 0, 0
    z.arg[0], z.arg[1] = c(0.25), c(1.0)
    x = abi.Site(); x.dist, x.observed, x.out_col = abi.DIST_NORMAL, 0, 1
    x.arg[0], x.arg[1] = abi.Arg(abi.ARG_SITE, 0, 1.0, 0.0, None), scale_arg
    y = abi.Site(); y.dist, y.observed, y.out_col = abi.DIST_NORMAL, 1, -1
    y.arg[0], y.arg[1] = abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None), scale_arg
    y.obs = c(0.7)
    return [z, x, y]


def test_other_scales_emit_the_unfused_forms(ops):
    os.environ.pop("GJX_JIT_FORM", None)
    # sigma = 0.3: 1 / 0.3 is no power of two — the two sites of that scale keep the three-operation form (the sigma = 1 site fuses)
    lit = importance_source(ops, ops.plan_create(_sites(abi.Arg(abi.ARG_CONST, 0, 0.0, 0.3, None))), 1)
    assert lit.count("logpdf_normal_pre(") == 12 and lit.count(FUSED) == 4
    for line in lit.splitlines():
        if "logpdf_normal_pre(vf1" in line or "logpdf_normal_pre(vf2" in line:
            assert FUSED not in line, line
    # a scale read from another site at run time: nothing is hoisted, logpdf_normal computes rs and lognorm per particle
    run = importance_source(ops, ops.plan_create(_sites(abi.Arg(abi.ARG_SITE, 0, 0.0, 0.5, None))), 1)
    assert run.count("logpdf_normal(") == 8 and run.count(FUSED) == 4
    # sigma = 0.3 everywhere: no fused form at all
    sites = _sites(abi.Arg(abi.ARG_CONST, 0, 0.0, 0.3, None))
    sites[0].arg[1] = abi.Arg(abi.ARG_CONST, 0, 0.0, 0.3, None)
    assert "NormalExactCuts" not in importance_source(ops, ops.plan_create(sites), 1)
    # sigma = 2 (rs = 2^-1, k < 0) stays unfused too
    sites = _sites(abi.Arg(abi.ARG_CONST, 0, 0.0, 2.0, None))
    sites[0].arg[1] = abi.Arg(abi.ARG_CONST, 0, 0.0, 2.0, None)
    assert "NormalExactCuts" not in importance_source(ops, ops.plan_create(sites), 1)
