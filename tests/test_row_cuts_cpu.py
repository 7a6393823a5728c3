"""The row-loop cuts of the quad importance kernel, checked without a GPU: the "full outputs" source variant
(GJX_SOURCE_FULL_OUTPUTS: a launch that passes every output asks nothing about them), the exact zero-add cuts of the shared
site emission (gjx_plan_jit.hpp zero_loc_unit / identity_ref / first contribution), the wave maximum on ordered integer keys
and rowfix's two trims (gjx_device.hpp).

tools/check_row_cuts.cpp holds the sweeps behind the "same bits" claims and must exit 0.  The flagship source of the 10-latent
Gaussian model, with and without the flag, compiled for gfx950 by the library's own helper under the shipped options, must
keep its registers and its arithmetic; its row loop, priced by tools/price_kernel.py, must cost at most 5060 cycles with the
flag (a hand edit of the generated source reached 5019.1) and at most 5130 without (the parent's: 5242.8).  The generator
applies each zero-add rule only where its conditions hold."""

import os
import subprocess

import pytest

from genjax._amd import abi, workloads as W
from offline import ROOT, importance_source, ops  # noqa: F401
from test_importance_issue_cost import KERNEL, SHIPPED, WT_STORES, _compile, _notes, _pricer

FULL_OUTPUTS = 0x400  # include/gjx.h GJX_SOURCE_FULL_OUTPUTS
PRICED_FULL, PRICED_GUARDED = 5060.0, 5130.0
GUARDS = ("if (score)", "if (logw)", "if (row_e)")


def test_the_sweeps_find_no_mismatch(tmp_path):
    exe = str(tmp_path / "check_row_cuts")
    flags = ["-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off"]
    if " fma " in open("/proc/cpuinfo").read():  # (without it fmaf is a library call: the same results, several times slower)
        flags.append("-mfma")
    subprocess.run(["g++", *flags, "-o", exe, os.path.join(ROOT, "tools", "check_row_cuts.cpp")], check=True, timeout=300)
    env = dict(os.environ, OMP_NUM_THREADS=str(min(16, os.cpu_count() or 1)))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    assert "x 2^24 angle words x 2 outputs = 3422552064 cases, 0 mismatches" in r.stdout
    assert "R rowfix, every d of [-86, 1]: 2183921666 floats, 0 mismatches" in r.stdout
    assert "M ordered maximum: " in r.stdout and "c first accumulation: 67108864 densities, 0 mismatches" in r.stdout
    assert "ok: 0 mismatches in all" in r.stdout


@pytest.fixture(scope="module")
def built(ops, tmp_path_factory):
    os.environ.pop("GJX_JIT_FORM", None)
    tmp = tmp_path_factory.mktemp("row_cuts")
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = {"guarded": importance_source(ops, plan, 1), "full": importance_source(ops, plan, 1 | FULL_OUTPUTS)}
    return plan, src, {k: _compile(v, tmp, k, SHIPPED) for k, v in src.items()}


@pytest.mark.parametrize("variant", ["guarded", "full"])
def test_both_variants_keep_registers_and_arithmetic(built, variant):
    _, src, co = built
    meta = _notes(co[variant])
    print(variant, meta)
    assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0 and meta["vgpr_count"] <= 61, meta
    r = _pricer().price(co[variant], KERNEL)
    print(variant, "row loop:", r["counts"], "priced cycles", r["priced_cycles"])
    assert r["vector_instructions"] > 1000, r  # (the row loop was found)
    assert r["counts"]["multiply"] == 168 and r["counts"]["transcendental"] == 20, r["counts"]
    assert src[variant].count("bm_pair(") == 20 and src[variant].count("logpdf_normal_pre(") == 80
    assert r["priced_cycles"] <= (PRICED_FULL if variant == "full" else PRICED_GUARDED), r["priced_cycles"]


def test_the_flag_removes_the_questions_and_nothing_else(ops, built):
    plan, src, _ = built
    assert all(g in src["guarded"] for g in GUARDS) and "if (max_partials || row_e)" in src["guarded"]
    assert not any(g in src["full"] for g in GUARDS) and "max_partials ||" not in src["full"] and "max_partials &&" not in src["full"]
    # the flags combine; the store kind stays the only other difference
    wt = importance_source(ops, plan, 1 | FULL_OUTPUTS | WT_STORES)
    assert wt == src["full"].replace("wt_one_pass = false", "wt_one_pass = true") and wt != src["full"]
    # the same sites either way: the questions are the whole difference
    strip = lambda s: s.replace("if (score) ", "").replace("if (logw) ", "").replace("if (row_e) ", "").replace(  # noqa: E731
        "if (max_partials || row_e) ", "").replace("max_partials && ", "")
    assert strip(src["guarded"]) == src["full"]
    for flags in (FULL_OUTPUTS, FULL_OUTPUTS | WT_STORES):
        ops.lib.call("gjx_plan_compile_check", plan.handle, 1 | flags)
    # the pair and one-particle forms ignore the flag
    for form in ("pair", "one"):
        os.environ["GJX_JIT_FORM"] = form
        try:
            assert importance_source(ops, plan, 1 | FULL_OUTPUTS) == importance_source(ops, plan, 1), form
        finally:
            del os.environ["GJX_JIT_FORM"]


def test_flagship_emits_every_cut(built):
    _, src, _ = built
    for s in src.values():
        assert s.count(", PlusZero());") == 20  # ten normal(0, 1) latents, two pairs per lane
        assert s.count("first_acc(") == 8  # the four weights and the four scores of a lane, once each
        assert "const float a0_1A = vf0A;" in s  # the observed site's location: the latent's value itself
        assert "wave_max_ordered(" in s and "wave_max(" not in s


def _c(v):
    return abi.Arg(abi.ARG_CONST, 0, 0.0, v, None)


def _site(dist, a0, a1, out_col=-1, obs=None):
    s = abi.Site()
    s.dist, s.observed, s.out_col = dist, 0 if obs is None else 1, out_col
    s.arg[0], s.arg[1] = a0, a1
    if obs is not None:
        s.obs = obs
    return s


def _ref(site, scale=1.0, offset=0.0):
    return abi.Arg(abi.ARG_SITE, site, scale, offset, None)


def _source(ops, sites):
    os.environ.pop("GJX_JIT_FORM", None)
    return importance_source(ops, ops.plan_create(sites), 1)


def test_zero_location_rule_fires_only_on_plus_zero_and_unit_scale(ops):
    obs = lambda loc: _site(abi.DIST_NORMAL, loc, _c(0.5), obs=_c(0.7))  # noqa: E731
    # the rule's own case
    s = _source(ops, [_site(abi.DIST_NORMAL, _c(0.0), _c(1.0), 0), obs(_ref(0))])
    assert s.count(", PlusZero());") == 2 and "const float a0_1A = vf0A;" in s
    # location -0.0f: the add of -0 is the identity, the two-operation form stays
    s = _source(ops, [_site(abi.DIST_NORMAL, _c(-0.0), _c(1.0), 0), obs(_ref(0))])
    assert "PlusZero" not in s and "const float vf0A = a0_0A + t0A;" in s and "const float a0_1A = vf0A;" not in s
    # location 0 with scale 2
    s = _source(ops, [_site(abi.DIST_NORMAL, _c(0.0), _c(2.0), 0), obs(_ref(0))])
    assert "PlusZero" not in s and "const float vf0A = a0_0A + t0A;" in s and "const float a0_1A = vf0A;" not in s
    # a run-time location: site 1 is centred on site 0 (which the rule does take)
    s = _source(ops, [_site(abi.DIST_NORMAL, _c(0.0), _c(1.0), 0), _site(abi.DIST_NORMAL, _ref(0), _c(1.0), 1), obs(_ref(1))])
    assert s.count(", PlusZero());") == 2 and "const float vf1A = a0_1A + t1A;" in s
    assert "const float a0_1A = vf0A;" in s and "const float a0_2A = vf1A;" not in s  # (site 1's value may be -0)


def test_identity_reference_needs_unit_scale_and_plus_zero_offset(ops):
    z = lambda: _site(abi.DIST_NORMAL, _c(0.0), _c(1.0), 0)  # noqa: E731
    for arg in (_ref(0, 2.0, 0.0), _ref(0, 1.0, -0.0), _ref(0, 1.0, 0.25)):
        s = _source(ops, [z(), _site(abi.DIST_NORMAL, arg, _c(0.5), obs=_c(0.7))])
        assert s.count(", PlusZero());") == 2 and "const float a0_1A = vf0A;" not in s
        assert "* vf0A) + " in s


def test_first_contribution_rule_needs_a_literal_power_of_two_normal(ops):
    # a Gamma site first: its log-density is added to the +0 the scores start with; the weights' first contribution (the
    # observed sigma = 0.5 Normal) still initialises them
    s = _source(ops, [_site(abi.DIST_GAMMA, _c(2.0), _c(2.0), 0), _site(abi.DIST_NORMAL, _c(0.0), _c(1.0), 1),
                      _site(abi.DIST_NORMAL, _ref(1), _c(0.5), obs=_c(0.7))])
    assert "scA = scA + lp; }" in s and "scA = first_acc(" not in s and "wA = first_acc(lp2A);" in s
    # a Normal whose scale is read at run time (from the Gamma site), observed, as the weights' first contribution
    s = _source(ops, [_site(abi.DIST_GAMMA, _c(2.0), _c(2.0), 0), _site(abi.DIST_NORMAL, _c(0.5), _ref(0, 1.0, 0.1), obs=_c(0.7)),
                      _site(abi.DIST_NORMAL, _c(0.25), _c(0.5), obs=_c(0.1))])
    assert "first_acc(" not in s and "wA = wA + lp1A;" in s and "wA = wA + lp2A;" in s
    # sigma = 0.3 (1 / 0.3 is no power of two: not a NormalExactCuts density) first, then a sigma = 1 site
    s = _source(ops, [_site(abi.DIST_NORMAL, _c(0.25), _c(0.3), 0), _site(abi.DIST_NORMAL, _c(0.0), _c(1.0), 1),
                      _site(abi.DIST_NORMAL, _ref(1), _c(0.5), obs=_c(0.7))])
    assert "scA = first_acc(" not in s and "wA = first_acc(lp2A);" in s


def test_escapes_compile_to_the_same_registers(built, tmp_path):
    """Each group's -D escape (what GJX_JIT_DEFINE=<name> builds) compiles, spills nothing and prices no lower than the cut form."""
    _, src, co = built
    pk = _pricer()
    cut = pk.price(co["full"], KERNEL)["priced_cycles"]
    for name in ("GJX_ZERO_LOC_PLAIN", "GJX_FIRST_ACC_PLAIN", "GJX_WAVE_MAX_SELECT", "GJX_ROWFIX_PLAIN"):
        c = _compile(src["full"], tmp_path, name.lower(), SHIPPED + ["-D" + name])
        meta, priced = _notes(c), pk.price(c, KERNEL)["priced_cycles"]
        print(name, meta, priced)
        assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0 and meta["vgpr_count"] <= 64, (name, meta)
        assert priced >= cut, (name, priced, cut)
