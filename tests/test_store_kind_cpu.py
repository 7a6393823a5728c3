"""The kind of store of the quad importance kernel (plain, write-through, non-temporal, both hints) as a source variant, checked
without a GPU.

The flagship source of the 10-latent Gaussian model under every kind, compiled for gfx950 by the library's own helper under the
shipped options, must keep the parent's registers (at most 61 VGPRs, nothing in scratch, no AGPRs) and arithmetic (168
multiplies, 20 transcendentals in the row loop), and the row loop of the variant a flagship launch takes (every output known)
must price within 10 cycles of the parent's 5020.6 (tools/price_kernel.py); the guarded source of every kind at most 10 cycles
above the guarded plain one.  The sources differ in their store lines alone.  tools/check_store_kind.cpp prints what
ImportanceVariant::of_launch answers for (1, 2, 32 passes) x (bytes written) x (some outputs, every output, fused tail) x (no
escape, each escape), and every launchable variant's slot."""

import os
import re
import subprocess

import pytest

from genjax._amd import abi
from offline import ROOT, importance_source, ops  # noqa: F401
from test_importance_issue_cost import KERNEL, SHIPPED, _compile, _notes, _pricer
from genjax._amd import workloads as W

FUSED_TAIL, WT_STORES, FULL_OUTPUTS, NT_STORES = 0x100, 0x200, 0x400, 0x800  # include/gjx.h GJX_SOURCE_*
KINDS = {"plain": 0, "wt": WT_STORES, "nt": NT_STORES, "nt_wt": NT_STORES | WT_STORES}  # kind number: bit 0 wt, bit 1 nt
NUMBER = {"plain": 0, "wt": 1, "nt": 2, "nt_wt": 3}
PARENT_PRICE, WITHIN = 5020.6, 10.0
BATCH_KIND = "nt_wt"  # what a launch of several passes takes from 1.5e9 bytes per launch on: profiles/stream_store_summary.md
SMALL, ONE_PASS, BATCH = 12288, 48000000, 1536000000  # the bytes tools/check_store_kind.cpp asks about


@pytest.fixture(scope="module")
def built(ops, tmp_path_factory):
    os.environ.pop("GJX_JIT_FORM", None)
    tmp = tmp_path_factory.mktemp("store_kind")
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = {(k, f): importance_source(ops, plan, 1 | bits | (FULL_OUTPUTS if f else 0)) for k, bits in KINDS.items() for f in (False, True)}
    return plan, src, {key: _compile(s, tmp, f"{key[0]}_{int(key[1])}", SHIPPED) for key, s in src.items()}


@pytest.mark.parametrize("full", [True, False], ids=["every_output", "guarded"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_every_kind_keeps_registers_arithmetic_and_price(built, kind, full):
    _, src, co = built
    meta = _notes(co[(kind, full)])
    pk = _pricer()
    r = pk.price(co[(kind, full)], KERNEL)
    print(kind, "every output" if full else "guarded", meta, r["counts"], "priced cycles", r["priced_cycles"])
    assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0 and meta["vgpr_count"] <= 61, meta
    assert r["vector_instructions"] > 1000, r  # (the row loop was found)
    assert r["counts"]["multiply"] == 168 and r["counts"]["transcendental"] == 20, r["counts"]
    if full:
        assert abs(r["priced_cycles"] - PARENT_PRICE) <= WITHIN, (r["priced_cycles"], PARENT_PRICE)
    else:  # (the parent's own guarded write-through source prices 26 cycles BELOW its plain one: only dearer counts)
        want = pk.price(co[("plain", False)], KERNEL)["priced_cycles"]
        assert r["priced_cycles"] <= want + WITHIN, (r["priced_cycles"], want)


def test_the_library_compiles_every_kind(ops, built):
    plan, _, _ = built
    for bits in KINDS.values():
        for more in (0, FULL_OUTPUTS, FUSED_TAIL):
            ops.lib.call("gjx_plan_compile_check", plan.handle, 1 | bits | more)


def _store_line(line):
    return "store16_at(" in line or "store16_out(" in line or "wt_one_pass =" in line or "nt_stores =" in line


@pytest.mark.parametrize("full", [True, False], ids=["every_output", "guarded"])
def test_sources_differ_in_their_store_lines_alone(built, full):
    _, src, _ = built
    rest = {k: [ln for ln in src[(k, full)].split("\n") if not _store_line(ln)] for k in KINDS}
    stores = {k: [ln for ln in src[(k, full)].split("\n") if _store_line(ln)] for k in KINDS}
    for k in KINDS:
        assert rest[k] == rest["plain"], k
        assert sum("store16_at(" in ln for ln in stores[k]) == 12 and "store16_out(" not in src[(k, full)], k  # ten latents, logw, score
        assert "bt.n_pass <= 1" not in src[(k, full)], "the kind of store must not be a run-time branch"
    assert len({src[(k, full)] for k in KINDS}) == 4
    # the two kinds the parent had keep their text; the non-temporal ones name a second constant in every store
    assert src[("wt", full)] == src[("plain", full)].replace("wt_one_pass = false", "wt_one_pass = true")
    assert "nt_stores" not in src[("plain", full)] + src[("wt", full)]
    for k, wt in (("nt", "false"), ("nt_wt", "true")):
        assert f"const bool wt_one_pass = {wt};" in src[(k, full)] and "const bool nt_stores = true;" in src[(k, full)]
        assert all("wt_one_pass, nt_stores);" in ln for ln in stores[k] if "store16_at(" in ln)


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rule") / "check_store_kind")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "genjax-chi_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "check_store_kind.cpp")],
                   check=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    launches, variants, narrow = {}, [], []
    for ln in out.splitlines():
        nums = [int(x) for x in re.findall(r"-?\d+", ln)]
        if ln.startswith("launch"):
            launches[tuple(nums[:4])] = dict(zip(("particles", "fused", "stores", "full", "slot", "launched"), nums[4:]))
        elif ln.startswith("variant"):
            variants.append(dict(zip(("impl", "particles", "fused", "stores", "full", "slot", "slots"), nums)))
        elif ln.startswith("narrow"):
            narrow.append(dict(zip(("allowed", "pref", "particles", "stores", "full", "slot"), nums)))
    return launches, variants, narrow


def test_of_launch_maps_passes_bytes_and_outputs_to_the_expected_variant(rule):
    launches, _, narrow = rule
    assert len(launches) == 3 * 3 * 3 * 5
    # the measured rule (gjx_plan_jit.hpp ImportanceVariant::stores_of): one pass writes through; several passes take plain stores
    # below the size the batch kind was measured at (1.5e9 bytes per launch), and the batch kind from there on
    expected = {(1, SMALL): "wt", (1, ONE_PASS): "wt", (1, BATCH): "wt", (2, SMALL): "plain", (2, ONE_PASS): "plain", (2, BATCH): BATCH_KIND,
                (32, SMALL): "plain", (32, ONE_PASS): "plain", (32, BATCH): BATCH_KIND}
    for (n_pass, nbytes, outputs, pref), v in launches.items():
        what = (n_pass, nbytes, outputs, pref, v)
        assert v["particles"] == 4 and v["launched"] == 1, what
        assert v["fused"] == int(outputs == 2) and v["full"] == int(outputs == 1), what
        assert v["stores"] == (pref if pref >= 0 else NUMBER[expected[(n_pass, nbytes)]]), what
    for v in narrow:  # one or two particles per lane: one kind of store, whatever is asked
        assert v["particles"] == v["allowed"] and v["stores"] == 0 and v["full"] == 0, v


def test_no_two_launchable_variants_share_a_slot(rule):
    launches, variants, _ = rule
    slots = [v["slot"] for v in variants]
    assert len(variants) == variants[0]["slots"] == 18 and sorted(slots) == list(range(18)), slots
    quads = [v for v in variants if v["particles"] == 4]
    assert len(quads) == 12 and {(v["fused"], v["full"], v["stores"]) for v in quads} == {(f, u, s) for f, u in ((0, 0), (1, 0), (0, 1)) for s in range(4)}
    # what of_launch answers is one of them, in its slot
    by_key = {(v["impl"], v["particles"], v["fused"], v["stores"], v["full"]): v["slot"] for v in variants}
    for v in launches.values():
        assert by_key[(1, 4, v["fused"], v["stores"], v["full"])] == v["slot"]


def _c(v):
    return abi.Arg(abi.ARG_CONST, 0, 0.0, v, None)


def _site(dist, a0, a1, out_col=-1, obs=None):
    s = abi.Site()
    s.dist, s.observed, s.out_col = dist, 0 if obs is None else 1, out_col
    s.arg[0], s.arg[1] = a0, a1
    if obs is not None:
        s.obs = obs
    return s


def test_the_bit_is_ignored_below_four_particles_per_lane(ops):
    """A model of tests/test_row_cuts_cpu.py's "no rule fires" set (location -0.0f): the same text with and without the bit."""
    sites = [_site(abi.DIST_NORMAL, _c(-0.0), _c(1.0), 0), _site(abi.DIST_NORMAL, abi.Arg(abi.ARG_SITE, 0, 1.0, 0.0, None), _c(0.5), obs=_c(0.7))]
    plan = ops.plan_create(sites)
    for form in ("pair", "one"):
        os.environ["GJX_JIT_FORM"] = form
        try:
            for more in (0, WT_STORES, FULL_OUTPUTS, FUSED_TAIL):
                assert importance_source(ops, plan, 1 | more | NT_STORES) == importance_source(ops, plan, 1 | more), (form, more)
            assert importance_source(ops, plan, 0 | NT_STORES) == importance_source(ops, plan, 0), form  # THREEFRY: one particle per lane
        finally:
            del os.environ["GJX_JIT_FORM"]
    assert importance_source(ops, plan, 1 | NT_STORES) != importance_source(ops, plan, 1)  # (four per lane: the bit counts)
