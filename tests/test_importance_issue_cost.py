"""Issue cost of the flagship importance kernel, checked without a GPU.

The default (quad, PHILOX, plain stores) kernel of the 10-latent Gaussian model and its one-pass variant (write-through
stores) are compiled for gfx950 by the library's own helper with the option list the library ships for importance plans
(gjx_plan_jit.hpp compile_options: the four fixed options and -fno-slp-vectorize).  The default kernel must fit eight waves
per SIMD (<= 64 VGPRs, nothing in scratch, no AGPRs), and its row loop, priced in issue cycles by tools/price_kernel.py,
must cost no more than the same source compiled with the former options (SLP vectorisation left on)."""

import importlib.util
import os
import re
import subprocess

import pytest

from genjax._amd import workloads as W
from offline import DEVICE_HDR, FUSED_TAIL, JITC, OPTIONS, ROOT, importance_source, ops, readelf  # noqa: F401

WT_STORES = 0x200  # include/gjx.h GJX_SOURCE_WT_STORES
SHIPPED = OPTIONS + ["-fno-slp-vectorize"]  # compile_options(PlanKind::importance)
FORMER = SHIPPED + ["-fslp-vectorize"]  # the same list with SLP left on (a later option wins): what GJX_JIT_OPTS=-fslp-vectorize builds
KERNEL = "gjx_plan_kernel_philox"


def _pricer():
    spec = importlib.util.spec_from_file_location("price_kernel", os.path.join(ROOT, "tools", "price_kernel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _compile(src, tmp_path, name, options):
    fsrc, fout, flog = (str(tmp_path / f"{name}.{ext}") for ext in ("hip", "co", "log"))
    with open(fsrc, "w") as f:
        f.write(src)
    r = subprocess.run([JITC, fsrc, DEVICE_HDR, fout, flog, *options], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, open(flog).read() if os.path.exists(flog) else r.stderr)
    return fout


def _notes(code_object):
    tool = readelf()
    assert tool is not None, "llvm-readelf (ROCm) is needed to read the code object's notes"
    notes = subprocess.run([tool, "--notes", code_object], capture_output=True, text=True, timeout=60).stdout
    blk = [b for b in re.split(r"^  - ", notes.split("amdhsa.kernels:")[1].split("\namdhsa.")[0], flags=re.M)[1:]
           if re.search(rf"^    \.name:\s+{KERNEL}\s*$", b, flags=re.M)][0]
    return {k: int(v) for k, v in re.findall(r"^(?:    )?\.(vgpr_count|agpr_count|private_segment_fixed_size|sgpr_count):\s+(\d+)", blk, flags=re.M)}


@pytest.fixture(scope="module")
def built(ops, tmp_path_factory):
    """The two variants' sources, and the code objects of the shipped and of the former option list (compiled once)."""
    os.environ.pop("GJX_JIT_FORM", None)
    tmp = tmp_path_factory.mktemp("issue_cost")
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = {"default": importance_source(ops, plan, 1), "one_pass": importance_source(ops, plan, 1 | WT_STORES)}
    co = {"default": _compile(src["default"], tmp, "default", SHIPPED), "one_pass": _compile(src["one_pass"], tmp, "one_pass", SHIPPED),
          "default_former": _compile(src["default"], tmp, "default_former", FORMER)}
    return plan, src, co


def test_shipped_options_are_the_library_s():
    text = open(os.path.join(ROOT, "genjax-chi_amd", "csrc", "gjx_plan_jit.hpp")).read()
    body = text.split("inline std::vector<std::string> compile_options(PlanKind kind) {")[1].split("\n}\n")[0]
    assert all(f'"{o}"' in body for o in SHIPPED), body
    assert re.search(r'kind == PlanKind::importance\) opts\.push_back\("-fno-slp-vectorize"\)', body), body


def test_store_kind_is_a_source_variant(built):
    _, src, _ = built
    assert "make_uint4(" in src["default"] and "__launch_bounds__(64" in src["default"]  # the quad form
    assert "const bool wt_one_pass = false;" in src["default"] and "const bool wt_one_pass = true;" in src["one_pass"]
    assert "bt.n_pass <= 1" not in src["default"] + src["one_pass"], "the store kind must not be a run-time branch"
    # nothing else differs
    assert src["default"].replace("wt_one_pass = false", "wt_one_pass = true") == src["one_pass"]


def test_default_kernel_fits_eight_waves(built):
    _, _, co = built
    meta = _notes(co["default"])
    print("default quad kernel, shipped options:", meta)
    assert meta["vgpr_count"] <= 64, meta
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["agpr_count"] == 0, meta
    wt = _notes(co["one_pass"])
    print("one-pass variant, shipped options:", wt)
    assert wt["private_segment_fixed_size"] == 0 and wt["agpr_count"] == 0, wt


def test_both_variants_pass_the_library_check(ops, built):
    plan, _, _ = built
    for flags in (0, WT_STORES, FUSED_TAIL | WT_STORES):
        ops.lib.call("gjx_plan_compile_check", plan.handle, 1 | flags)


def test_priced_cycles_do_not_exceed_the_former_options(built):
    _, _, co = built
    pk = _pricer()
    new, old = pk.price(co["default"], KERNEL), pk.price(co["default_former"], KERNEL)
    print("shipped:", new["counts"], new["priced_cycles"])
    print("former :", old["counts"], old["priced_cycles"])
    assert new["counts"]["multiply"] == old["counts"]["multiply"] and new["counts"]["transcendental"] == old["counts"]["transcendental"]
    assert new["vector_instructions"] > 1000, new  # (the row loop was found)
    assert new["priced_cycles"] <= old["priced_cycles"], (new["priced_cycles"], old["priced_cycles"])
