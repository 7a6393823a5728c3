"""The Philox round's three-input XOR as one v_bitop3_b32 (gjx_device.hpp xor3), checked without a GPU.

The default (quad, PHILOX, plain stores) kernel of the 10-latent Gaussian model is compiled for gfx950 twice with the option
list the library ships for importance plans: as shipped, and with the escape macro -DGJX_PHILOX_PLAIN_XOR, which gives the
round its two v_xor_b32 back.  The shipped build must hold no cipher XOR in its row loop, the same multiplies and
transcendentals, fit eight waves per SIMD (<= 64 VGPRs, nothing in scratch, no AGPRs) and price strictly below the escape
build in tools/price_kernel.py, whose price list has v_bitop3_b32 at its own measured rate (tools/README.md: 4.3 cycles, not
the 2.4 of a simple instruction).  The host's plain-XOR form of philox4x32 still gives the Random123 known answers."""

import collections
import json
import os
import shutil
import subprocess

import pytest

from genjax._amd import workloads as W
from offline import DEVICE_HDR, FUSED_TAIL, ROOT, importance_source, ops  # noqa: F401
from test_importance_issue_cost import KERNEL, SHIPPED, WT_STORES, _compile, _notes, _pricer

ESCAPE = SHIPPED + ["-DGJX_PHILOX_PLAIN_XOR"]  # what GJX_JIT_DEFINE=GJX_PHILOX_PLAIN_XOR builds
GOLD = os.path.join(ROOT, "tests", "golden", "rng_kat.json")


def _loop_mnemonics(pk, code_object):
    _, instrs = pk.disassemble(code_object, KERNEL)
    return collections.Counter(instrs[i][1].split("_e32")[0].split("_e64")[0] for i in pk.largest_loop(instrs))


@pytest.fixture(scope="module")
def built(ops, tmp_path_factory):
    """The default flagship source and its two code objects (compiled once)."""
    os.environ.pop("GJX_JIT_FORM", None)
    tmp = tmp_path_factory.mktemp("philox_xor3")
    plan = ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))
    src = importance_source(ops, plan, 1)
    return plan, src, {"shipped": _compile(src, tmp, "shipped", SHIPPED), "escape": _compile(src, tmp, "escape", ESCAPE)}


def test_price_list_has_the_measured_bitop3_rate():
    pk = _pricer()
    assert pk.classify("v_bitop3_b32") == "bitop3" and pk.classify("v_xor_b32_e32") == "simple"
    # measured (tools/README.md): one v_bitop3_b32 4.26 cycles, the v_xor_b32 pair it replaces 4.98
    assert pk.RATES["simple"] < pk.RATES["bitop3"] < 2 * pk.RATES["simple"]
    assert pk.RATES["bitop3"] == 4.3


def test_no_cipher_xor_is_left_in_the_row_loop(built):
    _, _, co = built
    pk = _pricer()
    new, old = _loop_mnemonics(pk, co["shipped"]), _loop_mnemonics(pk, co["escape"])
    print("shipped:", {k: new[k] for k in ("v_xor_b32", "v_bitop3_b32", "v_mad_u64_u32")})
    print("escape :", {k: old[k] for k in ("v_xor_b32", "v_bitop3_b32", "v_mad_u64_u32")})
    assert old["v_xor_b32"] >= 300 and old["v_bitop3_b32"] == 0, old  # (the escape build is the former round)
    assert new["v_xor_b32"] <= old["v_xor_b32"] // 10, (new["v_xor_b32"], old["v_xor_b32"])
    assert new["v_bitop3_b32"] >= old["v_xor_b32"] // 2, new
    assert new["v_mad_u64_u32"] == old["v_mad_u64_u32"]


def test_shipped_build_fits_eight_waves(built):
    _, _, co = built
    meta = _notes(co["shipped"])
    print("shipped:", meta, " escape:", _notes(co["escape"]))
    assert meta["vgpr_count"] <= 64, meta
    assert meta["private_segment_fixed_size"] == 0, meta
    assert meta["agpr_count"] == 0, meta


def test_shipped_build_prices_below_the_escape_build(built):
    _, _, co = built
    pk = _pricer()
    new, old = pk.price(co["shipped"], KERNEL), pk.price(co["escape"], KERNEL)
    print("shipped:", new["counts"], new["vector_instructions"], new["priced_cycles"])
    print("escape :", old["counts"], old["vector_instructions"], old["priced_cycles"])
    assert new["counts"]["multiply"] == old["counts"]["multiply"] and new["counts"]["transcendental"] == old["counts"]["transcendental"]
    assert old["counts"]["bitop3"] == 0 and new["counts"]["bitop3"] > 0
    assert new["vector_instructions"] > 1000, new  # (the row loop was found)
    assert new["priced_cycles"] < old["priced_cycles"], (new["priced_cycles"], old["priced_cycles"])


def test_variants_pass_the_library_check(ops, built):
    """The one-pass (write-through stores) and the fused-tail variant, in every form, compile with the new round."""
    plan, _, _ = built
    for flags in (WT_STORES, FUSED_TAIL | WT_STORES):
        ops.lib.call("gjx_plan_compile_check", plan.handle, 1 | flags)


def test_variants_have_no_scratch(ops, built, tmp_path):
    plan, _, _ = built
    for name, flags in (("one_pass", WT_STORES), ("fused_tail", FUSED_TAIL | WT_STORES)):
        meta = _notes(_compile(importance_source(ops, plan, 1 | flags), tmp_path, name, SHIPPED))
        print(name, meta)
        assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0, (name, meta)


HOST_PROGRAM = r"""
#include "gjx_device.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {  // argv: groups of six hex words (key 0, 1, counter 0 .. 3) -> one line of four words each
  for (int i = 1; i + 5 < argc; i += 6) {
    uint32_t w[6], o[4];
    for (int j = 0; j < 6; ++j) w[j] = (uint32_t)strtoul(argv[i + j], nullptr, 16);
    gjx::philox4x32(w[0], w[1], w[2], w[3], w[4], w[5], o[0], o[1], o[2], o[3]);
    printf("%08x %08x %08x %08x\n", o[0], o[1], o[2], o[3]);
  }
  return 0;
}
"""


def test_host_form_gives_the_known_answers(tmp_path):
    """philox4x32 compiled for the HOST (no device pass: the builtin does not exist there, so this is the plain-XOR form)
    against the Random123 vectors of tests/golden/rng_kat.json (zeros, ones and the digits of pi)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is needed to compile the host form"
    src, exe = tmp_path / "philox_host.cpp", tmp_path / "philox_host"
    src.write_text(HOST_PROGRAM)
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-I", os.path.dirname(DEVICE_HDR), "-o", str(exe), str(src)],
                   check=True, capture_output=True, text=True, timeout=600)
    kat = [(v["key"] + v["ctr"], v["out"]) for v in json.load(open(GOLD))["philox4x32_10"]]
    r = subprocess.run([str(exe), *[w for words, _ in kat for w in words]], check=True, capture_output=True, text=True, timeout=60)
    assert [line.split() for line in r.stdout.splitlines()] == [out for _, out in kat]
