"""What the tests that run without a GPU share: libgjx_hip.so loaded without a device (plans are host objects: no compute
call is made), the symbols a header declares, and generated sources compiled for gfx950 by the library's own helper with
their code-object notes read back."""

import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from genjax._amd.abi import GjxLib
from genjax._amd.ops import Ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "genjax-chi_amd", "lib")
HIP_LIB = os.path.join(LIB_DIR, "libgjx_hip.so")
JITC = os.path.join(LIB_DIR, "gjx_jitc")
DEVICE_HDR = os.path.join(ROOT, "genjax-chi_amd", "csrc", "gjx_device.hpp")
OPTIONS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"]  # gjx_plan_jit.hpp compile_options()
FUSED_TAIL = 0x100  # include/gjx.h GJX_SOURCE_FUSED_TAIL


@pytest.fixture(scope="module")
def ops():
    """(A fixture: the modules that use it import it by name.)"""
    if not os.path.exists(HIP_LIB) or not os.path.exists(JITC):
        import __graft_entry__ as g

        g.build()
    return Ops(GjxLib(HIP_LIB, "cuda"))  # no compute calls: plans are host objects


def header_symbols(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(gjx_[a-z0-9_]+)\s*\(", txt))


def llvm_tool(name):
    for cand in (f"/opt/rocm/llvm/bin/{name}", f"/opt/rocm/lib/llvm/bin/{name}"):
        if os.path.exists(cand):
            return cand
    return shutil.which(name)


def readelf():
    return llvm_tool("llvm-readelf")


def importance_source(ops, plan, impl):
    """gjx_plan_specialized_source (SMC, guided and backward-simulation plans have a `source` method of their own)."""
    need = C.c_size_t()
    ops.lib.call("gjx_plan_specialized_source", plan.handle, impl, None, 0, C.byref(need))
    buf = C.create_string_buffer(need.value)
    ops.lib.call("gjx_plan_specialized_source", plan.handle, impl, buf, need.value, None)
    return buf.value.decode()


def source_shape(src):
    """-> (struct names, kernel names, the source without its one generated struct and without the prelude's #include):
    what a generated source of the fixed-body kinds consists of (gjx_plan_jit.hpp: a generator emits what the table decides)."""
    src = src.replace('#include "gjx_device.hpp"\n', "")
    structs = re.findall(r"^struct (\w+) \{$", src, flags=re.M)
    kernels = re.findall(r'^extern "C" __global__ __launch_bounds__\(256\) void (\w+)\(', src, flags=re.M)
    rest = re.sub(r"^struct \w+ \{\n.*?^\};\n", "", src, flags=re.M | re.S)
    return structs, kernels, rest


def kernel_notes(src, tmp_path, name):
    """Compile `src` with the helper the library itself uses (the code object stays at tmp_path / f"{name}.co") and read its
    notes -> {kernel: {field: int}}, fields vgpr_count, agpr_count, sgpr_count, private_segment_fixed_size."""
    tool = readelf()
    if tool is None:
        pytest.skip("llvm-readelf is not installed")
    fsrc, fout, flog = (str(tmp_path / f"{name}.{ext}") for ext in ("hip", "co", "log"))
    with open(fsrc, "w") as f:
        f.write(src)
    r = subprocess.run([JITC, fsrc, DEVICE_HDR, fout, flog, *OPTIONS], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, open(flog).read() if os.path.exists(flog) else r.stderr)
    notes = subprocess.run([tool, "--notes", fout], capture_output=True, text=True, timeout=60).stdout
    out = {}
    # one entry of the amdhsa.kernels list per kernel, its own fields four columns in (an argument's lie deeper)
    for blk in re.split(r"^  - ", notes.split("amdhsa.kernels:")[1].split("\namdhsa.")[0], flags=re.M)[1:]:
        kname = re.search(r"^    \.name:\s+(\S+)", blk, flags=re.M).group(1)
        out[kname] = {k: int(v) for k, v in re.findall(
            r"^(?:    )?\.(vgpr_count|agpr_count|private_segment_fixed_size|sgpr_count):\s+(\d+)", blk, flags=re.M)}
    return out
