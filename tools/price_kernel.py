#!/usr/bin/env python3
"""Issue-cycle price of a generated kernel's row loop, from its code object (no GPU needed):

  python tools/price_kernel.py <code object> [--kernel NAME] [--json]

The kernel is disassembled with the ROCm llvm-objdump.  Its row loop is found from the control flow alone: the largest
strongly connected component of the instruction graph (fall-through and branch edges), i.e. the grid-stride loop over
rows with every block that branches back into it.  Each instruction of the loop is put into one class by the PREFIX of
its mnemonic (PREFIXES, first match wins) and priced with the class's rate (RATES: cycles of one SIMD's vector issue per
wave64 instruction, measured by tools/microbench/valu_rate.hip and recorded in tools/README.md).  A wait state (`s_nop k`
is k + 1 of them) stalls the wave one cycle.  Scalar, LDS and memory instructions issue through ports of their own, next to
another wave's vector instruction: they are counted and priced 0 in the vector-issue total.

The price is a static one: every instruction of the loop once, both sides of the branches inside it (for the importance
kernels that is the launch with score, log-weights and row sums all present, as the benchmark has it)."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys

# cycles per wave64 instruction per SIMD (tools/README.md has the measurements)
# bitop3: v_bitop3_b32 issues at the packed instructions' rate, not at the simple one (4.26 measured with a scalar third source,
# against 4.98 for the v_xor_b32 pair it replaces in the Philox round)
RATES = {"simple": 2.4, "multiply": 5.5, "transcendental": 8.0, "packed": 4.2, "bitop3": 4.3, "wait_states": 1.0, "scalar": 0.0,
         "lds": 0.0, "memory": 0.0}
# class by mnemonic prefix, first match wins
PREFIXES = [
    ("s_nop", "wait_states"),
    ("s_", "scalar"),
    ("v_pk_", "packed"),
    ("v_bitop3", "bitop3"),
    ("v_mad_u64", "multiply"), ("v_mad_i64", "multiply"), ("v_mul_lo", "multiply"), ("v_mul_hi", "multiply"),
    ("v_sqrt", "transcendental"), ("v_rsq", "transcendental"), ("v_rcp", "transcendental"), ("v_log", "transcendental"),
    ("v_exp", "transcendental"), ("v_sin", "transcendental"), ("v_cos", "transcendental"),
    ("v_", "simple"),
    ("ds_", "lds"),
    ("global_", "memory"), ("buffer_", "memory"), ("flat_", "memory"), ("scratch_", "memory"),
]
CLASSES = ["simple", "multiply", "transcendental", "packed", "bitop3", "wait_states", "scalar", "lds", "memory"]


def objdump():
    for cand in ("/opt/rocm/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-objdump"):
        if os.path.exists(cand):
            return cand
    return shutil.which("llvm-objdump")


def classify(mnemonic):
    for prefix, cls in PREFIXES:
        if mnemonic.startswith(prefix):
            return cls
    raise ValueError(f"no class for {mnemonic!r}")


def disassemble(code_object, kernel=None):
    """-> (kernel name, [(offset, mnemonic, operands, branch target offset or None)]) of one kernel of the code object."""
    tool = objdump()
    if tool is None:
        raise RuntimeError("llvm-objdump is not installed")
    text = subprocess.run([tool, "-d", code_object], capture_output=True, text=True, check=True).stdout
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-fA-F]+ <([^>]+)>:$", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            base = None
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if cur is None or not m:
            continue
        addr = int(m.group(3), 16)
        if base is None:
            base = addr
        t = re.search(r"<[^>+]+\+0x([0-9a-fA-F]+)>\s*$", line) or re.search(r"<([^>+]+)>\s*$", line)
        target = None
        if t and m.group(1).startswith(("s_cbranch", "s_branch")):
            target = int(t.group(1), 16) if "+0x" in t.group(0) else 0
        cur.append((addr - base, m.group(1), m.group(2), target))
    if kernel is None:
        kernel = max(kernels, key=lambda k: len(kernels[k]))
    return kernel, kernels[kernel]


def largest_loop(instrs):
    """Indices of the instructions in the largest strongly connected component of the instruction graph."""
    index_of = {off: i for i, (off, _, _, _) in enumerate(instrs)}
    n = len(instrs)
    succ = [[] for _ in range(n)]
    for i, (_, mn, _, target) in enumerate(instrs):
        if target is not None and target in index_of:
            succ[i].append(index_of[target])
        if not mn.startswith(("s_branch", "s_endpgm", "s_setpc")) and i + 1 < n:
            succ[i].append(i + 1)
    # Tarjan, iteratively
    order, low, on, stack, best, counter = [-1] * n, [0] * n, [False] * n, [], [], 0
    for root in range(n):
        if order[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                order[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on[v] = True
            if k < len(succ[v]):
                work.append((v, k + 1))
                w = succ[v][k]
                if order[w] < 0:
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], order[w])
                continue
            if low[v] == order[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > len(best) and (len(comp) > 1 or v in succ[v]):
                    best = comp
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return sorted(best)


def price(code_object, kernel=None):
    """-> {"kernel", "loop_instructions", "counts": {class: n}, "cycles": {class: c}, "vector_instructions",
    "priced_cycles"} of the kernel's row loop."""
    name, instrs = disassemble(code_object, kernel)
    loop = largest_loop(instrs)
    counts = {c: 0 for c in CLASSES}
    nops = 0
    for i in loop:
        _, mn, ops, _ = instrs[i]
        cls = classify(mn)
        if cls == "wait_states":
            nops += 1
            counts[cls] += int(ops.split()[0], 0) + 1
        else:
            counts[cls] += 1
    cycles = {c: counts[c] * RATES[c] for c in CLASSES}
    return {"kernel": name, "loop_instructions": len(loop), "counts": counts, "s_nop_instructions": nops, "cycles": cycles,
            "vector_instructions": sum(counts[c] for c in ("simple", "multiply", "transcendental", "packed", "bitop3")),
            "priced_cycles": sum(cycles.values())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("code_object")
    ap.add_argument("--kernel", help="kernel symbol (default: the largest kernel of the code object)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    r = price(a.code_object, a.kernel)
    if a.json:
        print(json.dumps(r))
        return 0
    print(f"{r['kernel']}: row loop of {r['loop_instructions']} instructions, {r['vector_instructions']} vector")
    print(f"{'class':16s} {'count':>7s} {'rate':>6s} {'cycles':>9s}")
    for c in CLASSES:
        extra = f"   ({r['s_nop_instructions']} s_nop)" if c == "wait_states" else ""
        print(f"{c:16s} {r['counts'][c]:7d} {RATES[c]:6.1f} {r['cycles'][c]:9.1f}{extra}")
    print(f"{'priced cycles':16s} {'':7s} {'':6s} {r['priced_cycles']:9.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
