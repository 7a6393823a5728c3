#!/usr/bin/env python3
"""The directory profiles/collect_occupancy.sh filled -> one JSON summary of the importance kernel:
  python3 profiles/summarize_occupancy.py <tag> <collected dir> <out.json>

Durations come from the kernel trace, counters from the two --pmc runs (per launch = 32 passes of 1e6 particles).
Units, as established from profiles/r04_pmc.json: SQ_WAVE_CYCLES / SQ_BUSY_CYCLES / SQ_WAIT_INST_ANY count in units of FOUR
clock cycles (1856 vector instructions of one wave do not fit into the 4960 "cycles" a wave lives otherwise).
The trace's VGPR_Count column is HALF of what the code object allocates on gfx950 (every entry doubles to a multiple of
the allocation granule of 8: 68 -> 136 = 132 rounded up); the allocation itself is printed by the library under
GJX_PLAN_JIT_VERBOSE=1 (hipFuncGetAttribute NUM_REGS) and asserted by tests/test_importance_occupancy.py from the code
object's notes.  Waves per SIMD that fit = 512 // allocation rounded up to 8, at most 8."""
import collections
import csv
import glob
import json
import os
import statistics
import sys

tag, src, out = sys.argv[1], sys.argv[2], sys.argv[3]
CLOCK_HZ = 2.4e9   # MI355X peak engine clock
N_SIMD = 256 * 4   # 256 CUs x 4 SIMDs
KERNEL = "gjx_plan_kernel_philox"


def newest(pattern):
    files = glob.glob(os.path.join(src, pattern), recursive=True)
    assert files, pattern
    return max(files, key=os.path.getmtime)


durs, vg = collections.defaultdict(list), {}
for r in csv.DictReader(open(newest("trace/**/*kernel_trace.csv"))):
    if KERNEL in r["Kernel_Name"]:
        # (threads of the whole grid: an importance launch is (rows of a pass, passes) workgroups, so x alone is the same for
        # launches of any number of passes; the counter tables' Grid_Size is the whole grid as well)
        g = int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y") or 1) * int(r.get("Grid_Size_Z") or 1)
        durs[g].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        vg[g] = int(r["VGPR_Count"])
grid = max(durs, key=lambda g: len(durs[g]))  # the timed launches (32 passes each)
ts = durs[grid]
ctr = collections.defaultdict(list)
for d in ("pmc1", "pmc2"):
    for r in csv.DictReader(open(newest(f"{d}/**/*counter_collection.csv"))):
        if KERNEL in r["Kernel_Name"] and int(r["Grid_Size"]) == grid:
            ctr[r["Counter_Name"]].append(float(r["Counter_Value"]))
c = {k: statistics.median(v) for k, v in ctr.items()}
passes = 32
med_ns = statistics.median(ts)
cycles = med_ns * 1e-9 * CLOCK_HZ
alloc = 2 * vg[grid]
res = {
    "tag": tag,
    "grid_threads": grid,
    "launches": len(ts),
    "passes_per_launch": passes,
    "kernel_ns_per_launch_median": med_ns,
    "kernel_ns_per_launch_min": min(ts),
    "kernel_us_per_pass_median": med_ns / passes / 1e3,
    "trace_VGPR_Count_column(half_the_allocation)": vg[grid],
    "allocated_vgprs_from_trace(2x_column)": alloc,
    "waves_per_simd_that_fit": min(8, 512 // alloc),
    "counters_per_launch_median": c,
}
if {"SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_INSTS_VALU"} <= set(c):
    res["wave_lifetime_cycles"] = 4.0 * c["SQ_WAVE_CYCLES"] / c["SQ_WAVES"]
    res["resident_waves_per_simd_average"] = 4.0 * c["SQ_WAVE_CYCLES"] / (cycles * N_SIMD)
    res["cycles_per_valu_instruction_per_simd"] = cycles * N_SIMD / c["SQ_INSTS_VALU"]
    res["valu_instructions_per_wave"] = c["SQ_INSTS_VALU"] / c["SQ_WAVES"]
if {"SQ_WAVES", "SQ_INSTS_SALU"} <= set(c):
    res["salu_instructions_per_wave"] = c["SQ_INSTS_SALU"] / c["SQ_WAVES"]
if {"SQ_WAIT_INST_ANY", "SQ_WAVE_CYCLES"} <= set(c):
    res["waiting_fraction_of_wave_cycles"] = c["SQ_WAIT_INST_ANY"] / c["SQ_WAVE_CYCLES"]
res["note"] = (f"durations from the trace run, counters from the counter runs (kernels serialised); cycles = duration x {CLOCK_HZ / 1e9} GHz; "
               f"{N_SIMD} SIMDs; cycle counters taken as units of 4 cycles")
json.dump(res, open(out, "w"), indent=1)
