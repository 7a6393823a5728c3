"""PSIS leave-one-group-out without a GPU (include/gjx_psis_units.h): the unit-sum kernel's source is that of another data set,
n, U and G; it compiles for gfx950 without scratch, flat and grouped; the size function refuses what the
entry point refuses."""

import math
import re

import numpy as np
import pytest

import group_ref as GR
import plate_ref as P
from genjax._amd import abi, temper
from genjax._amd.runtime import use_ops
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)

ENTRY = {"plated": "gjx_psis_units_kernel", "intercept": "gjx_psis_units_grouped_kernel", "slope": "gjx_psis_units_grouped_kernel"}


def _lower(ops, name, sizes, seed):  # noqa: F811
    with use_ops(ops):
        target = GR.target(name, sizes, seed)[0] if name != "plated" else P.target("normal", sum(sizes), seed=seed)[0]
        tr = temper.lower(target, 64)
        return tr, ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_source_compiles_and_holds_no_length(ops, tmp_path, name):  # noqa: F811
    tr, plan = _lower(ops, name, [0, 14, 0, 26, 0], 0)
    src = plan.psis_units_source()
    assert src == _lower(ops, name, GR.LAYOUTS[17], 4)[1].psis_units_source()  # another D, G, group layout and data set
    assert plan.psis_units_compile_check() == 0
    assert ENTRY[name] + "(PsisUnitArgs a" in src and ("GroupCols gc" in src) == (name != "plated")
    data_bits = {"0x%08xu" % int(v) for c in tr.data for v in c.numpy().astype(np.float32).view(np.uint32)}
    assert not (set(re.findall(r"0x[0-9a-f]{8}u", src)) & (data_bits - {"0x00000000u", "0x3f800000u"}))
    # the term is the PSIS kernel's function text
    term = lambda s, nm: s.split(nm + "(", 1)[1].split("\n}\n", 1)[0]
    row = plan.psis_source() if name == "plated" else plan.group_checks_source("psis")
    assert term(src, "float us_term") == term(row, "float ps_term")
    notes = kernel_notes(src, tmp_path, "units_" + name)[ENTRY[name]]
    print(f"unit-sum kernel {name}: {notes}")
    assert notes["private_segment_fixed_size"] == 0 and notes["vgpr_count"] + notes.get("agpr_count", 0) <= 128


def test_header_and_workspace(ops, oracle_ops):  # noqa: F811
    h = abi.CHECK_HEADERS["psis_units"]
    assert header_symbols("gjx_psis_units.h") == set(h.prototypes) and h in abi.bound_headers() and h not in abi.all_optional_headers()
    assert ops.lib.has["psis_units"] and not oracle_ops.lib.has["psis_units"]
    ws = lambda *a: int(ops.lib.call("gjx_psis_units_workspace_bytes", *a))
    assert ws(1000, 9, 95, 0) > ws(1000, 9, 95, 16 * 1000) > 0  # (a smaller table: a smaller workspace)
    for bad in ((0, 9, 95, 0), (1 << 31, 9, 95, 0), (1000, 0, 95, 0), (1000, 1 << 31, 95, 0), (1000, 9, 4, 0), (1000, 9, 4096, 0), (1000, 9, 95, 16 * 1000 - 1)):
        assert ws(*bad) == 0, bad


def test_end_to_end_reference():
    """The condition and the record behind tests/test_gpu_logo.py::test_end_to_end, on its first three seeds: every unit of the
    float64 restatement has khat below the threshold, and the errors lie in the recorded range."""
    import test_gpu_logo as T

    e = T.e2e_errors(T.e2e_model(), T.E2E_SEEDS[:3])
    assert abs(T.closed_form_logo(T.e2e_model()).sum() + 77.6253) < 1e-4
    assert e[:, 1].max() <= T.E2E_MAX_KHAT < min(1.0 - 1.0 / math.log10(T.E2E_N), 0.7) and -0.1344 <= e[:, 0].min() and e[:, 0].max() <= 0.1103
