"""include/gjx_group_cov.h without a GPU: the header's registration, the block move source of grouped plans (compiled for
gfx950, no scratch, no shape or data value, the diagonal source untouched), the refusals of the size function and of
TemperedSMC(proposal="block")."""

import re

import numpy as np
import pytest

import group_ref as GR
import temper_cov_ref as TC
from genjax._amd import abi, temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from offline import header_symbols, kernel_notes, ops  # noqa: F401  (ops: a fixture)

ENTRY = "gjx_temper_move_grouped_cov_kernel"


def _plan(ops, name, sizes, seed=0):  # noqa: F811
    with use_ops(ops):
        target, _, _ = GR.target(name, sizes, seed)
        tracer = temper.lower(target, 64)
        return tracer, ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.CHECK_HEADERS["group_cov"]
    assert list(abi.CHECK_HEADERS) == ["psis_units", "group_cov"]
    assert h in abi.bound_headers() and h not in abi.all_optional_headers() and abi.bound_headers()[-1] is h
    syms = header_symbols("gjx_group_cov.h")
    assert h.header == "gjx_group_cov.h" and syms == set(h.prototypes) == set(abi.GROUP_COV_PROTOTYPES) and h.version_fn in syms
    assert h.version == abi.GROUP_COV_ABI_VERSION == (0, 1) and h.unavailable is abi.GroupCovUnavailable
    for other in abi.bound_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes)), other.header
    assert not (syms & header_symbols("gjx.h")) and not (syms & set(abi.PROTOTYPES))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_group_cov and not oracle_ops.lib.has_group_cov
    with pytest.raises(abi.GroupCovUnavailable, match="gjx_group_moments"):
        oracle_ops.lib.call("gjx_group_moments", None, None)


@pytest.mark.parametrize("name", ["intercept", "slope"])
def test_block_source(ops, name, tmp_path):  # noqa: F811
    """S = 1 and S = 2, both generators: the block source compiles for gfx950 without scratch, LDS or a barrier inside the
    register budget of the diagonal grouped kernel (94 .. 108 VGPRs: at most 108), holds no G, n or data value (it is
    the source of another layout and data set), and asking for it leaves the diagonal source as it was."""
    tracer, plan = _plan(ops, name, GR.LAYOUTS[5])
    other = _plan(ops, name, GR.LAYOUTS[17], seed=4)[1]
    for impl in (0, 1):
        before = plan.source(impl)
        src = plan.group_cov_source(impl)
        assert plan.source(impl) == before and ENTRY not in before and "FactorPtr" not in before
        assert plan.group_cov_compile_check(impl) == 0 and src == other.group_cov_source(impl)
        assert ENTRY + "(" in src and "gjx_temper_move_grouped_kernel" not in src and "__shared__" not in src and "__syncthreads" not in src
        data_bits = {"0x%08xu" % int(v) for c in tracer.data for v in c.numpy().astype(np.float32).view(np.uint32)}
        assert not (set(re.findall(r"0x[0-9a-f]{8}u", src)) & (data_bits - {"0x00000000u", "0x3f800000u"}))
        notes = kernel_notes(src, tmp_path, f"gcov_{name}_{impl}")[ENTRY]
        print(f"block move kernel {name} impl {impl}: {notes}")
        assert notes["private_segment_fixed_size"] == 0 and notes.get("group_segment_fixed_size", 0) == 0, notes
        assert notes["vgpr_count"] + notes.get("agpr_count", 0) <= 108, notes


def test_refusals(ops):  # noqa: F811
    size = lambda n, G, S: ops.lib.call("gjx_group_moments_workspace_bytes", n, G, S)
    assert size(1000, 10, 2) > 0 and size(abi.GROUP_MOMENTS_MAX_N, 1, 1) > 0
    for n, G, S in ((0, 1, 1), (abi.GROUP_MOMENTS_MAX_N + 1, 1, 1), (64, 0, 1), (64, abi.GROUP_MAX_GROUPS, 1), (64, 1, 0),
                    (64, 1, abi.GROUP_MAX_SITES + 1), (64, 1, -1)):
        assert size(n, G, S) == 0, (n, G, S)
    with use_ops(ops):
        flat = TC.correlated_target()
        with pytest.raises(ValueError, match='"block".*"covariance"'):
            TemperedSMC(flat, 64, proposal="block")._state()
        grouped = GR.target("slope", GR.LAYOUTS[5])[0]
        with pytest.raises(ValueError, match='scale=.*"block"'):
            TemperedSMC(grouped, 64, proposal="block", scale=0.1)
        with pytest.raises(ValueError, match="proposal must be"):
            TemperedSMC(grouped, 64, proposal="full")
        with pytest.raises(PlanUnsupported, match="covariance.*'a'"):
            TemperedSMC(grouped, 64, proposal="covariance")._state()
        st = TemperedSMC(grouped, 64, proposal="block")._state()
        assert st["tplan"].n_grouped == 2
        assert ops.lib._gjx_group_cov_compile_check(TemperedSMC(flat, 64)._state()["tplan"].handle, 0) == -1  # (no block kernel)


def test_end_to_end_reference():
    """The record behind tests/test_gpu_group_cov.py::test_block_route_end_to_end, on its first three seeds: the closed form,
    the within-group correlation the model is about, and errors of the float64 restatement inside the recorded ranges."""
    import group_cov_ref as V

    m = V.e2e_model()
    G = m.G
    corr = [m.post_cov[2 + k, 2 + G + k] / (m.post_sd[2 + k] * m.post_sd[2 + G + k]) for k in range(G)]
    assert abs(m.log_z + 171.5919) < 1e-3 and max(corr) < -0.9
    ez, em, vr, rate = V.restatement_errors(m, V.E2E_SEEDS[:3])
    print(f"log Z errors {ez.tolist()}, last-stage group accept rates {rate.tolist()}")
    assert -1.777 <= ez.min() and ez.max() <= 0.732 and 0.886 <= vr.min() and vr.max() <= 1.140
    assert V.MIN_LAST_RATE <= rate.min() and rate.max() <= 0.3415 and np.all(np.abs(em) <= V.E2E_FACTOR * np.asarray(V.RMS_MEAN))
