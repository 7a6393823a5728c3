"""include/gjx_quantiles.h without a GPU: the header's registration, the refusals of the size function and of
TemperedSMC.summary."""

import pytest

import group_ref as GR
from genjax._amd import abi
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from offline import header_symbols, ops  # noqa: F401  (ops: a fixture)


def test_header_is_registered(ops, oracle_ops):  # noqa: F811
    h = abi.SUMMARY_HEADERS["quantiles"]
    assert list(abi.SUMMARY_HEADERS) == ["quantiles"]
    assert h in abi.bound_headers() and h not in abi.all_optional_headers() and h not in abi.CHECK_HEADERS.values()
    assert abi.bound_headers() == (*abi.all_optional_headers(), h, *abi.CHECK_HEADERS.values())
    syms = header_symbols("gjx_quantiles.h")
    assert h.header == "gjx_quantiles.h" and syms == set(h.prototypes) == set(abi.QUANTILES_PROTOTYPES) and h.version_fn in syms
    assert h.version == abi.QUANTILES_ABI_VERSION == (0, 1) and h.unavailable is abi.QuantilesUnavailable
    for other in abi.bound_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes)), other.header
    assert not (syms & header_symbols("gjx.h")) and not (syms & set(abi.PROTOTYPES))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_quantiles and not oracle_ops.lib.has_quantiles
    with pytest.raises(abi.QuantilesUnavailable, match="gjx_column_quantiles"):
        oracle_ops.lib.call("gjx_column_quantiles", None, None)


def test_refusals(ops):  # noqa: F811
    size = lambda n, C, Q: ops.lib.call("gjx_quantiles_workspace_bytes", n, C, Q)
    top = 2**31 - 1
    assert size(1, 1, 1) > 0 and size(top, top, abi.QUANTILES_MAX_PROBS) > 0
    assert size(1000, 256, 3) == size(1000, 100000, 3) > size(1000, 255, 3)  # (batches: no growth beyond 256 columns)
    for n, C, Q in ((0, 1, 1), (top + 1, 1, 1), (64, 0, 1), (64, top + 1, 1), (64, 1, 0), (64, 1, abi.QUANTILES_MAX_PROBS + 1), (64, 1, -1)):
        assert size(n, C, Q) == 0, (n, C, Q)
    io = abi.ColumnQuantilesIO()
    assert ops.lib._gjx_column_quantiles(None, None) == -1 and ops.lib._gjx_column_quantiles(io, None) == -1  # (NULL everywhere)
    with use_ops(ops):
        alg = TemperedSMC(GR.target("intercept", GR.LAYOUTS[2])[0], 64)
        for probs in ((), (0.1,) * 9, (-0.01, 0.5), (0.5, 1.01), (0.5, float("nan")), 0.5):
            with pytest.raises(ValueError, match="summary: probs"):
                alg.summary([], probs)
