"""The weighted entry points of include/gjx_quantiles.h without a GPU: the refusals of the size function and of the call
(each returns before any launch), and those of SMCResult.summary / Trajectories.summary."""

import ctypes as C

import numpy as np
import pytest
import torch

from genjax._amd import abi
from genjax.inference.smc import SMCResult, Trajectories
from offline import ops  # noqa: F401  (a fixture)


def test_refusals(ops):  # noqa: F811
    size = lambda n, cols, V, Q: ops.lib.call("gjx_weighted_quantiles_workspace_bytes", n, cols, V, Q)
    top = 2**31 - 1
    assert size(1, 1, 1, 1) > 0 and size(top, top, top, abi.QUANTILES_MAX_PROBS) > 0
    assert size(1000, 256, 1, 3) == size(1000, 100000, 1, 3) > size(1000, 255, 1, 3)  # (no growth beyond 256 columns)
    assert size(1000, 256, 256, 3) == size(1000, 100000, 100000, 3) > size(1000, 256, 255, 3)
    for n, cols, V, Q in ((0, 1, 1, 1), (top + 1, 1, 1, 1), (64, 0, 1, 1), (64, top + 1, 1, 1), (64, 1, 1, 0), (64, 1, 1, 9), (64, 1, 1, -1),
                          (64, 4, 0, 1), (64, 4, 5, 1)):
        assert size(n, cols, V, Q) == 0, (n, cols, V, Q)
    call = ops.lib._gjx_weighted_column_quantiles
    probs = np.array([0.5])
    fake = 0x10000  # (never read: every case below is refused on the host)

    def io(**kw):
        a = abi.WeightedQuantilesIO()
        a.n, a.n_segments, a.n_probs, a.probs = 64, 1, 1, probs.ctypes.data_as(C.POINTER(C.c_double))
        a.seg[0].base, a.seg[0].n_cols, a.seg[0].stride = fake, 4, 64
        a.logw, a.n_weight_cols, a.logw_stride, a.quant, a.stats = fake, 2, 64, fake, fake
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert call(None, None) == -1 and call(abi.WeightedQuantilesIO(), None) == -1
    for bad in (dict(logw=None), dict(n_weight_cols=0), dict(n_weight_cols=5), dict(logw_stride=63), dict(quant=None), dict(ws=4)):
        assert call(io(**bad), None) == -1, bad
    assert call(io(), None) not in (0, -1)  # (the shape is right: the missing workspace is what is refused)


def test_summary_refusals():
    res = SMCResult(0.0, None, None, torch.zeros(4), torch.zeros(4), None)
    with pytest.raises(ValueError, match="record_history=True"):
        res.summary()
    tr = Trajectories(torch.zeros(2, 4), None, None, None, None, None, None, [True])
    for probs in ((), (0.1,) * 9, (-0.01, 0.5), (0.5, 1.01), (0.5, float("nan")), 0.5):
        with pytest.raises(ValueError, match="SMCResult.summary: probs"):
            res.summary(probs)
        with pytest.raises(ValueError, match="Trajectories.summary: probs"):
            tr.summary(probs)
