"""The shared host path of gjx_temper_pointwise and gjx_temper_predictive without a GPU: where a call has TWO defects, the
status is the one the entry points returned when each had its own copy of the checks (recorded from that build):
GJX_ERR_INVALID before GJX_ERR_WORKSPACE before GJX_ERR_UNSUPPORTED, decided on the host (the pointers are never followed)."""

import ctypes as C

import pytest

import genjax
import plate_ref as P
import temper_ref as R
from genjax._amd import abi, temper
from genjax._amd.runtime import use_ops
from offline import ops  # noqa: F401  (a fixture)

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
D, N = 20, 1000


def _plans(ops):  # noqa: F811
    """-> (a plated plan with its parameters set and NO data, the same with data, a plan without a plated site)"""
    with use_ops(ops):
        tr = temper.lower(P.target("normal", D)[0], 64)
        bare, ready = (ops.temper_plan_create(tr.sites, keep=(tr.keep, tr)).set_params(tr.params) for _ in range(2))
        t2 = temper.lower(R.models()["regression"], 64)
        flat = ops.temper_plan_create(t2.sites, keep=(t2.keep, t2)).set_params(t2.params)
    assert ops.lib._gjx_temper_plan_set_data(ready.handle, (C.c_void_p * 2)(0x5000, 0x6000), 2, D) == 0
    return bare, ready, flat


@pytest.mark.parametrize("what", ["pointwise", "predictive"])
def test_two_defects_at_once(ops, monkeypatch, what):  # noqa: F811
    lib = ops.lib
    bare, ready, flat = _plans(ops)
    need = int(lib.call(f"gjx_{what}_workspace_bytes", N, D, *((1,) if what == "predictive" else ())))
    key = ops._keys(genjax.random.key(3, "philox").literal(), 1)

    def io(**kw):
        o = abi.PointwiseIO() if what == "pointwise" else abi.PredictiveIO()
        o.n, o.out, o.ws, o.ws_bytes = N, 0x4000, 0x8000, need
        o.x[0], o.x[1] = 0x1000, 0x2000
        for k, v in kw.items():
            if k == "x1":
                o.x[1] = v
            else:
                setattr(o, k, v)
        return o

    def call(plan, o):
        ref = C.byref(o) if o is not None else None
        if what == "pointwise":
            return lib._gjx_temper_pointwise(plan.handle, ref, None)
        return lib._gjx_temper_predictive(plan.handle, C.byref(key), ref, None)

    monkeypatch.setenv("GJX_PLAN_JIT", "0")  # whatever passes every check stops at GJX_ERR_UNSUPPORTED: nothing is launched
    assert call(ready, io()) == UNSUPPORTED
    # each defect alone
    assert call(ready, io(x1=None)) == INVALID and call(ready, io(ws_bytes=need - 1)) == WORKSPACE
    assert call(bare, io()) == INVALID and call(ready, io(ws=0x8004)) == INVALID
    assert call(flat, io()) == INVALID and call(ready, None) == INVALID
    # ... and in pairs: the statuses of the build before the two entry points shared their checks
    assert call(ready, io(x1=None, ws_bytes=need - 1)) == INVALID  # a null column, a short workspace
    assert call(ready, io(x1=None, ws=None)) == INVALID  # a null column, no workspace
    assert call(bare, io(ws=0x8004)) == INVALID  # no set_data, a misaligned workspace
    assert call(bare, io(ws_bytes=need - 1)) == INVALID  # no set_data, a short workspace
    assert call(flat, None) == INVALID  # no plated site, a null io
    assert call(ready, io(ws=0x8004, ws_bytes=need - 1)) == INVALID  # misaligned and short
    assert call(ready, io(ws_bytes=need - 1)) == WORKSPACE  # short, and the compiler switched off
