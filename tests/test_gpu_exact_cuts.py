"""The bit-exact cuts of the sampler and the Normal log-density on the device (gjx_device.hpp bm_pair, sqrt_pos, the fused
overload of logpdf_normal_pre) against the general square root and against the unchanged oracle, bit for bit.

sqrt_pos: one launch compares it with the correctly rounded square root at every float of [1e-7, 45] and at both zeros
(the hardware's reciprocal-square-root estimate is the one input the CPU sweep of tools/check_exact_cuts.cpp can only
bracket).  Importance kernels: the three PHILOX forms (four, two, one particle per lane), one lane / one full row / a
partial second row / five rows, 1, 3 and 32 passes per launch, on the flagship sites (every log-density fused), on a model
with nonzero locations and sigma = 0.3 (nothing fused) and on a model whose scales are computed from a Gamma site at run
time.  One LGSSM scan and one LGSSM filter step, which share the sampler."""

import ctypes as C

import numpy as np
import pytest
import torch

from genjax._amd import abi, prng, workloads as W

pytestmark = pytest.mark.gpu

SEED = 83
POPULATIONS = [4, 256, 260, 1028]
PASSES = [1, 3, 32]
FORMS = {4: 0, 2: 2, 1: 1}  # particles per lane -> the columns' offset in floats (16- / 8- / 4-byte aligned)


def same(a, b, what):
    a, b = a.cpu(), b.cpu()
    ok = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
    assert ok, f"{what}: {int((a != b).sum())} of {a.numel()} differ"


def test_sqrt_pos_equals_the_general_square_root_on_its_domain(hip_ops):
    fn = hip_ops.lib._dll.gjx_debug_sqrt_pos_sweep  # (a debug entry of libgjx_hip.so outside the headers)
    fn.restype, fn.argtypes = C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    lo, hi = int(np.float32(1e-7).view(np.uint32)), int(np.float32(45.0).view(np.uint32))
    assert hi - lo + 1 == 240992364
    for a, b, what in ((lo, hi, "[1e-7, 45]"), (0, 0, "+0"), (0x80000000, 0x80000000, "-0")):
        out = torch.tensor([0, -1], dtype=torch.int64, device=hip_ops.device())
        assert fn(a, b, out.data_ptr(), hip_ops.stream()) == 0
        bad, first = (int(v) for v in out.cpu())
        assert bad == 0, f"sqrt_pos differs from sqrtf at {bad} floats of {what}, the smallest with bits {first & 0xFFFFFFFF:#010x}"


def _c(v):
    return abi.Arg(abi.ARG_CONST, 0, 0.0, v, None)


def _site(dist, a0, a1, out_col=-1, obs=None):
    s = abi.Site()
    s.dist, s.observed, s.out_col = dist, 0 if obs is None else 1, out_col
    s.arg[0], s.arg[1] = a0, a1
    if obs is not None:
        s.obs = obs
    return s


def sigma03_sites():
    """z ~ Normal(0.25, 0.3); x ~ Normal(z + 0.1, 0.3); y ~ Normal(x, 0.3) observed at 0.7: 1 / 0.3 is no power of two."""
    return [_site(abi.DIST_NORMAL, _c(0.25), _c(0.3), 0), _site(abi.DIST_NORMAL, abi.Arg(abi.ARG_SITE, 0, 1.0, 0.1, None), _c(0.3), 1),
            _site(abi.DIST_NORMAL, abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None), _c(0.3), obs=_c(0.7))]


def runtime_scale_sites():
    """g ~ Gamma(2, 2); x ~ Normal(0.5, g + 0.1); y ~ Normal(x, 0.5 g + 0.2) observed at 0.7: scales known at run time only."""
    return [_site(abi.DIST_GAMMA, _c(2.0), _c(2.0), 0), _site(abi.DIST_NORMAL, _c(0.5), abi.Arg(abi.ARG_SITE, 0, 1.0, 0.1, None), 1),
            _site(abi.DIST_NORMAL, abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None), abi.Arg(abi.ARG_SITE, 0, 0.5, 0.2, None), obs=_c(0.7))]


MODELS = {"flagship": (lambda: W.gaussian10_sites(W.gaussian10_data()), W.G10_LATENTS), "sigma03": (sigma03_sites, 2),
          "runtime_scale": (runtime_scale_sites, 2)}


def keys_of(p, n):
    return W.importance_particle_keys(prng.key(SEED + p, 1), n, 0)  # (a parent key of its own per pass)


_PLANS, _REF = {}, {}


def plans_of(hip_ops, oracle_ops, model):
    if model not in _PLANS:
        make, _ = MODELS[model]
        _PLANS[model] = (hip_ops.plan_create(make()), oracle_ops.plan_create(make()))
    return _PLANS[model]


def reference(oracle_ops, oplan, model, p, n):
    """The oracle's pass p over n particles (computed once, shared by the three forms, never modified)."""
    k = (model, p, n)
    if k not in _REF:
        ncol = MODELS[model][1]
        vals, score, logw, mp, rows = oracle_ops.importance_run(oplan, keys_of(p, n), n, [], [torch.float32] * ncol, want_rows=True)
        _REF[k] = dict(values=vals, score=score, logw=logw, mp=mp, row_e=rows.e, row_s=rows.s)
    return _REF[k]


def columns(ops, L, stride, off):
    return ops.empty(L * stride + 4, torch.float32)[off:off + L * stride].view(L, stride)


def launch(ops, plan, ncol, n, L, form):
    stride, R = -(-n // 256) * 256, ops.num_max_partials(n)
    off = FORMS[form]
    o = dict(values=[columns(ops, L, stride, off) for _ in range(ncol)], score=columns(ops, L, stride, off), logw=columns(ops, L, stride, off),
             mp=ops.empty((L, R), torch.float32), row_e=ops.empty((L, R), torch.int32), row_s=ops.empty((L, R), torch.int64))
    keys = (abi.Keys * L)(*[ops._keys(keys_of(p, n), n) for p in range(L)])
    ins = (C.c_void_p * 1)()
    outs = (C.c_void_p * ncol)(*[t.data_ptr() for t in o["values"]])
    ops.lib.call("gjx_importance_run_batch", plan.handle, keys, L, stride, R, ins, 0, outs, ncol, C.c_void_p(o["score"].data_ptr()),
                 C.c_void_p(o["logw"].data_ptr()), n, ops._p(o["mp"]), ops._p(o["row_e"]), ops._p(o["row_s"]), ops.stream())
    return o


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("model", list(MODELS))
def test_importance_kernels_equal_the_oracle(hip_ops, oracle_ops, model, form):
    hplan, oplan = plans_of(hip_ops, oracle_ops, model)
    ncol = MODELS[model][1]
    for n in POPULATIONS:
        for L in PASSES:
            o = launch(hip_ops, hplan, ncol, n, L, form)
            for p in range(L):
                ref, tag = reference(oracle_ops, oplan, model, p, n), f"{model}, {form} per lane, n={n}, pass {p} of {L}"
                for c in range(ncol):
                    same(o["values"][c][p, :n], ref["values"][c], f"column {c}, {tag}")
                same(o["score"][p, :n], ref["score"], f"score, {tag}")
                same(o["logw"][p, :n], ref["logw"], f"logw, {tag}")
                same(o["mp"][p], ref["mp"], f"row maxima, {tag}")
                same(o["row_e"][p], ref["row_e"], f"row anchors e, {tag}")
                same(o["row_s"][p], ref["row_s"], f"row sums S, {tag}")


def test_lgssm_scan_equals_the_oracle(hip_ops, oracle_ops):
    got, ref = W.lgssm_scan(hip_ops, 1, SEED, 1024, 3), W.lgssm_scan(oracle_ops, 1, SEED, 1024, 3)
    for k in ("x", "logw", "score", "carry", "max_partials", "row_e", "row_s"):
        same(got[k], ref[k], f"LGSSM scan {k}")
    assert got["log_z"] == ref["log_z"]


def test_lgssm_filter_step_equals_the_oracle(hip_ops, oracle_ops):
    """T = 2: the initial population and one step of the library's own bootstrap filter (smc_quad_normals -> bm_pair)."""
    h = W.lgssm_smc(hip_ops, 1, seed=SEED, n=1024, T=2, want_ancestors=True)
    o = W.lgssm_smc(oracle_ops, 1, seed=SEED, n=1024, T=2, want_ancestors=True)
    for k in ("ancestors", "out_e", "out_q", "state", "logw"):
        same(h[k], o[k], f"LGSSM filter {k}")
    assert h["log_z"] == o["log_z"]
