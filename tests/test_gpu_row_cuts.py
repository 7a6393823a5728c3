"""The row-loop cuts of the quad importance kernel on the device, against the unchanged oracle bit for bit: the "full outputs"
source variant (a launch that passes score, logw, max_partials, row_e and row_s runs a kernel that asks nothing about them;
every other set of outputs runs the guarded one), the exact zero-add cuts of the site emission, the wave maximum on ordered
integer keys and rowfix's trims (gjx_plan_jit.hpp, gjx_device.hpp).

Models: the flagship sites (every rule fires), sigma = 0.3 with nonzero locations (none does) and a model built so that the
rules must not fire (location -0.0, a reference with scale 2).  One lane / one full wave / a row with one live lane / four
rows and a lane; 1, 3 and 32 passes per launch; four sets of outputs.  One LGSSM scan and one LGSSM filter step, which share
rowfix, the epilogue and the sampler.  One launch runs both forms of a normal(0, 1) site's value over every angle word at
the two smallest radii."""

import ctypes as C

import pytest
import torch

from genjax._amd import abi, prng, workloads as W

pytestmark = pytest.mark.gpu

SEED = 97
POPULATIONS = [4, 256, 260, 1028]
PASSES = [1, 3, 32]
SENTINEL = 1234.5
# name -> (score, max_partials, rows) passed?  (logw always is)
OUTPUTS = {"all": (True, True, True), "no_score": (False, True, True), "no_max_partials": (True, False, True), "logw_and_rows": (False, False, True)}


def same(a, b, what):
    a, b = a.cpu(), b.cpu()
    ok = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
    assert ok, f"{what}: {int((a != b).sum())} of {a.numel()} differ"


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
    """z ~ Normal(0.25, 0.3); x ~ Normal(z + 0.1, 0.3); y ~ Normal(x, 0.3) observed at 0.7."""
    return [_site(abi.DIST_NORMAL, _c(0.25), _c(0.3), 0), _site(abi.DIST_NORMAL, abi.Arg(abi.ARG_SITE, 0, 1.0, 0.1, None), _c(0.3), 1),
            _site(abi.DIST_NORMAL, abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None), _c(0.3), obs=_c(0.7))]


def unfired_sites():
    """z ~ Normal(-0.0, 1); x ~ Normal(2 z, 1); y ~ Normal(x, 0.5) observed at 0.7: the location is -0.0 and the reference has
    scale 2 (tests/test_row_cuts_cpu.py asserts on the source that neither rule fires)."""
    return [_site(abi.DIST_NORMAL, _c(-0.0), _c(1.0), 0), _site(abi.DIST_NORMAL, abi.Arg(abi.ARG_SITE, 0, 2.0, 0.0, None), _c(1.0), 1),
            _site(abi.DIST_NORMAL, abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None), _c(0.5), obs=_c(0.7))]


MODELS = {"flagship": (lambda: W.gaussian10_sites(W.gaussian10_data()), W.G10_LATENTS), "sigma03": (sigma03_sites, 2), "unfired": (unfired_sites, 2)}


def keys_of(p, n):
    return W.importance_particle_keys(prng.key(SEED + p, 1), n, 0)  # (a parent key of its own per pass)


_PLANS, _REF = {}, {}


def plans_of(hip_ops, oracle_ops, model):
    if model not in _PLANS:
        make, _ = MODELS[model]
        _PLANS[model] = (hip_ops.plan_create(make()), oracle_ops.plan_create(make()))
    return _PLANS[model]


def reference(oracle_ops, oplan, model, p, n):
    """The oracle's pass p over n particles (computed once, shared by the four sets of outputs, never modified)."""
    k = (model, p, n)
    if k not in _REF:
        ncol = MODELS[model][1]
        vals, score, logw, mp, rows = oracle_ops.importance_run(oplan, keys_of(p, n), n, [], [torch.float32] * ncol, want_rows=True)
        _REF[k] = dict(values=vals, score=score, logw=logw, mp=mp, row_e=rows.e, row_s=rows.s)
    return _REF[k]


def launch(ops, plan, ncol, n, L, outputs):
    want_score, want_mp, _ = OUTPUTS[outputs]
    stride, R = -(-n // 256) * 256, ops.num_max_partials(n)
    full = lambda shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=ops.device())  # noqa: E731
    o = dict(values=[ops.empty((L, stride), torch.float32) for _ in range(ncol)], score=full((L, stride)), logw=full((L, stride)),
             mp=full((L, R)), row_e=ops.empty((L, R), torch.int32), row_s=ops.empty((L, R), torch.int64))
    keys = (abi.Keys * L)(*[ops._keys(keys_of(p, n), n) for p in range(L)])
    ins = (C.c_void_p * 1)()
    outs = (C.c_void_p * ncol)(*[t.data_ptr() for t in o["values"]])
    ops.lib.call("gjx_importance_run_batch", plan.handle, keys, L, stride, R, ins, 0, outs, ncol, ops._p(o["score"]) if want_score else None,
                 ops._p(o["logw"]), n, ops._p(o["mp"]) if want_mp else None, ops._p(o["row_e"]), ops._p(o["row_s"]), ops.stream())
    return o


def check(o, ref, ncol, n, p, outputs, tag):
    want_score, want_mp, _ = OUTPUTS[outputs]
    for c in range(ncol):
        same(o["values"][c][p, :n], ref["values"][c], f"column {c}, {tag}")
    same(o["logw"][p, :n], ref["logw"], f"logw, {tag}")
    same(o["row_e"][p], ref["row_e"], f"row anchors e, {tag}")
    same(o["row_s"][p], ref["row_s"], f"row sums S, {tag}")
    if want_score:
        same(o["score"][p, :n], ref["score"], f"score, {tag}")
    else:
        assert bool((o["score"] == SENTINEL).all()), f"an absent score was written, {tag}"
    if want_mp:
        same(o["mp"][p], ref["mp"], f"row maxima, {tag}")
    else:
        assert bool((o["mp"] == SENTINEL).all()), f"absent row maxima were written, {tag}"


@pytest.mark.parametrize("outputs", list(OUTPUTS))
@pytest.mark.parametrize("model", list(MODELS))
def test_importance_kernels_equal_the_oracle(hip_ops, oracle_ops, model, outputs):
    hplan, oplan = plans_of(hip_ops, oracle_ops, model)
    ncol = MODELS[model][1]
    for n in POPULATIONS:
        for L in PASSES:
            o = launch(hip_ops, hplan, ncol, n, L, outputs)
            for p in range(L):
                check(o, reference(oracle_ops, oplan, model, p, n), ncol, n, p, outputs, f"{model}, {outputs}, n={n}, pass {p} of {L}")


def test_the_flagged_variant_is_built_for_every_output_only(hip_ops):
    """gjx_jit_stats: a launch with every output compiles a kernel of its own (one per kind of store); the other three sets of
    outputs share the guarded kernel."""
    sites = sigma03_sites()
    sites[1].arg[1] = _c(0.2871)  # a structure no other test compiles
    plan = hip_ops.plan_create(sites)
    compiles = lambda: hip_ops.jit_stats()["compiles"]  # noqa: E731
    c0 = compiles()
    launch(hip_ops, plan, 2, 260, 3, "no_score")
    assert compiles() == c0 + 1, "the guarded kernel, plain stores"
    launch(hip_ops, plan, 2, 260, 3, "all")
    assert compiles() == c0 + 2, "every output: the variant that asks nothing"
    for outputs in ("no_max_partials", "logw_and_rows", "no_score", "all"):
        launch(hip_ops, plan, 2, 260, 3, outputs)
    assert compiles() == c0 + 2, "the other sets of outputs share the guarded kernel"
    launch(hip_ops, plan, 2, 260, 1, "all")
    assert compiles() == c0 + 3, "every output, one pass: the variant with write-through stores"
    launch(hip_ops, plan, 2, 260, 1, "logw_and_rows")
    assert compiles() == c0 + 4, "the guarded kernel, write-through stores"
    for outputs in OUTPUTS:
        launch(hip_ops, plan, 2, 260, 1, outputs)
    assert compiles() == c0 + 4


def test_lgssm_scan_equals_the_oracle(hip_ops, oracle_ops):
    got, ref = W.lgssm_scan(hip_ops, 1, SEED, 1024, 3), W.lgssm_scan(oracle_ops, 1, SEED, 1024, 3)
    for k in ("x", "logw", "score", "carry", "max_partials", "row_e", "row_s"):
        same(got[k], ref[k], f"LGSSM scan {k}")
    assert got["log_z"] == ref["log_z"]


def test_lgssm_filter_step_equals_the_oracle(hip_ops, oracle_ops):
    h = W.lgssm_smc(hip_ops, 1, seed=SEED, n=1024, T=2, want_ancestors=True)
    o = W.lgssm_smc(oracle_ops, 1, seed=SEED, n=1024, T=2, want_ancestors=True)
    for k in ("ancestors", "out_e", "out_q", "state", "logw"):
        same(h[k], o[k], f"LGSSM filter {k}")
    assert h["log_z"] == o["log_z"]


def test_zero_location_forms_agree_on_the_device(hip_ops):
    """(r t) + 0 against fma(r, t, 0) over all 2^24 angle words, both outputs, at r = 0 (radius word 0xFFFFFFFF) and at the
    smallest nonzero radius (0xFFFFFF7F: u = 1 - 2^-24), in one launch."""
    fn = hip_ops.lib._dll.gjx_debug_zero_loc_sweep  # (a debug entry of libgjx_hip.so outside the headers)
    fn.restype, fn.argtypes = C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    out = torch.tensor([0, -1], dtype=torch.int64, device=hip_ops.device())
    assert fn(0xFFFFFFFF, 0xFFFFFF7F, out.data_ptr(), hip_ops.stream()) == 0
    bad, first = (int(v) for v in out.cpu())
    assert bad == 0, f"the two forms differ at {bad} (radius, angle) words, the first at angle index {first & 0xFFFFFF:#08x}"
