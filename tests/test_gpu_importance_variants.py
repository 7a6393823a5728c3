"""The source variants of the flagship importance kernel against the oracle, bit for bit.

The four-particles-per-lane (quad) PHILOX kernel of the 10-latent Gaussian model exists with plain stores (launches of
several passes) and with write-through stores (a launch of ONE pass), each with and without the fused fold, and is built
without SLP vectorisation (gjx_plan_jit.hpp compile_options).  None of that may move a bit: populations of one lane, a short
last row, an exact row and a crossed row boundary, a first particle index of 0 and of 1024, one and three passes per launch,
score and log-weights present and absent, the row sums and the folded log-marginal of every pass."""

import ctypes as C

import pytest
import torch

from genjax._amd import abi, prng, workloads as W

pytestmark = pytest.mark.gpu

SEED = 40
POPULATIONS = [4, 252, 256, 260, 1028]  # one lane / a short last row / an exact row / a row boundary crossed (twice: 4 full rows + one lane)
FIRSTS = [0, 1024]
PASSES = [1, 3]  # 1: the write-through variant; 3: the plain one
DTYPES = [torch.float32] * W.G10_LATENTS


def same(a, b, what):
    a, b = a.cpu(), b.cpu()
    ok = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
    assert ok, f"{what}: {int((a != b).sum())} of {a.numel()} differ"


def keys_of(p, n, first):
    return W.importance_particle_keys(prng.key(SEED + p, 1), n, first)


@pytest.fixture(scope="module")
def plans(hip_ops, oracle_ops):
    sites = W.gaussian10_sites(W.gaussian10_data())
    return hip_ops.plan_create(sites), oracle_ops.plan_create(sites)


_REF = {}


def reference(oracle_ops, plan, p, n, first):
    """The oracle's pass p over particles first .. first + n - 1 (computed once, shared, never modified)."""
    k = (p, n, first)
    if k not in _REF:
        vals, score, logw, mp, rows = oracle_ops.importance_run(plan, keys_of(p, n, first), n, [], DTYPES, want_rows=True)
        lse, e, q = oracle_ops.lse_rows(rows)
        _REF[k] = dict(values=vals, score=score, logw=logw, mp=mp, row_e=rows.e, row_s=rows.s, lse=lse, e=e, q=q)
    return _REF[k]


def launch(ops, plan, n, first, L, want_score=True, want_logw=True, fused=False, cols=None):
    """One launch of L passes through the C ABI (L == 1: gjx_importance_run, optionally with the in-launch fold; else
    gjx_importance_run_batch), then one fold launch of the row sums unless the launch folded them itself."""
    stride, R = -(-n // 256) * 256, ops.num_max_partials(n)
    o = cols or dict(values=[ops.empty((L, stride), torch.float32) for _ in range(W.G10_LATENTS)],
                     score=ops.empty((L, stride), torch.float32), logw=ops.empty((L, stride), torch.float32),
                     mp=ops.empty((L, R), torch.float32), row_e=ops.empty((L, R), torch.int32), row_s=ops.empty((L, R), torch.int64),
                     lse=ops.empty(L, torch.float32), e=ops.empty(L, torch.int32), q=ops.empty(L, torch.int64))
    keys = (abi.Keys * L)(*[ops._keys(keys_of(p, n, first), n) for p in range(L)])
    ins = (C.c_void_p * 1)()
    outs = (C.c_void_p * W.G10_LATENTS)(*[t.data_ptr() for t in o["values"]])
    score = ops._p(o["score"]) if want_score else None
    logw = ops._p(o["logw"]) if want_logw else None
    tail = (ops._p(o["mp"]), ops._p(o["row_e"]), ops._p(o["row_s"]))
    if L == 1:
        lse = abi.LseOut(o["e"].data_ptr(), o["q"].data_ptr(), o["lse"].data_ptr(), None, ops.tickets().data_ptr()) if fused else None
        ops.lib.call("gjx_importance_run", plan.handle, keys, ins, 0, outs, W.G10_LATENTS, score, logw, n, *tail,
                     C.byref(lse) if fused else None, ops.stream())
    else:
        assert not fused
        ops.lib.call("gjx_importance_run_batch", plan.handle, keys, L, stride, R, ins, 0, outs, W.G10_LATENTS, score, logw, n, *tail,
                     ops.stream())
    if not fused:
        ops.lib.call("gjx_lse_rows_batch", ops._p(o["row_e"]), ops._p(o["row_s"]), R, L, R, ops._p(o["e"]), ops._p(o["q"]),
                     ops._p(o["lse"]), None, ops.stream())
    return o


def check(o, oracle_ops, oplan, n, first, L, want_score=True, want_logw=True, what=""):
    for p in range(L):
        ref = reference(oracle_ops, oplan, p, n, first)
        tag = f"{what} n={n} first={first} pass {p} of {L}"
        for c in range(W.G10_LATENTS):
            same(o["values"][c][p, :n], ref["values"][c], f"column {c}, {tag}")
        if want_score:
            same(o["score"][p, :n], ref["score"], f"score, {tag}")
        if want_logw:
            same(o["logw"][p, :n], ref["logw"], f"logw, {tag}")
        same(o["mp"][p], ref["mp"], f"row maxima, {tag}")
        same(o["row_e"][p], ref["row_e"], f"row anchors e, {tag}")
        same(o["row_s"][p], ref["row_s"], f"row sums S, {tag}")
        same(o["lse"][p:p + 1], ref["lse"], f"folded lse, {tag}")
        same(o["e"][p:p + 1], ref["e"], f"folded e, {tag}")
        same(o["q"][p:p + 1], ref["q"], f"folded q, {tag}")


@pytest.mark.parametrize("L", PASSES)
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", POPULATIONS)
def test_variants_equal_the_oracle(hip_ops, oracle_ops, plans, n, first, L):
    hplan, oplan = plans
    check(launch(hip_ops, hplan, n, first, L), oracle_ops, oplan, n, first, L)


@pytest.mark.parametrize("L", PASSES)
@pytest.mark.parametrize("want_score,want_logw", [(False, True), (True, False), (False, False)])
def test_score_and_logw_absent(hip_ops, oracle_ops, plans, L, want_score, want_logw):
    """An absent column is not written (its buffer keeps the sentinel) and everything else is unchanged."""
    hplan, oplan = plans
    n, first = 1028, 1024
    stride, R = -(-n // 256) * 256, hip_ops.num_max_partials(n)
    sentinel = 1234.5
    cols = dict(values=[hip_ops.empty((L, stride), torch.float32) for _ in range(W.G10_LATENTS)],
                score=torch.full((L, stride), sentinel, device=hip_ops.device()), logw=torch.full((L, stride), sentinel, device=hip_ops.device()),
                mp=hip_ops.empty((L, R), torch.float32), row_e=hip_ops.empty((L, R), torch.int32), row_s=hip_ops.empty((L, R), torch.int64),
                lse=hip_ops.empty(L, torch.float32), e=hip_ops.empty(L, torch.int32), q=hip_ops.empty(L, torch.int64))
    o = launch(hip_ops, hplan, n, first, L, want_score, want_logw, cols=cols)
    check(o, oracle_ops, oplan, n, first, L, want_score, want_logw, what=f"score {want_score} logw {want_logw}")
    if not want_score:
        assert bool((o["score"] == sentinel).all())
    if not want_logw:
        assert bool((o["logw"] == sentinel).all())


@pytest.mark.parametrize("n,first", [(260, 0), (1028, 1024)])
def test_fused_tail_variant(hip_ops, oracle_ops, plans, n, first):
    """One pass with a gjx_lse_out: the write-through variant WITH the in-launch fold."""
    hplan, oplan = plans
    check(launch(hip_ops, hplan, n, first, 1, fused=True), oracle_ops, oplan, n, first, 1, what="fused tail")


def test_former_compiler_options_give_the_same_bits(hip_ops, oracle_ops, plans, monkeypatch):
    """GJX_JIT_OPTS=-fslp-vectorize builds the kernels with the option list they had before (another module: the options
    are part of the cache key); packed or not, the arithmetic is the same."""
    _, oplan = plans
    n, first = 1028, 1024
    monkeypatch.setenv("GJX_JIT_OPTS", "-fslp-vectorize")
    c0 = hip_ops.jit_stats()["compiles"]
    hplan = hip_ops.plan_create(W.gaussian10_sites(W.gaussian10_data()))  # (a plan of its own: its slots are built under the option)
    for L in PASSES:
        check(launch(hip_ops, hplan, n, first, L), oracle_ops, oplan, n, first, L, what="former options")
    assert hip_ops.jit_stats()["compiles"] == c0 + 2, "the plain and the write-through variant, compiled under the other options"


def test_store_kind_is_chosen_per_launch(hip_ops):
    """A launch of one pass and a launch of three build two different kernels of the same plan, once each."""
    sites = W.gaussian10_sites(W.gaussian10_data())[:4]
    sites[1].arg[1] = abi.Arg(abi.ARG_CONST, 0, 0.0, 0.4321, None)  # a structure no other test compiles
    plan = hip_ops.plan_create(sites)
    n, L = 256, 3
    vals = [hip_ops.empty((L, n), torch.float32) for _ in range(2)]
    score, logw = hip_ops.empty((L, n), torch.float32), hip_ops.empty((L, n), torch.float32)
    outs = (C.c_void_p * 2)(*[t.data_ptr() for t in vals])
    ins = (C.c_void_p * 1)()
    keys = (abi.Keys * L)(*[hip_ops._keys(keys_of(p, n, 0), n) for p in range(L)])

    def batch():
        hip_ops.lib.call("gjx_importance_run_batch", plan.handle, keys, L, n, 1, ins, 0, outs, 2, hip_ops._p(score), hip_ops._p(logw), n,
                         None, None, None, hip_ops.stream())
        return logw[0].clone()

    def single():
        hip_ops.lib.call("gjx_importance_run", plan.handle, keys, ins, 0, outs, 2, hip_ops._p(score), hip_ops._p(logw), n, None, None, None,
                         None, hip_ops.stream())
        return logw[0].clone()

    c0 = hip_ops.jit_stats()["compiles"]
    a = batch()
    assert hip_ops.jit_stats()["compiles"] == c0 + 1
    b = single()
    assert hip_ops.jit_stats()["compiles"] == c0 + 2, "the one-pass launch takes the write-through variant"
    same(a, b, "pass 0 of three == the single pass")
    batch(), single()
    assert hip_ops.jit_stats()["compiles"] == c0 + 2
