"""The Philox round with its three-input XOR as one v_bitop3_b32 (gjx_device.hpp xor3) against the unchanged oracle, bit
for bit (uint32 views: the sign of a zero counts).

Every Philox user shares the round: the generated importance kernels in their three forms (four, two, one particle per
lane), the library's own SMC step and resampler, the scan kernels, key split and fold.  Populations of one particle, a
partial quad, a row less one, one row exactly, a row and one, and four rows and a quad; one pass per launch and three (the
per-pass parent keys)."""

import ctypes as C

import numpy as np
import pytest
import torch

from genjax._amd import abi, prng, workloads as W
from genjax._amd.ops import KeyBatch

pytestmark = pytest.mark.gpu

SEED = 61
POPULATIONS = [1028, 256, 1, 3, 255, 257]  # (the first two let every lane own whole quads: the form asked for is the form built)
PASSES = [1, 3]
FORMS = {"quad": 4, "pair": 2, "one": 1}  # GJX_JIT_FORM -> particles per lane
DTYPES = [torch.float32] * W.G10_LATENTS


def u32(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint64)


def same(a, b, what):
    a, b = u32(a), u32(b)
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {int((a != b).sum()) if a.shape == b.shape else 'shapes'} of {a.size} differ"


def keys_of(p, n):
    return W.importance_particle_keys(prng.key(SEED + p, 1), n, 0)


_REF = {}


def reference(oracle_ops, oplan, p, n):
    """The oracle's pass p over n particles (computed once, shared by the three forms, never modified)."""
    if (p, n) not in _REF:
        vals, score, logw, mp, rows = oracle_ops.importance_run(oplan, keys_of(p, n), n, [], DTYPES, want_rows=True)
        _REF[(p, n)] = dict(values=vals, score=score, logw=logw, row_e=rows.e, row_s=rows.s)
    return _REF[(p, n)]


def launch(ops, plan, n, L):
    """One launch of L passes through the C ABI (L == 1: gjx_importance_run, else gjx_importance_run_batch)."""
    stride, R = -(-n // 256) * 256, ops.num_max_partials(n)
    o = dict(values=[ops.empty((L, stride), torch.float32) for _ in range(W.G10_LATENTS)], score=ops.empty((L, stride), torch.float32),
             logw=ops.empty((L, stride), torch.float32), mp=ops.empty((L, R), torch.float32), row_e=ops.empty((L, R), torch.int32),
             row_s=ops.empty((L, R), torch.int64))
    keys = (abi.Keys * L)(*[ops._keys(keys_of(p, n), n) for p in range(L)])
    ins = (C.c_void_p * 1)()
    outs = (C.c_void_p * W.G10_LATENTS)(*[t.data_ptr() for t in o["values"]])
    tail = (ops._p(o["mp"]), ops._p(o["row_e"]), ops._p(o["row_s"]))
    if L == 1:
        ops.lib.call("gjx_importance_run", plan.handle, keys, ins, 0, outs, W.G10_LATENTS, ops._p(o["score"]), ops._p(o["logw"]), n, *tail,
                     None, ops.stream())
    else:
        ops.lib.call("gjx_importance_run_batch", plan.handle, keys, L, stride, R, ins, 0, outs, W.G10_LATENTS, ops._p(o["score"]),
                     ops._p(o["logw"]), n, *tail, ops.stream())
    return o


@pytest.mark.parametrize("form", list(FORMS))
def test_importance_forms_equal_the_oracle(hip_ops, oracle_ops, form, monkeypatch, capfd):
    monkeypatch.setenv("GJX_JIT_FORM", form)
    monkeypatch.setenv("GJX_PLAN_JIT_VERBOSE", "1")  # (the library names the form of every kernel it builds for a plan)
    sites = W.gaussian10_sites(W.gaussian10_data())
    hplan, oplan = hip_ops.plan_create(sites), oracle_ops.plan_create(sites)  # a plan of its own: its kernels are built under the form
    for n in POPULATIONS:
        for L in PASSES:
            o = launch(hip_ops, hplan, n, L)
            if n == POPULATIONS[0] and L == PASSES[0]:  # the plan's first launch built its kernel
                built = capfd.readouterr().err
                assert f"gjx jit: {FORMS[form]} particle(s) per lane" in built, (form, built[-400:])
            for p in range(L):
                ref, tag = reference(oracle_ops, oplan, p, n), f"{form} n={n} pass {p} of {L}"
                for c in range(W.G10_LATENTS):
                    same(o["values"][c][p, :n], ref["values"][c], f"column {c}, {tag}")
                same(o["score"][p, :n], ref["score"], f"score, {tag}")
                same(o["logw"][p, :n], ref["logw"], f"logw, {tag}")
                same(o["row_e"][p], ref["row_e"], f"row anchors e, {tag}")
                same(o["row_s"][p], ref["row_s"], f"row sums S, {tag}")


def test_lgssm_bootstrap_filter(hip_ops, oracle_ops):
    """The library's own step: the resampler's quad draws (one block per four slots) and the transition draws."""
    h = W.lgssm_smc(hip_ops, 1, seed=SEED, n=1028, T=3, want_ancestors=True)
    o = W.lgssm_smc(oracle_ops, 1, seed=SEED, n=1028, T=3, want_ancestors=True)
    for k in ("ancestors", "out_e", "out_q", "state", "logw"):
        same(h[k], o[k], f"LGSSM filter {k}")
    assert h["log_z"] == o["log_z"]


def test_lgssm_scan(hip_ops, oracle_ops):
    h = W.lgssm_scan(hip_ops, 1, seed=SEED, n=260, T=3)
    o = W.lgssm_scan(oracle_ops, 1, seed=SEED, n=260, T=3)
    for k in ("x", "logw", "score", "carry", "row_e", "row_s"):
        same(h[k], o[k], f"LGSSM scan {k}")
    assert h["log_z"] == o["log_z"]


def _words(k):
    return (k.k0, k.k1, k.lane & 0xFFFFFFFF, k.lane >> 32)


def test_key_split_and_fold_equal_the_host(hip_ops):
    """Five parents against the host derivation (prng.py, pure Python): lane-0 keys (children are lanes: no block), laned keys
    (one block per child), indices beyond 32 bits."""
    k = prng.key(0x1234567890ABCDEF, 1)
    big = (1 << 33) + 5
    parents = [k, prng.split_at(k, 3), prng.fold_in(k, 1), prng.split_at(k, big), prng.split_at(prng.split_at(k, 3), 2)]
    assert [p.lane == 0 for p in parents] == [True, False, True, False, True]
    for parent in parents:
        kb = KeyBatch(1, 1, parent=parent.words(), first=big, parent_lane=parent.lane)
        dev = u32(hip_ops.rng_keys(kb, 6))
        assert np.array_equal(dev, np.array([_words(prng.split_at(parent, big + i)) for i in range(6)], dtype=np.uint32)), parent
        lit = KeyBatch(1, 2, parent=parent.words(), parent_lane=parent.lane)
        assert tuple(u32(hip_ops.rng_keys(lit.with_fold(77), 1))[0]) == _words(prng.fold_in(parent, 77)), parent
        se = u32(hip_ops.rng_split_each(kb, 2, 3)).reshape(2, 3, -1)
        for i in range(2):
            for j in range(3):
                assert tuple(se[i, j]) == _words(prng.split_at(prng.split_at(parent, big + i), j)), (parent, i, j)
