"""One plated tempered plan, every generated kernel: the move, the covariance move, the pointwise kernel and the predictive
kernel of ONE plan object run in turn under both generators, each held to the check its own suite applies (test_gpu_plate,
test_gpu_temper_cov, test_gpu_pointwise, test_gpu_predictive) — a plan's kernels live in slots of one table, and a slot, an
entry name or an option list taken for another's shows here."""

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import pointwise_ref as W
import predictive_ref as Q
import temper_cov_ref as V
import temper_ref as R
from genjax._amd import temper
from genjax._amd.runtime import use_ops
from test_gpu_plate import SCALES, _dev, _equal, _f32
from test_gpu_pointwise import _check
from test_gpu_predictive import _pin

pytestmark = pytest.mark.gpu

# two chunks of particles, one particle left after the blocks of four, two workgroups in the move; an odd row count (the last
# predictive lane has row A alone)
N, D, K, BETA = 301, 5, 3, 0.37


def test_one_plan_every_slot(hip_ops, oracle_ops):
    name = "normal"
    with use_ops(hip_ops):
        tracer = temper.lower(P.target(name, 20)[0], 64)
        plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
    assert plan.n_latents == 2
    if tracer.params:
        plan.set_params(tracer.params)
    data = [_f32(t)[:D] for t in P.target(name, D, seed=1)[1]]
    plan.set_data(_dev(data))
    assert int(hip_ops.lib.call("gjx_pointwise_chunks", N, D)) == 2 and int(hip_ops.lib.call("gjx_predictive_chunks", N, D)) == 2
    rng = np.random.default_rng(77)
    cols = W.centred_columns(name, N, rng)
    F = (0.3 * V.pack(np.tril(np.random.default_rng(40).standard_normal((2, 2))))).astype(np.float32)
    assess = {impl: P.Assess(oracle_ops, tracer, data, impl) for impl in (0, 1)}
    lp0, ll0 = assess[1](cols)  # (no draw is made: one start for both generators)
    start = (_dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda())

    def move(impl):
        key = genjax.random.key(1000 + impl, "philox" if impl else "threefry")
        ref = R.move_ref(oracle_ops, assess[impl], key, cols, lp0, ll0, BETA, K, SCALES[name])
        assert 0 < int(ref[3].sum()) < N * K
        return ref, hip_ops.temper_move(plan, key, *start, BETA, K, SCALES[name])

    def move_cov(impl):
        key = genjax.random.key(2000 + impl, "philox" if impl else "threefry")
        ref = V.move_cov_ref(oracle_ops, assess[impl], key, cols, lp0, ll0, BETA, K, F)
        assert 0 < int(ref[3].sum()) < N * K
        return ref, hip_ops.temper_move_cov(plan, key, *start, BETA, K, torch.from_numpy(F).cuda())

    def pinned(what, ref, got):
        x, lp, ll, acc = got
        assert np.array_equal(acc.cpu().numpy(), ref[3]), what
        assert all(_equal(a.cpu().numpy(), b) for a, b in zip(x, ref[0])), what
        assert _equal(lp.cpu().numpy(), ref[1]) and _equal(ll.cpu().numpy(), ref[2]), what

    def pointwise():
        t = W.terms(assess[1], cols)
        assert t.shape == (D, N) and np.isfinite(t).all()
        out = hip_ops.temper_pointwise(plan, start[0])
        assert out.shape == (4, D) and out.dtype == torch.float64
        _check(out.cpu().numpy(), t, ("pointwise", D, N))

    def predictive(impl):
        key = genjax.random.key(41, impl)
        replay = Q.Replay(oracle_ops, tracer, data, key.impl)
        _pin(hip_ops, plan, replay, key, cols, replay.draws(key, cols), ("predictive", impl, D, N))

    pinned("move, philox", *move(1))
    pinned("covariance move, threefry", *move_cov(0))
    pointwise()
    predictive("threefry")
    predictive("philox")
    pinned("move, threefry", *move(0))
    pinned("covariance move, philox", *move_cov(1))
    plan.__del__()  # gjx_temper_plan_destroy walks every slot
    assert plan.handle is None
