"""Posterior predictive draws on the GPU (include/gjx_predictive.h): every stored draw held bit for bit to the replay
tests/predictive_ref.py makes from unchanged oracle entry points, the per-row summaries to float64 numpy reductions of those
draws, NaN draws and an infinite observed value, the stride of the stored subset, held-out rows and new inputs through a
second Target without a second compilation, the closed form of the conjugate regression, and the public call end to end in two
kernel launches."""

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import pointwise_ref as W
import predictive_ref as Q
from genjax import ChoiceMap, Target
from genjax._amd import temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PosteriorPredictive, TemperedSMC
from test_gpu_guided import _kernel_nodes

pytestmark = pytest.mark.gpu

NS = (1, 4, 5, 257)                          # a lone particle; a four-block; a block and a remainder; two chunks
DS = (1, 2, 3, 127, 129, 511, 513, 1025)     # a lone row, a pair, an odd tail, a wave's edge, a tile's edge, three tiles
IMPLS = ("threefry", "philox")


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


def _f32(t):
    return t.detach().to(torch.float32).numpy().copy()


@pytest.fixture(scope="module")
def lowered(hip_ops):
    """Per model: (tracer, plan) lowered once, from 20 rows — the plan knows no length: data of any D is set per case."""
    out = {}
    with use_ops(hip_ops):
        for name in P.MODELS:
            target, _ = P.target(name, 20)
            tracer = temper.lower(target, 64)
            plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            if tracer.params:
                plan.set_params(tracer.params)
            out[name] = (tracer, plan)
    return out


def _case(lowered, oracle_ops, name, impl, D, inf_row=False):
    tracer, plan = lowered[name]
    _, data = P.target(name, max(D, 2), seed=1)
    data = [_f32(t)[:D] for t in data]
    if inf_row:
        data[-1][D // 2] = np.inf
    plan.set_data(_dev(data))
    return plan, Q.Replay(oracle_ops, tracer, data, impl)


def _call(hip_ops, plan, key, cols, stride):
    out, draws = hip_ops.temper_predictive(plan, key, _dev(cols), stride)
    torch.cuda.synchronize()
    return out, draws


def _pin(hip_ops, plan, replay, key, cols, y, case):
    """One population against the replay's draws y [S, D, n]: stride 1, every draw, every count, the moments, twice."""
    n, D, S = len(cols[0]), replay.D, replay.S
    out, draws = _call(hip_ops, plan, key, cols, 1)
    again, draws2 = _call(hip_ops, plan, key, cols, 1)
    assert out.shape == (S, 5, D) and out.dtype == torch.float64 and out.is_cuda, case
    assert draws.shape == (S, n, D) and draws.dtype == torch.float32 and draws.is_cuda, case
    assert torch.equal(out.view(torch.int64), again.view(torch.int64)) and torch.equal(draws.view(torch.int32), draws2.view(torch.int32)), case
    got = draws.cpu().numpy()  # [S, n, D]
    assert Q.same_bits(got, np.transpose(y, (0, 2, 1))), case
    Q.check(out.cpu().numpy(), y, replay.observed(), case)


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", P.MODELS)
def test_predictive_pin(hip_ops, oracle_ops, lowered, name, impl):
    """Every D x n of the grid: one replay of 257 particles per D — particle i's draws are a function of (key, i, x_i), so the
    smaller populations are its prefixes."""
    rng = np.random.default_rng(31)
    key = genjax.random.key(41, impl)
    chunks = set()
    for D in DS:
        plan, replay = _case(lowered, oracle_ops, name, key.impl, D)
        cols = W.centred_columns(name, max(NS), rng)
        y = replay.draws(key, cols)
        assert y.shape == (replay.S, D, max(NS)) and np.isfinite(y).all()
        for n in NS:
            _pin(hip_ops, plan, replay, key, [c[:n].copy() for c in cols], y[:, :, :n], (name, impl, D, n))
            chunks.add(int(hip_ops.lib.call("gjx_predictive_chunks", n, D)))
    assert chunks == {1, 2}


@pytest.mark.parametrize("impl", IMPLS)
def test_predictive_several_chunks(hip_ops, oracle_ops, lowered, impl):
    n, D = 1000, 129
    key = genjax.random.key(42, impl)
    assert int(hip_ops.lib.call("gjx_predictive_chunks", n, D)) == 4
    for name in ("normal", "logistic"):
        plan, replay = _case(lowered, oracle_ops, name, key.impl, D)
        cols = W.centred_columns(name, n, np.random.default_rng(32))
        _pin(hip_ops, plan, replay, key, cols, replay.draws(key, cols), (name, impl, D, n))


def test_predictive_edges(hip_ops, oracle_ops, lowered):
    n, D = 1000, 65
    key = genjax.random.key(43, "philox")
    rng = np.random.default_rng(33)
    # NaN draws: a NaN Gamma latent makes the scale of `hetero` NaN (a negative or zero one still draws a finite value)
    plan, replay = _case(lowered, oracle_ops, "hetero", key.impl, D)
    cols = P.columns("hetero", n, rng, outside=True)
    y = replay.draws(key, cols)
    bad = np.isnan(y[0])
    assert np.array_equal(bad.any(axis=0), np.isnan(cols[1])) and bad.any() and bad.all(axis=0).sum() == np.isnan(cols[1]).sum()
    out, draws = _call(hip_ops, plan, key, cols, 1)
    got = out.cpu().numpy()
    assert Q.same_bits(draws.cpu().numpy(), np.transpose(y, (0, 2, 1)))
    ref = Q.check(got, y, replay.observed(), ("hetero", "outside"))
    k = float(np.isnan(cols[1]).sum())
    assert np.array_equal(got[0, 4], np.full(D, k)) and np.isnan(got[0, 0]).all() and np.isnan(got[0, 1]).all()  # counted, visible
    assert np.all(got[0, 2] + got[0, 3] <= n - k) and np.array_equal(got[0, 2], ref[0, 2])  # absent from below / equal
    # a +inf observed row: every draw that is not NaN lies below it
    plan, replay = _case(lowered, oracle_ops, "hetero", key.impl, D, inf_row=True)
    y = replay.draws(key, cols)
    got = _call(hip_ops, plan, key, cols, 0)[0].cpu().numpy()
    Q.check(got, y, replay.observed(), ("hetero", "inf_row"))
    r = D // 2
    assert replay.observed()[0, r] == np.inf and got[0, 2, r] == n - got[0, 4, r] == n - k and got[0, 3, r] == 0.0


def test_predictive_stride(hip_ops, oracle_ops, lowered):
    n, D, k = 1000, 129, 7
    key = genjax.random.key(44, "philox")
    plan, _ = _case(lowered, oracle_ops, "normal", key.impl, D)
    cols = W.centred_columns("normal", n, np.random.default_rng(34))
    full, every = _call(hip_ops, plan, key, cols, 1)
    out, draws = _call(hip_ops, plan, key, cols, k)
    none, nothing = _call(hip_ops, plan, key, cols, 0)
    assert draws.shape == (1, 143, D) and nothing is None
    assert torch.equal(draws.view(torch.int32), every[:, ::k].contiguous().view(torch.int32))
    assert torch.equal(out.view(torch.int64), full.view(torch.int64)) and torch.equal(none.view(torch.int64), full.view(torch.int64))
    pp = PosteriorPredictive(["y"], out, n, draws, k)
    assert torch.equal(pp.index.cpu(), torch.arange(0, n, k)) and pp.index.dtype == torch.int64 and pp.draws["y"].shape == (143, D)
    # a stride of n or more keeps particle 0 alone
    one = _call(hip_ops, plan, key, cols, 5 * n)[1]
    assert one.shape == (1, 1, D) and torch.equal(one[:, 0].view(torch.int32), every[:, 0].contiguous().view(torch.int32))


def _against_replay(pp, replay, key, cols, k, observed, case):
    y = replay.draws(key, cols)
    n = len(cols[0])
    ref = Q.summarize(y, replay.observed())
    b1, _ = Q.moment_bounds(y)
    for s, a in enumerate(replay.addrs):
        assert Q.same_bits(pp.draws[a].cpu().numpy(), y[s].T[::k]), case
        assert np.all(np.abs(pp.mean[a].cpu().numpy() * n - ref[s, 0]) <= b1[s] + np.abs(ref[s, 0]) * 2.0 ** -51), case
        assert np.allclose(pp.var[a].cpu().numpy(), y[s].astype(np.float64).var(axis=1, ddof=1), rtol=1e-9, atol=0), case
        assert np.array_equal(pp.nan_count[a].cpu().numpy(), ref[s, 4]), case
        if observed:
            assert np.array_equal(pp.below[a].cpu().numpy(), ref[s, 2]) and np.array_equal(pp.equal[a].cpu().numpy(), ref[s, 3]), case
            # (the device divides by n through its reciprocal: two roundings against numpy's one)
            assert np.allclose(pp.pit[a].cpu().numpy(), (ref[s, 2] + 0.5 * ref[s, 3]) / n, rtol=2.0 ** -51, atol=0), case


@pytest.mark.parametrize("name", ["normal", "logistic"])
def test_held_out_and_new_inputs(hip_ops, oracle_ops, name):
    """Columns and a second Target of 65 other rows, then the same inputs with nothing observed: the results are the replay's
    on those rows, and the kernel comes out of the JIT cache."""
    n, k = 300, 4
    key = genjax.random.key(45, "philox")
    cols = W.centred_columns(name, n, np.random.default_rng(35))
    with use_ops(hip_ops):
        train, _ = P.target(name, 40, seed=2)
        alg = TemperedSMC(train, n)
        first = alg.predictive(_dev(cols), key, draw_stride=k)
        assert first.mean["y"].shape == (40,) and first.draws["y"].shape == (75, 40)
        before = hip_ops.jit_stats()["compiles"]
        held, data = P.target(name, 65, seed=7)
        pp = alg.predictive(_dev(cols), key, target=held, draw_stride=k)
        new = alg.predictive(_dev(cols), key, args=held.args, draw_stride=k)
        assert hip_ops.jit_stats()["compiles"] == before
        tracer = temper.lower(held, 64)
    assert isinstance(pp, PosteriorPredictive) and pp.n == n and pp.addresses == ["y"] and pp.mean["y"].shape == (65,)
    replay = Q.Replay(oracle_ops, tracer, [_f32(c) for c in data], key.impl)
    _against_replay(pp, replay, key, cols, k, True, (name, "held out"))
    assert new.pit is None and new.below is None and new.equal is None and new.mean["y"].shape == (65,)
    _against_replay(new, replay, key, cols, k, False, (name, "new inputs"))
    for f in ("mean", "var", "nan_count"):  # nothing observed changes no draw
        assert torch.equal(getattr(new, f)["y"], getattr(pp, f)["y"])
    assert torch.equal(new.draws["y"], pp.draws["y"]) and torch.equal(new.index, pp.index)


def test_closed_form(hip_ops):
    """n = 8192 columns from the exact posterior of the conjugate regression with 500 rows: the predictive mean, the
    predictive variance and the uniformity of the PIT values within FOUR TIMES the spreads predictive_ref records."""
    model = P.conjugate(500)
    n = 8192
    cols = W.posterior_columns(model, n, 9000)
    xs, ys = torch.tensor(model.xs, dtype=torch.float32), torch.tensor(model.ys, dtype=torch.float32)
    target = Target(P.bodies()["normal"], (xs, model.noise), ChoiceMap.d({"y": ys}))
    with use_ops(hip_ops):
        pp = TemperedSMC(target, n).predictive(_dev(cols), genjax.random.key(46, "philox"))
    e = Q.errors_of(model, n, pp.mean["y"].cpu().numpy(), pp.var["y"].cpu().numpy(), pp.pit["y"].cpu().numpy())
    print("closed form: mean, var, pit errors", e, "spreads", (Q.SPREAD_MEAN, Q.SPREAD_VAR, Q.SPREAD_PIT), "factor", Q.CLOSED_FORM_FACTOR)
    assert e[0] <= Q.CLOSED_FORM_FACTOR * Q.SPREAD_MEAN and e[1] <= Q.CLOSED_FORM_FACTOR * Q.SPREAD_VAR
    assert e[2] <= Q.CLOSED_FORM_FACTOR * Q.SPREAD_PIT
    assert pp.draws is None and pp.index is None and torch.equal(pp.nan_count["y"], torch.zeros(500, dtype=torch.float64, device="cuda"))


def test_end_to_end_api(hip_ops):
    """TemperedSMC over the plated regression, then predictive(res, key, n_draws=64): shapes and dtypes, and exactly two
    kernel nodes per call."""
    D, n = 100, 4096
    target, _ = P.target("normal", D, seed=3)
    key = genjax.random.key(47, "philox")
    with use_ops(hip_ops):
        alg = TemperedSMC(target, n, n_moves=2)
        res = alg.run(genjax.random.key(11, "philox"))
        pp = alg.predictive(res, key, n_draws=64)
        assert pp.draws["y"].shape == (64, D) and pp.draws["y"].dtype == torch.float32 and pp.draws["y"].is_cuda
        assert torch.equal(pp.index.cpu(), torch.arange(0, n, 64)) and pp.index.dtype == torch.int64
        for f in (pp.mean, pp.var, pp.pit, pp.below, pp.equal, pp.nan_count):
            assert list(f) == ["y"] and f["y"].shape == (D,) and f["y"].dtype == torch.float64 and f["y"].is_cuda
        assert torch.equal(pp.nan_count["y"], torch.zeros_like(pp.nan_count["y"])) and bool((pp.var["y"] > 0).all())
        assert bool(((pp.pit["y"] >= 0) & (pp.pit["y"] <= 1)).all())
        assert alg.predictive(res, key, n_draws=100).draws["y"].shape == (100, D)  # stride 41: ceil(4096 / 41) rows
        assert torch.equal(alg.predictive(res.columns, key, draw_stride=64).draws["y"], pp.draws["y"])  # a list of columns is the same call
        # the call's launches, counted by graph capture (compiled above: nothing compiles inside the capture)
        plan = alg._state()["tplan"]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g, stream=side):
            out, draws = hip_ops.temper_predictive(plan, key, res.columns, 64)
        nodes = _kernel_nodes(g.raw_cuda_graph())
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(draws[0], pp.draws["y"]) and torch.equal(out[0, 0] / n, pp.mean["y"])
        del g, out, draws
    assert nodes == 2
