"""Guided particle filters on the product path (libgjx_hip.so on cuda:0).  The CPU oracle knows no proposed / guided sites,
so the filter is pinned to it in two steps: with a proposal equal to the model's transition it IS the bootstrap filter
(which the rest of the suite pins to the oracle), bit for bit; with a real proposal every step's draws, resampling and
weights are checked against references built from the unchanged oracle (guided_ref.py).  Then: it does what it is for
(sharp observations), and it has the bootstrap filter's launch structure."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import genjax
import guided_ref as G
from genjax import ChoiceMapBuilder as Cm
from genjax._amd import workloads as W
from genjax._amd.runtime import use_ops
from genjax.inference.smc import BootstrapSMC, GuidedSMC, StateSpaceModel

pytestmark = pytest.mark.gpu
IMPLS = ["threefry", "philox"]


def _cols(x):
    return list(x) if isinstance(x, tuple) else [x]


def _same(g, b, what=""):
    """Every field of two SMCResults, under torch.equal."""
    assert torch.equal(g.log_weights, b.log_weights), f"log-weights {what}"
    for a, c in zip(_cols(g.particles), _cols(b.particles)):
        assert torch.equal(a, c), f"states {what}"
    assert torch.equal(g.ancestors, b.ancestors), f"ancestors {what}"
    assert torch.equal(g.step_e, b.step_e) and torch.equal(g.step_q, b.step_q), f"step_e / step_q {what}"
    assert g.log_marginal_likelihood == b.log_marginal_likelihood, f"log Z {what}"
    assert (g.resampled is None) == (b.resampled is None)
    if g.resampled is not None:
        assert torch.equal(g.resampled, b.resampled), f"resampling flags {what}"
    assert (g.history is None) == (b.history is None)
    if g.history is not None:
        for a, c in zip(_cols(g.history), _cols(b.history)):
            assert torch.equal(a, c), f"state history {what}"
        assert torch.equal(g.log_weight_history, b.log_weight_history), f"log-weight history {what}"


# ---- 1. proposal = transition: the bootstrap filter, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("ess", [0.0, 0.5])
@pytest.mark.parametrize("latents", [1, 2])
def test_transition_proposal_is_the_bootstrap_filter(hip_ops, latents, ess, impl):
    n, T = 20_000, 12
    y = W.lgssm_data(T)
    obs = Cm["y"].set(torch.tensor(y))
    if latents == 1:
        init, step = G.lgssm_model(W.LGSSM["r"])
        tq, sq = G.lgssm_transition_proposals()
    else:
        init, step, tq, sq = G.two_latent_model()
    model = StateSpaceModel(init, step)
    keys = [genjax.random.key(40 + k, impl) for k in range(3)]
    with use_ops(hip_ops):
        for hist in (False, True):
            kw = dict(record_ancestors=True, ess_threshold=ess, record_history=hist)
            guided = GuidedSMC(model, obs, n, step_proposal=tq, init_proposal=sq, **kw)
            boot = BootstrapSMC(model, obs, n, **kw)
            _same(guided.run(keys[0]), boot.run(keys[0]), f"run, history {hist}")
            if not hist:
                gm, bm = guided.run_many(keys), boot.run_many(keys)
                for f in range(3):
                    _same(gm[f], bm[f], f"run_many filter {f}")
                _same(gm[0], guided.run(keys[0]), "run_many[0] against its own run")
        # without an init proposal step 0 is the bootstrap step 0 and the later steps are guided: still the same filter
        g0 = GuidedSMC(model, obs, n, step_proposal=tq, record_ancestors=True, ess_threshold=ess).run(keys[1])
        _same(g0, BootstrapSMC(model, obs, n, record_ancestors=True, ess_threshold=ess).run(keys[1]), "no init proposal")
    torch.cuda.synchronize()


# ---- 2. a real proposal against the unchanged oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("scale_mult", [1.0, 3.0])  # the locally optimal proposal; a deliberately mismatched scale
def test_real_proposal_against_the_oracle(hip_ops, oracle_ops, scale_mult, impl):
    r, n, T = 0.05, 8192, 10
    y, _ = G.lgssm_setting(r, T)
    init, step = G.lgssm_model(r)
    tq, sq, co = G.lgssm_optimal(r, scale_mult)
    key = genjax.random.key(7, impl)
    with use_ops(hip_ops):
        alg = GuidedSMC(StateSpaceModel(init, step), Cm["y"].set(torch.tensor(y)), n, step_proposal=tq, init_proposal=sq,
                        record_history=True)
        res = alg.run(key)
    torch.cuda.synchronize()
    hist, lw, anc = res.history.cpu(), res.log_weight_history.cpu(), res.ancestors.cpu()
    assert bool(torch.isfinite(lw).all()) and math.isfinite(res.log_marginal_likelihood)
    shadow = G.shadow_plan(oracle_ops, alg._plan[0])
    sk, rk = W.smc_key_schedule(key, T)
    cfg = oracle_ops.smc_config(key.impl, n, 0, n, sk, rk, 0.0)
    bad_a, bad_b = [], []
    for t in range(T):
        # (a) the oracle draws and resamples exactly what the device did
        st, a = G.oracle_step_from(oracle_ops, shadow, cfg, t, y[t], [hist[t - 1]] if t else None, lw[t - 1] if t else None, n)
        same_anc = torch.equal(a, anc[t])
        same_x = torch.equal(st[0].view(torch.int32), hist[t].contiguous().view(torch.int32))
        # (b) the weights, from the device's own states and ancestors
        x_prev = hist[t - 1][anc[t].long()].contiguous() if t else None
        want = G.lgssm_log_weights(oracle_ops, co, t, y[t], hist[t].contiguous(), x_prev)
        got = lw[t].contiguous()
        differ = int((want.view(torch.int32) != got.view(torch.int32)).sum())
        print(f"t={t}: ancestors equal {same_anc}, states equal {same_x}, log-weights differing {differ} of {n}, "
              f"max |diff| {float((want - got).abs().max()):.3e}")
        if not (same_anc and same_x):
            bad_a.append(t)
        if differ:
            bad_b.append(t)
    assert not bad_a, f"(a) states / ancestors differ from the oracle's shadow step at steps {bad_a}"
    assert not bad_b, f"(b) log-weights differ from the oracle's log-densities at steps {bad_b}"


# ---- 3. it does what it is for ----------------------------------------------------------------------------------------------
def _sharp_setting():
    r, T, n = 0.05, 50, 8192
    y, exact = G.lgssm_setting(r, T)
    init, step = G.lgssm_model(r)
    tq, sq, _ = G.lgssm_optimal(r)
    return r, T, n, y, exact, StateSpaceModel(init, step), tq, sq


def test_sharp_observations(hip_ops):
    """r = 0.05 against q = 1: the bootstrap filter collapses (a float64 numpy restatement: RMS log Z error 0.43, 9 % distinct
    parents), the filter that proposes from p(x_t | x_{t-1}, y_t) does not (0.0034, 99 %)."""
    r, T, n, y, exact, model, tq, sq = _sharp_setting()
    obs = Cm["y"].set(torch.tensor(y))
    keys = [genjax.random.key(k, "philox") for k in range(8)]
    with use_ops(hip_ops):
        guided = GuidedSMC(model, obs, n, step_proposal=tq, init_proposal=sq, record_ancestors=True).run_many(keys)
        boot = BootstrapSMC(model, obs, n, record_ancestors=True).run_many(keys)
    torch.cuda.synchronize()
    rms = lambda rs: math.sqrt(sum((x.log_marginal_likelihood - exact) ** 2 for x in rs) / len(rs))  # noqa: E731
    share = lambda rs: float(np.mean([G.distinct_parent_share(x.ancestors) for x in rs]))  # noqa: E731
    rg, rb, sg, sb = rms(guided), rms(boot), share(guided), share(boot)
    print(f"exact log Z {exact:.4f}; RMS error guided {rg:.5f} bootstrap {rb:.5f} (ratio {rb / max(rg, 1e-300):.1f}); "
          f"distinct parents guided {sg:.4f} bootstrap {sb:.4f}")
    assert rg <= rb / 10.0
    assert sg > 0.9 and sb < 0.2


# ---- 4. structure -----------------------------------------------------------------------------------------------------------
def _loaded_hip_runtime():
    """The HIP runtime this process already uses (torch's), for hipGraphGetNodes: never a second copy."""
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line:
            return C.CDLL(line.split()[-1])
    pytest.fail("no libamdhip64.so mapped in a process that runs HIP")


def _kernel_nodes(graph_handle) -> int:
    hip = _loaded_hip_runtime()
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(C.c_void_p(graph_handle), None, C.byref(count)) == 0
    nodes = (C.c_void_p * count.value)()
    assert hip.hipGraphGetNodes(C.c_void_p(graph_handle), nodes, C.byref(count)) == 0
    kernels = 0
    for k in range(count.value):
        ty = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(nodes[k]), C.byref(ty)) == 0
        kernels += 1 if ty.value == 0 else 0  # hipGraphNodeTypeKernel
    return kernels


@pytest.mark.parametrize("impl", IMPLS)
def test_one_launch_per_step_and_one_replayed_graph(hip_ops, impl):
    """A whole guided run captured as ONE graph holds T + 1 kernels — the init step, T - 1 resample+propose+weight steps and
    the closing merge — exactly as the bootstrap plan filter's; replayed, it computes the plain run's results.  The library's
    own run-graph cache (gjx_smc_run_graph_stats) treats both plan filters alike."""
    r, T, n, y, exact, model, tq, sq = _sharp_setting()
    T = 20
    y = y[:T]
    obs = Cm["y"].set(torch.tensor(y))
    key = genjax.random.key(5, impl)
    sk, rk = W.smc_key_schedule(key, T)
    counts, deltas = {}, {}
    with use_ops(hip_ops):
        for name, alg in (("guided", GuidedSMC(model, obs, n, step_proposal=tq, init_proposal=sq, record_ancestors=True)),
                          ("bootstrap", BootstrapSMC(model, obs, n, record_ancestors=True))):
            before = hip_ops.smc_run_graph_stats()
            plain = [alg.run(key) for _ in range(3)][-1]  # (compiles at the first run; three runs of one shape)
            after = hip_ops.smc_run_graph_stats()
            deltas[name] = {k: after[k] - before[k] for k in after}
            bound = alg._bind(hip_ops)
            side = torch.cuda.Stream()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(g, stream=side):
                out = hip_ops._smc_run(bound, key.impl, n, sk, rk, True, 0.0)
            counts[name] = _kernel_nodes(g.raw_cuda_graph())
            g.replay()
            torch.cuda.synchronize()
            out_e, out_q, states, logw, anc = out[:5]
            assert torch.equal(out_e, plain.step_e) and torch.equal(out_q, plain.step_q), name
            assert torch.equal(states[0], plain.particles) and torch.equal(logw, plain.log_weights), name
            assert torch.equal(anc, plain.ancestors), name
            del g
    print("kernels per captured run:", counts, " run-graph cache deltas:", deltas)
    assert counts["guided"] == T + 1 and counts["bootstrap"] == T + 1
    assert deltas["guided"] == deltas["bootstrap"]


def test_trajectories_keep_their_ancestry(hip_ops):
    """`trajectories(key)` of a guided history run: the paths still have many distinct ancestors at step 0 where the
    bootstrap filter's have collapsed."""
    r, T, n, y, exact, model, tq, sq = _sharp_setting()
    obs = Cm["y"].set(torch.tensor(y))
    key = genjax.random.key(2, "philox")
    with use_ops(hip_ops):
        g = GuidedSMC(model, obs, n, step_proposal=tq, init_proposal=sq, record_history=True).run(key)
        b = BootstrapSMC(model, obs, n, record_history=True).run(key)
        tg, tb = g.trajectories(genjax.random.key(3, "philox")), b.trajectories(genjax.random.key(3, "philox"))
    ug, ub = tg.unique_ancestors.cpu(), tb.unique_ancestors.cpu()
    print("distinct ancestors at step 0: guided", int(ug[0]), "bootstrap", int(ub[0]), "; at step T-1:", int(ug[-1]), int(ub[-1]))
    assert tg.paths.shape == (T, n) and tg.lineage.shape == (T, n)
    assert int(ug[0]) > int(ub[0])
    mean = tg.mean()
    assert mean.shape == (T,) and bool(torch.isfinite(mean).all())
    # the smoothing mean sits on the sharp observations
    assert float((mean - torch.tensor(y, dtype=torch.float64)).abs().max()) < 5 * r
