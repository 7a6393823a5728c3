"""Backward-simulation smoothing on the product path (libgjx_hip.so on cuda:0): `BootstrapSMC.backward_simulate` over the
device's own recorded history, held bit for bit (tolerance 0) to the reference tests/backsim_ref.py builds from unchanged
oracle entry points; the oracle's corner cases; that it does what it is for (no genealogy collapse, the RTS smoothing
mean); and its errors."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import backsim_ref as B
import genjax
import guided_ref as G
from genjax import ChoiceMapBuilder as Cm
from genjax._amd import abi, prng, workloads as W
from genjax._amd.runtime import use_ops
from genjax._amd.smc_plan import build_transition_table
from genjax.inference.smc import BootstrapSMC, DiscreteHMM, GuidedSMC, LinearGaussianSSM, StateSpaceModel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_PAR = 5


def _cols(x):
    return list(x) if isinstance(x, tuple) else [x]


def _ref_table(oracle_ops, model, addrs):
    with use_ops(oracle_ops):
        return build_transition_table(StateSpaceModel(*model), addrs)


def _setup(kind, hip_ops, oracle_ops, T):
    """-> (filter factory(n, ess), the oracle-side transition table, observation rows for the reference)."""
    y = W.lgssm_data(T)
    ych = Cm["y"].set(torch.tensor(y))
    if kind == "lgssm_fixed":
        return (lambda n, ess: BootstrapSMC(LinearGaussianSSM(), y, n, ess_threshold=ess, record_history=True),
                _ref_table(oracle_ops, B.lgssm_model(), [("y",)]), None)
    if kind in ("hmm_fixed", "hmm_user"):
        trans, emit = B.hmm_tables(8)
        ys = (np.arange(T) * 3 + 1) % 8
        table = _ref_table(oracle_ops, B.hmm_model(trans, emit), [("x",)])
        if kind == "hmm_fixed":
            return (lambda n, ess: BootstrapSMC(DiscreteHMM(trans, emit, 0), ys.astype(np.int32), n, ess_threshold=ess,
                                                record_history=True), table, None)
        dev = hip_ops.device()
        model = StateSpaceModel(*B.hmm_model(trans.to(dev), emit.to(dev)))
        obs = Cm["x"].set(torch.tensor(ys, dtype=torch.float32))
        return (lambda n, ess: BootstrapSMC(model, obs, n, ess_threshold=ess, record_history=True), table, ys.reshape(T, 1))
    if kind == "guided":
        r = 0.5
        init, step = G.lgssm_model(r)
        tq, sq, _ = G.lgssm_optimal(r, 1.5)  # a non-trivial proposal: it plays no part in the backward weights
        return (lambda n, ess: GuidedSMC(StateSpaceModel(init, step), ych, n, step_proposal=tq, init_proposal=sq,
                                         ess_threshold=ess, record_history=True),
                _ref_table(oracle_ops, (init, step), [("y",)]), y.reshape(T, 1))
    if kind == "increment":
        u = np.linspace(-1.0, 1.0, T).astype(np.float32)
        d = (0.3 * np.cos(np.arange(T))).astype(np.float32)
        obs = Cm["u"].set(torch.tensor(u)) | Cm["d"].set(torch.tensor(d))
        addrs = [a for a, _ in obs.leaves()]
        rows = np.stack([u if a == ("u",) else d for a in addrs], axis=1)
        return (lambda n, ess: BootstrapSMC(StateSpaceModel(*B.increment_model()), obs, n, ess_threshold=ess, record_history=True),
                _ref_table(oracle_ops, B.increment_model(), addrs), rows)
    model = dict(lgssm=B.lgssm_model, two=B.two_component_model, gamma=B.gamma_model)[kind]()
    return (lambda n, ess: BootstrapSMC(StateSpaceModel(*model), ych, n, ess_threshold=ess, record_history=True),
            _ref_table(oracle_ops, model, [("y",)]), y.reshape(T, 1))


def _check(hip_ops, oracle_ops, alg, table, rows, key, key2, m, what):
    with use_ops(hip_ops):
        res = alg.run(key)
        sm = alg.backward_simulate(res, key2, n_paths=m)
    torch.cuda.synchronize()
    hist, lw = [c.cpu() for c in _cols(res.history)], res.log_weight_history.cpu()
    lin, paths = B.backsim_ref(oracle_ops, table, key2, hist, lw, rows, m)
    got_lin, got_paths = sm.lineage.cpu(), [p.cpu() for p in _cols(sm.paths)]
    n = lw.shape[1]
    assert int(got_lin.min()) >= 0 and int(got_lin.max()) < n, what
    differ = int((got_lin != lin).sum())
    print(f"{what}: lineage entries differing {differ} of {lin.numel()}")
    assert torch.equal(got_lin, lin), what
    for a, b in zip(got_paths, paths):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), what
    # the Trajectories fields that are computed from the returned columns
    assert sm.log_weights is None and sm.log_weight_paths is None
    want_unique = torch.tensor([int(torch.unique(lin[t]).numel()) for t in range(lin.shape[0])])
    assert torch.equal(sm.unique_ancestors.cpu(), want_unique), what
    if paths[0].dtype == torch.float32:
        mean = _cols(sm.mean())[0]
        assert torch.allclose(mean, paths[0].double().mean(1), rtol=1e-12, atol=1e-12), what
    return res, sm


# ---- 1. parity, tolerance 0 ----------------------------------------------------------------------------------------------
# (kind, generator, n, m, ESS threshold): every model kind under both generators, every-step and ESS-adaptive filters, n a
# non-multiple of the tile / a tile multiple / several chunks of candidates, m = 1 / a ragged trajectory block / many blocks;
# n m T stays small enough for the CPU reference
CASES = [
    ("lgssm", "philox", 1000, 7, 0.0), ("lgssm", "philox", 4096, 256, 0.0), ("lgssm", "philox", 70_000, 1, 0.5),
    ("lgssm", "threefry", 1000, 7, 0.5), ("lgssm", "threefry", 4096, 1, 0.0),
    ("lgssm_fixed", "philox", 4096, 7, 0.5), ("lgssm_fixed", "threefry", 1000, 1, 0.0),
    ("hmm_fixed", "philox", 1000, 256, 0.0), ("hmm_fixed", "threefry", 4096, 7, 0.5),
    ("hmm_user", "philox", 1000, 7, 0.0), ("hmm_user", "threefry", 1000, 7, 0.0),
    ("two", "philox", 4096, 7, 0.0), ("two", "threefry", 1000, 7, 0.5),
    ("gamma", "philox", 1000, 7, 0.0), ("gamma", "threefry", 1000, 1, 0.0),
    ("increment", "philox", 1000, 7, 0.0), ("increment", "threefry", 1000, 7, 0.0),
    ("guided", "philox", 4096, 7, 0.0), ("guided", "threefry", 1000, 7, 0.5),
]


@pytest.mark.parametrize("kind,impl,n,m,ess", CASES)
def test_parity_with_the_oracle_reference(hip_ops, oracle_ops, kind, impl, n, m, ess):
    make, table, rows = _setup(kind, hip_ops, oracle_ops, T_PAR)
    _check(hip_ops, oracle_ops, make(n, ess), table, rows, genjax.random.key(21, impl), genjax.random.key(22, impl), m,
           f"{kind} {impl} n={n} m={m} ess={ess}")


def test_results_do_not_depend_on_the_grid_or_the_call(hip_ops, oracle_ops):
    make, table, rows = _setup("lgssm", hip_ops, oracle_ops, T_PAR)
    alg = make(70_000, 0.0)
    key2 = genjax.random.key(32, "philox")
    res, sm = _check(hip_ops, oracle_ops, alg, table, rows, genjax.random.key(31, "philox"), key2, 7, "lgssm n=70000 m=7")
    with use_ops(hip_ops):
        assert alg._transition is not None
        plan = alg._transition[0]
        again = alg.backward_simulate(res, key2, n_paths=7)
        assert alg._transition[0] is plan  # built once per filter object
        others = [alg.backward_simulate(res, key2, n_paths=7, max_workgroups=g) for g in (0, 1, 7)]
    torch.cuda.synchronize()
    for o in [again] + others:
        assert torch.equal(o.lineage, sm.lineage) and torch.equal(o.paths.view(torch.int32), sm.paths.view(torch.int32))
    # lineage alone / paths alone through the low-level call
    with use_ops(hip_ops):
        a = hip_ops.backsim_run(plan, key2, [res.history], res.log_weight_history, rows, 7, paths=False)
        b = hip_ops.backsim_run(plan, key2, [res.history], res.log_weight_history, rows, 7, lineage=False)
    assert a["paths"] is None and torch.equal(a["lineage"], sm.lineage)
    assert b["lineage"] is None and torch.equal(b["paths"][0].view(torch.int32), sm.paths.view(torch.int32))


# ---- 2. the oracle's corner cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["threefry", "philox"])
def test_corner_cases_equal_the_oracle(hip_ops, oracle_ops, impl):
    n, m, T = 1000, 7, 7
    g = torch.Generator().manual_seed(5)
    hist = torch.rand(T, n, generator=g) * 2.0 + 0.2  # positive: Gamma states
    lw = torch.randn(T, n, generator=g)
    lw[4] = -float("inf")            # a step whose log-weights are all -inf: index 0
    lw[3, 0] = float("nan")          # a NaN at i = 0 always wins
    lw[2, 1] = float("nan")          # a NaN at i > 0 never wins
    lw[2, 77] = float("nan")
    lw[1, 5] = float("inf")
    hist[6] = -1.0                   # an impossible next state for step 5: every transition density is -inf
    y = np.zeros((T, 1), dtype=np.float32)
    key2 = genjax.random.key(41, impl)
    table = _ref_table(oracle_ops, B.gamma_model(), [("y",)])
    with use_ops(hip_ops):
        plan = hip_ops.backsim_plan_create(build_transition_table(StateSpaceModel(*B.gamma_model()), [("y",)]))
        out = hip_ops.backsim_run(plan, key2, [hist.cuda()], lw.cuda(), y, m)
    torch.cuda.synchronize()
    lin, (paths,) = B.backsim_ref(oracle_ops, table, key2, [hist], lw, y, m)
    got = out["lineage"].cpu()
    assert int(got.min()) >= 0 and int(got.max()) < n
    assert torch.equal(got, lin) and torch.equal(out["paths"][0].cpu().view(torch.int32), paths.view(torch.int32))
    assert bool((lin[4] == 0).all()) and bool((lin[3] == 0).all()) and bool((lin[5] == 0).all())
    assert not bool(((lin[2] == 1) | (lin[2] == 77)).any()) and bool((lin[1] == 5).all())


# ---- 3. it does what it is for ---------------------------------------------------------------------------------------------
def test_backward_simulation_keeps_the_early_steps_alive(hip_ops):
    """LGSSM, T = 100, n = 65 536, m = 1024: more distinct particles at t = 0 than trace-back keeps, and the smoothing mean
    within 4 standard errors of RTS over 8 runs (a filter and a backward pass each).  Both counts and the largest |z| are
    printed; they had not been taken on a GPU when this was written."""
    T, n, m, R = 100, 65_536, 1024, 8
    y = W.lgssm_data(T)
    ms, _ = B.lgssm_rts(y)
    alg = BootstrapSMC(LinearGaussianSSM(), y, n, record_history=True)
    means = []
    with use_ops(hip_ops):
        for r in range(R):  # a run = a filter of its own and a backward pass over it: the spread holds both errors
            res = alg.run(genjax.random.key(50 + r, "philox"))
            sm = alg.backward_simulate(res, genjax.random.key(60 + r, "philox"), n_paths=m)
            means.append(sm.mean().cpu().numpy())
            if r == 0:
                trace = res.trajectories(genjax.random.key(70, "philox"), n_paths=m)
                back0, trace0 = int(sm.unique_ancestors[0]), int(trace.unique_ancestors[0])
    torch.cuda.synchronize()
    print(f"distinct particles at t = 0 among {m} paths: backward simulation {back0}, trace-back {trace0}")
    assert back0 > trace0
    means = np.asarray(means)
    z = (means.mean(0) - ms) / (means.std(0, ddof=1) / np.sqrt(R))
    print("smoothing-mean z-scores against RTS: max |z| =", float(np.abs(z).max()), "at t =", int(np.abs(z).argmax()))
    assert np.all(np.abs(z) <= 4.0), z


# ---- 4. errors -------------------------------------------------------------------------------------------------------------
def test_errors(hip_ops, oracle_ops):
    y = W.lgssm_data(4)
    with use_ops(hip_ops):
        alg = BootstrapSMC(LinearGaussianSSM(), y, 1024)
        res = alg.run(genjax.random.key(1, "philox"))
        with pytest.raises(ValueError, match="record_history"):
            alg.backward_simulate(res, genjax.random.key(2, "philox"), n_paths=4)
        hist = BootstrapSMC(LinearGaussianSSM(), y, 1024, record_history=True)
        res = hist.run(genjax.random.key(1, "philox"))
        plan = hip_ops.backsim_plan_create(hist._bind(hip_ops).transition_table()[0])
        laned_threefry = prng.PRNGKey(1, 2, prng.THREEFRY, lane=3)
        with pytest.raises(abi.GjxError, match="GJX_ERR_INVALID"):  # a THREEFRY key has no lane: nothing is launched
            hip_ops.backsim_run(plan, laned_threefry, [res.history], res.log_weight_history, None, 4)
        with pytest.raises(abi.GjxError, match="GJX_ERR_INVALID"):  # no output at all
            hip_ops.backsim_run(plan, genjax.random.key(2, "philox"), [res.history], res.log_weight_history, None, 4, lineage=False,
                                paths=False)
    torch.cuda.synchronize()
    with use_ops(oracle_ops):
        alg = BootstrapSMC(LinearGaussianSSM(), y, 256, record_history=True)
        res = alg.run(genjax.random.key(1))
        with pytest.raises(abi.BacksimUnavailable):
            alg.backward_simulate(res, genjax.random.key(2), n_paths=4)


JIT_OFF_SCRIPT = """
import sys
sys.path.insert(0, {pkg!r})
import genjax
from genjax._amd import abi, workloads as W
from genjax.inference.smc import BootstrapSMC, LinearGaussianSSM
alg = BootstrapSMC(LinearGaussianSSM(), W.lgssm_data(4), 1024, record_history=True)
res = alg.run(genjax.random.key(1, "philox"))
try:
    alg.backward_simulate(res, genjax.random.key(2, "philox"), n_paths=4)
except abi.GjxError as e:
    print("code", e.code)
"""


def test_without_the_compiler_the_call_is_unsupported(hip_ops):
    env = dict(os.environ, GJX_PLAN_JIT="0")
    r = subprocess.run([sys.executable, "-c", JIT_OFF_SCRIPT.format(pkg=os.path.join(ROOT, "genjax-chi_amd"))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "code -2" in r.stdout, (r.stdout, r.stderr[-2000:])
