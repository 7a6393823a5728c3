"""The MCMC backward sampler on the product path (libgjx_hip.so on cuda:0): `backward_simulate(..., n_moves=K)` over the
device's own recorded history, held bit for bit (tolerance 0) to the reference tests/backmove_ref.py builds from unchanged
oracle entry points; K = 0 against the trace-back kernel; grid independence; numeric corners; that it does what it is for
(the genealogy's collapse is undone); and its errors."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import backmove_ref as M
import backsim_ref as B
import genjax
from genjax._amd import abi, prng, workloads as W
from genjax._amd.runtime import use_ops
from genjax._amd.smc_plan import build_transition_table
from genjax.inference.smc import BootstrapSMC, LinearGaussianSSM, StateSpaceModel
from test_gpu_backsim import _cols, _ref_table, _setup  # the model kinds of the exact smoother's parity tests

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_PAR = 6


def _check(hip_ops, oracle_ops, alg, table, rows, key, key2, m, K, what):
    with use_ops(hip_ops):
        res = alg.run(key)
        sm = alg.backward_simulate(res, key2, n_paths=m, n_moves=K)
    torch.cuda.synchronize()
    hist, lw, anc = [c.cpu() for c in _cols(res.history)], res.log_weight_history.cpu(), res.ancestors.cpu()
    stats = {}
    lin, paths = M.backmove_ref(oracle_ops, table, key2, hist, lw, anc, rows, m, K, stats)
    got_lin, got_paths = sm.lineage.cpu(), [p.cpu() for p in _cols(sm.paths)]
    n = lw.shape[1]
    assert int(got_lin.min()) >= 0 and int(got_lin.max()) < n, what
    differ = int((got_lin != lin).sum())
    print(f"{what}: lineage entries differing {differ} of {lin.numel()}; the reference accepted {stats['accepted']} of "
          f"{m * K * (lin.shape[0] - 1)} moves")
    assert torch.equal(got_lin, lin), what
    for a, b in zip(got_paths, paths):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), what
    assert sm.log_weights is None and sm.log_weight_paths is None
    want_unique = torch.tensor([int(torch.unique(lin[t]).numel()) for t in range(lin.shape[0])])
    assert torch.equal(sm.unique_ancestors.cpu(), want_unique), what
    return res, sm


# ---- 1. parity, tolerance 0 ----------------------------------------------------------------------------------------------
# (kind, generator, n, m, K, ESS threshold): every model kind under both generators; n below a tile / whole tiles / many
# tiles (the coarse level has 1 / 4 / 69 entries); m = 1 / a ragged wave / more than one workgroup; K = 0, 1, 5, 9 cross the
# blocks of 4 / 2 / 1 moves (1 = 1; 5 = 4 + 1; 9 = 4 + 4 + 1) and 2, 3, 6 the block of two (2; 2 + 1; 4 + 2)
CASES = [
    ("lgssm_fixed", "philox", 1000, 7, 1, 0.0), ("lgssm_fixed", "threefry", 4096, 300, 5, 0.0), ("lgssm_fixed", "philox", 70_000, 300, 9, 0.0),
    ("lgssm_fixed", "philox", 4096, 7, 0, 0.0), ("lgssm_fixed", "philox", 70_000, 1, 5, 0.5),
    ("hmm_fixed", "philox", 1000, 300, 5, 0.0), ("hmm_fixed", "threefry", 4096, 7, 9, 0.0), ("hmm_fixed", "philox", 70_000, 7, 1, 0.0),
    ("lgssm", "philox", 4096, 300, 9, 0.0), ("lgssm", "threefry", 1000, 1, 5, 0.0), ("lgssm", "threefry", 70_000, 7, 2, 0.0),
    ("two", "philox", 1000, 7, 5, 0.0), ("two", "threefry", 4096, 300, 1, 0.0), ("two", "philox", 70_000, 1, 9, 0.0),
    ("gamma", "philox", 4096, 7, 9, 0.0), ("gamma", "threefry", 1000, 300, 3, 0.0),
    ("hmm_user", "philox", 1000, 7, 6, 0.0), ("hmm_user", "threefry", 1000, 300, 1, 0.0),
    ("increment", "philox", 1000, 300, 5, 0.0), ("increment", "threefry", 4096, 7, 9, 0.0),
    ("guided", "philox", 4096, 7, 5, 0.0), ("guided", "threefry", 1000, 300, 0, 0.5),
    ("lgssm", "philox", 1000, 300, 0, 0.0), ("hmm_fixed", "threefry", 1000, 1, 0, 0.0),
]


@pytest.mark.parametrize("kind,impl,n,m,K,ess", CASES)
def test_parity_with_the_oracle_reference(hip_ops, oracle_ops, kind, impl, n, m, K, ess):
    make, table, rows = _setup(kind, hip_ops, oracle_ops, T_PAR)
    _check(hip_ops, oracle_ops, make(n, ess), table, rows, genjax.random.key(21, impl), genjax.random.key(22, impl), m, K,
           f"{kind} {impl} n={n} m={m} K={K} ess={ess}")


@pytest.mark.parametrize("kind,impl,n,m,K", [("lgssm_fixed", "philox", 70_000, 300, 9), ("hmm_fixed", "threefry", 4096, 7, 5)])
def test_parity_of_the_one_level_search(hip_ops, oracle_ops, monkeypatch, kind, impl, n, m, K):
    """GJX_BACKMOVE_SEARCH=plain: the search populations beyond 2^21 particles take, at a size the reference is cheap at."""
    monkeypatch.setenv("GJX_BACKMOVE_SEARCH", "plain")
    make, table, rows = _setup(kind, hip_ops, oracle_ops, T_PAR)
    _check(hip_ops, oracle_ops, make(n, 0.0), table, rows, genjax.random.key(23, impl), genjax.random.key(24, impl), m, K,
           f"plain search: {kind} {impl} n={n} m={m} K={K}")


def test_a_large_shape_in_full(hip_ops, oracle_ops):
    """T = 20, n = m = 300 000, K = 4: 293 coarse entries, m K past 2^20, 1172 workgroups of paths."""
    T = 20
    make, table, rows = _setup("lgssm_fixed", hip_ops, oracle_ops, T)
    _check(hip_ops, oracle_ops, make(300_000, 0.0), table, rows, genjax.random.key(25, "philox"), genjax.random.key(26, "philox"),
           300_000, 4, "lgssm_fixed philox n=m=300000 K=4")


# ---- 2. K = 0 is trace-back; results depend on neither the grid nor the call --------------------------------------------
def test_no_moves_is_the_trace_back_kernel_and_results_do_not_depend_on_the_grid(hip_ops, oracle_ops):
    make, table, rows = _setup("two", hip_ops, oracle_ops, T_PAR)
    alg = make(70_000, 0.0)
    key2 = genjax.random.key(32, "philox")
    with use_ops(hip_ops):
        res = alg.run(genjax.random.key(31, "philox"))
        zero = alg.backward_simulate(res, key2, n_paths=300, n_moves=0)
        traced = hip_ops.paths_trace(res.ancestors, list(res.history), zero.lineage[-1].contiguous())
        assert torch.equal(zero.lineage, traced["lineage"])
        for a, b in zip(zero.paths, traced["paths"]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        sm = alg.backward_simulate(res, key2, n_paths=300, n_moves=5)
        assert torch.equal(sm.lineage[-1], zero.lineage[-1]) and not torch.equal(sm.lineage, zero.lineage)
        plan = alg._transition[0]
        again = alg.backward_simulate(res, key2, n_paths=300, n_moves=5)
        assert alg._transition[0] is plan  # the transition plan is shared with the exact method and built once
        others = [alg.backward_simulate(res, key2, n_paths=300, max_workgroups=g, n_moves=5) for g in (0, 1, 7)]
        for o in [again] + others:
            assert torch.equal(o.lineage, sm.lineage)
            for a, b in zip(o.paths, sm.paths):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        # lineage alone / paths alone (the lineage rows then live in the workspace) through the low-level call
        args = (plan, key2, list(res.history), res.log_weight_history, res.ancestors, rows, 300, 5)
        a = hip_ops.backmove_run(*args, paths=False)
        b = hip_ops.backmove_run(*args, lineage=False)
    torch.cuda.synchronize()
    assert a["paths"] is None and torch.equal(a["lineage"], sm.lineage)
    assert b["lineage"] is None and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(b["paths"], sm.paths))


# ---- 3. numeric corners, against the reference ---------------------------------------------------------------------------
def _low_level(hip_ops, oracle_ops, model, addrs, key2, hist, lw, anc, y, m, K, ref_model=None):
    table = _ref_table(oracle_ops, ref_model or model, addrs)
    with use_ops(hip_ops):
        plan = hip_ops.backsim_plan_create(build_transition_table(StateSpaceModel(*model), addrs))
        out = hip_ops.backmove_run(plan, key2, [h.cuda() for h in hist], lw.cuda(), anc.cuda(), y, m, K)
    torch.cuda.synchronize()
    lin, paths = M.backmove_ref(oracle_ops, table, key2, hist, lw, anc, y, m, K)
    got = out["lineage"].cpu()
    assert int(got.min()) >= 0 and int(got.max()) < lw.shape[1]
    assert torch.equal(got, lin)
    for a, b in zip(out["paths"], paths):
        assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))
    return lin


@pytest.mark.parametrize("impl", ["threefry", "philox"])
def test_corner_cases_equal_the_reference(hip_ops, oracle_ops, impl):
    n, m, T, K = 1000, 70, 7, 5
    g = torch.Generator().manual_seed(5)
    hist = torch.rand(T, n, generator=g) * 2.0 + 0.2  # positive: Gamma states
    lw = torch.randn(T, n, generator=g)
    anc = torch.randint(0, n, (T, n), generator=g, dtype=torch.int32)
    lw[4] = -float("inf")            # a step without any mass: every proposal is what the oracle's multinomial returns for it
    lw[3, 0] = float("nan")          # NaN log-weights
    lw[2, 77] = float("nan")
    hist[6] = -1.0                   # an impossible next state for step 5: every s is -inf, d is NaN, no move is accepted
    anc[3, :50] = -1                 # words that are no index: read as min((uint32) word, n - 1)
    anc[2, 50:90] = n + 7
    y = np.zeros((T, 1), dtype=np.float32)
    key2 = genjax.random.key(41, impl)
    lin = _low_level(hip_ops, oracle_ops, B.gamma_model(), [("y",)], key2, [hist], lw, anc, y, m, K)
    start5 = torch.clamp(anc[6][lin[6].long()].long() & 0xFFFFFFFF, max=n - 1)
    assert torch.equal(lin[5].long(), start5)  # nothing moved at step 5
    # T = 1: the leaves alone;  n = 1: every index is 0
    _low_level(hip_ops, oracle_ops, B.gamma_model(), [("y",)], key2, [hist[:1]], lw[:1], anc[:1], y[:1], m, K)
    one = _low_level(hip_ops, oracle_ops, B.gamma_model(), [("y",)], key2, [hist[:3, :1].contiguous()], lw[:3, :1].contiguous(),
                     torch.zeros((3, 1), dtype=torch.int32), y[:3], m, K)
    assert int(one.abs().max()) == 0


@pytest.mark.parametrize("impl", ["threefry", "philox"])
def test_an_impossible_transition_at_the_start_particle(hip_ops, oracle_ops, impl):
    """An HMM whose transition matrix has -inf logits: where the START particle cannot reach the next state s_cur = -inf, so
    d is +inf (any possible proposal is accepted) or NaN (-inf minus -inf: rejected)."""
    n, m, T, K, S = 1000, 300, 5, 5, 8
    trans, emit = B.hmm_tables(S)
    trans[:4, :4] = -float("inf")
    g = torch.Generator().manual_seed(6)
    hist = torch.randint(0, S, (T, n), generator=g).to(torch.float32)
    lw = torch.randn(T, n, generator=g)
    anc = torch.randint(0, n, (T, n), generator=g, dtype=torch.int32)
    dev = hip_ops.device()
    ys = ((np.arange(T) * 3 + 1) % S).astype(np.float32).reshape(T, 1)
    _low_level(hip_ops, oracle_ops, B.hmm_model(trans.to(dev), emit.to(dev)), [("x",)], genjax.random.key(42, impl), [hist], lw, anc, ys,
               m, K, ref_model=B.hmm_model(trans, emit))


# ---- 4. it does what it is for ---------------------------------------------------------------------------------------------
def test_a_few_moves_undo_the_collapse_of_the_genealogy(hip_ops):
    """LGSSM, T = 50, n = m = 4096: at least four times the distinct particles at t = 0 with K = 2 than with K = 0 (the CPU
    reference: 1 846 against 37).  Both counts are printed."""
    T, n = 50, 4096
    alg = BootstrapSMC(LinearGaussianSSM(), W.lgssm_data(T), n, record_history=True)
    with use_ops(hip_ops):
        res = alg.run(genjax.random.key(50, "philox"))
        u0 = int(alg.backward_simulate(res, genjax.random.key(60, "philox"), n_paths=n, n_moves=0).unique_ancestors[0])
        u2 = int(alg.backward_simulate(res, genjax.random.key(60, "philox"), n_paths=n, n_moves=2).unique_ancestors[0])
    print(f"distinct particles at t = 0 among {n} paths: K = 0 {u0}, K = 2 {u2}")
    assert u2 >= 4 * u0


# ---- 5. errors -------------------------------------------------------------------------------------------------------------
def test_errors(hip_ops, oracle_ops):
    y = W.lgssm_data(4)
    with use_ops(hip_ops):
        alg = BootstrapSMC(LinearGaussianSSM(), y, 1024, record_ancestors=True)
        res = alg.run(genjax.random.key(1, "philox"))
        with pytest.raises(ValueError, match="record_history"):
            alg.backward_simulate(res, genjax.random.key(2, "philox"), n_paths=4, n_moves=2)
        hist = BootstrapSMC(LinearGaussianSSM(), y, 1024, record_history=True)
        res = hist.run(genjax.random.key(1, "philox"))
        for bad in (-1, 257):
            with pytest.raises(ValueError, match="n_moves"):
                hist.backward_simulate(res, genjax.random.key(2, "philox"), n_paths=4, n_moves=bad)
        plan = hip_ops.backsim_plan_create(hist._bind(hip_ops).transition_table()[0])
        args = ([res.history], res.log_weight_history, res.ancestors, None, 4)
        with pytest.raises(abi.GjxError, match="GJX_ERR_INVALID"):  # a THREEFRY key has no lane: nothing is launched
            hip_ops.backmove_run(plan, prng.PRNGKey(1, 2, prng.THREEFRY, lane=3), *args, 2)
        with pytest.raises(abi.GjxError, match="GJX_ERR_INVALID"):  # no output at all
            hip_ops.backmove_run(plan, genjax.random.key(2, "philox"), *args, 2, lineage=False, paths=False)
        with pytest.raises(abi.GjxError, match="GJX_ERR_INVALID"):
            hip_ops.backmove_run(plan, genjax.random.key(2, "philox"), *args, 257)
        with pytest.raises(ValueError, match="same"):
            hip_ops.backmove_run(plan, genjax.random.key(2, "philox"), [res.history], res.log_weight_history, res.ancestors[:3], None, 4, 2)
    torch.cuda.synchronize()
    with use_ops(oracle_ops):
        alg = BootstrapSMC(LinearGaussianSSM(), y, 256, record_history=True)
        res = alg.run(genjax.random.key(1))
        with pytest.raises(abi.BackmoveUnavailable):
            alg.backward_simulate(res, genjax.random.key(2), n_paths=4, n_moves=2)


JIT_OFF_SCRIPT = """
import sys
sys.path.insert(0, {pkg!r})
import genjax
from genjax._amd import abi, workloads as W
from genjax.inference.smc import BootstrapSMC, LinearGaussianSSM
alg = BootstrapSMC(LinearGaussianSSM(), W.lgssm_data(4), 1024, record_history=True)
res = alg.run(genjax.random.key(1, "philox"))
try:
    alg.backward_simulate(res, genjax.random.key(2, "philox"), n_paths=4, n_moves=2)
except abi.GjxError as e:
    print("code", e.code)
"""


def test_without_the_compiler_the_call_is_unsupported(hip_ops):
    env = dict(os.environ, GJX_PLAN_JIT="0")
    r = subprocess.run([sys.executable, "-c", JIT_OFF_SCRIPT.format(pkg=os.path.join(ROOT, "genjax-chi_amd"))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "code -2" in r.stdout, (r.stdout, r.stderr[-2000:])
