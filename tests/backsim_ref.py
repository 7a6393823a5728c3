"""Shared pieces of the backward-simulation tests (test_backsim_cpu.py, test_gpu_backsim.py): the models, and the
reference a smoother run is held to — built from UNCHANGED oracle entry points (the oracle knows no gjx_backsim.h):

  * the transition sum s over all candidates of one step and one trajectory is the LOG-WEIGHT COLUMN of an oracle
    importance plan: the transition table's sites as observed sites, the step's state columns as GJX_ARG_INPUT columns,
    the trajectory's next-state values and the observation row as launch parameters (GJX_ARG_PARAM);
  * the logit is a numpy f32 add, lw[t] + s (lw[T-1] itself at the last step);
  * the draw is the oracle's gjx_categorical_index (mode 0) under the lazy key {mode 1, parent fold_in(key, t), first j}.

No m x n array exists beyond one row at a time."""

import numpy as np
import torch

from genjax import categorical, gamma, gen, normal
from genjax._amd import abi, prng, workloads as W
from genjax._amd.ops import KeyBatch

A, Q, R = W.LGSSM["a"], W.LGSSM["q"], W.LGSSM["r"]


# ---- models ----------------------------------------------------------------------------------------------------------
def lgssm_model():
    """The LinearGaussianSSM defaults as a user model."""

    @gen
    def init():
        x = normal(W.LGSSM["x0_loc"], W.LGSSM["x0_scale"]) @ "x"
        normal(x, R) @ "y"
        return x

    @gen
    def step(x):
        x2 = normal(A * x, Q) @ "x"
        normal(x2, R) @ "y"
        return x2

    return init, step


def two_component_model():
    """A two-component carry; the second site's location reads the first site's value."""

    @gen
    def init():
        p = normal(0.0, 1.0) @ "p"
        v = normal(0.0, 0.5) @ "v"
        normal(p, 0.6) @ "y"
        return p, v

    @gen
    def step(c):
        p, v = c
        v2 = normal(0.9 * v - 0.1 * p, 0.3) @ "v"
        p2 = normal(p + 0.5 * v2, 0.2) @ "p"
        normal(p2, 0.6) @ "y"
        return p2, v2

    return init, step


def gamma_model():
    """A positive scale that drifts: a Gamma carry."""

    @gen
    def init():
        g = gamma(2.0, 2.0) @ "g"
        normal(0.0, g) @ "y"
        return g

    @gen
    def step(g):
        g2 = gamma(4.0, 4.0 / g) @ "g"
        normal(0.0, g2) @ "y"
        return g2

    return init, step


def hmm_tables(K=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    trans = torch.randn(K, K, generator=g) * 1.5
    emit = torch.randn(K, K, generator=g) * 1.5
    return trans, emit


def hmm_model(trans, emit, init_state=0):
    """A user-written K-state HMM as DiscreteHMM states it (`init_state` is z_-1: z_0 is drawn from its row): categorical
    rows chosen by the carried state / the new state.  `trans`, `emit`: tensors on the device of the ops the model is
    lowered under."""
    start = trans[init_state].clone()

    @gen
    def init():
        z = categorical(logits=start) @ "z"
        categorical(logits=emit[z]) @ "x"
        return z

    @gen
    def step(z):
        z2 = categorical(logits=trans[z]) @ "z"
        categorical(logits=emit[z2]) @ "x"
        return z2

    return init, step


def increment_model():
    """Observed sites of three kinds: "u" reads nothing of the old state (dropped, and it sits in front of the latents, so
    later site references move), "d" is an observed INCREMENT and reads the old state (kept)."""

    @gen
    def init():
        normal(0.0, 2.0) @ "u"
        p = normal(0.0, 1.0) @ "p"
        v = normal(0.0, 0.5) @ "v"
        normal(p, 0.4) @ "d"
        return p, v

    @gen
    def step(c):
        p, v = c
        normal(0.0, 2.0) @ "u"
        v2 = normal(0.9 * v, 0.3) @ "v"
        p2 = normal(p + 0.5 * v2, 0.2) @ "p"
        normal(p2 - p, 0.4) @ "d"
        return p2, v2

    return init, step


def track_model():
    """The README's constant-velocity tracker: the carry is `p + 0.5 * v2`, a function of the draw — a degenerate transition."""

    @gen
    def init():
        p = normal(0.0, 1.0) @ "p"
        v = normal(0.0, 0.5) @ "v"
        normal(p, 0.6) @ "y"
        return p, v

    @gen
    def step(c):
        p, v = c
        v2 = normal(0.9 * v, 0.3) @ "v"
        normal(p + 0.5 * v2, 0.6) @ "y"
        return p + 0.5 * v2, v2

    return init, step


def arg_fields(a):
    return (int(a.kind), int(a.ref), float(a.scale), float(a.offset))


def site_fields(s):
    """What two tables must share to be the same table (device pointers aside)."""
    two = s.dist not in (abi.DIST_BERNOULLI, abi.DIST_CATEGORICAL)
    return (int(s.dist), int(s.observed), int(s.out_col), int(s.n_cat), int(s.n_rows), int(s.cat_mode), arg_fields(s.arg[0]),
            arg_fields(s.arg[1]) if two else None, arg_fields(s.obs))


# ---- the reference -----------------------------------------------------------------------------------------------------
def _as_importance_arg(table, a, keep):
    """An argument of a transition table as the oracle's importance plan reads it: the state is an input column, next-state
    components are parameters 0 .. n_state - 1, observations the parameters behind them."""
    D = table.n_state
    if a.kind == abi.ARG_STATE:
        return abi.Arg(abi.ARG_INPUT, a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_OBS:
        return abi.Arg(abi.ARG_PARAM, D + a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_NEXT:
        return abi.Arg(abi.ARG_PARAM, a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_EXPR:
        ops = (abi.ExprOp * a.ref).from_address(a.table)
        swap = {abi.EXPR_STATE: (abi.EXPR_INPUT, 0), abi.EXPR_OBS: (abi.EXPR_PARAM, D)}
        prog = [(swap[o.op][0], o.ref + swap[o.op][1], o.value) if o.op in swap else (o.op, o.ref, o.value) for o in ops]
        return abi.expr_arg(prog, keep)
    return abi.Arg(a.kind, a.ref, a.scale, a.offset, a.table)


def transition_importance_plan(oracle_ops, table):
    """-> the oracle importance plan whose log-weight column is the transition sum s.  `table`: a TransitionTable whose
    device tables (categorical logits) are CPU tensors — lower the model under the oracle's ops."""
    keep, sites = [], []
    for s in table.sites:
        c = abi.Site.from_buffer_copy(s)
        c.arg[0] = _as_importance_arg(table, s.arg[0], keep)
        c.arg[1] = _as_importance_arg(table, s.arg[1], keep)
        c.obs = _as_importance_arg(table, s.obs, keep)
        c.observed, c.out_col = 1, -1
        sites.append(c)
    plan = oracle_ops.plan_create(sites)
    plan._keep = (keep, table)
    return plan


def backsim_ref(oracle_ops, table, key, cols, lw, obs, m):
    """The specification of include/gjx_backsim.h from oracle pieces.  `cols`: CPU [T, n] tensors (float32, or int32 for the
    fixed HMM's states), `lw` f32[T, n], `obs` [T, n_obs] or None.  -> (lineage int32[T, m], [path columns [T, m]])."""
    T, n = lw.shape
    D = table.n_state
    plan = transition_importance_plan(oracle_ops, table) if T > 1 else None
    lwn = lw.detach().cpu().numpy().astype(np.float32)
    cols = [c.detach().cpu() for c in cols]
    fcols = [c.to(torch.float32) for c in cols]  # (the kernel reads an int32 column as (float) value)
    obs = None if obs is None else np.asarray(obs, dtype=np.float32).reshape(T, -1)
    lineage = torch.empty((T, m), dtype=torch.int32)
    kb_unused = prng.split_lazy(prng.key(0, key.impl), n)  # (the plan has no latent site: no draw is made)
    for t in range(T - 1, -1, -1):
        kt = prng.fold_in(key, t)
        ins = [c[t].contiguous() for c in fcols]
        cache = {}
        for j in range(m):
            if t == T - 1:
                logit = lwn[t]
            else:
                w = int(lineage[t + 1, j])
                params = np.asarray([float(c[t + 1, w]) for c in fcols] + ([] if obs is None else list(obs[t + 1])), dtype=np.float32)
                s = cache.get(params.tobytes())
                if s is None:
                    plan.set_params(params)
                    s = oracle_ops.importance_run(plan, kb_unused, n, ins, [], want_score=False, want_max_partials=False)[2].numpy().copy()
                    if len(cache) < 64:
                        cache[params.tobytes()] = s
                logit = lwn[t] + s  # f32 + f32: one rounding
            kb = KeyBatch(key.impl, 1, parent=(kt.k0, kt.k1), first=j, parent_lane=kt.lane)
            lineage[t, j] = int(oracle_ops.categorical_index(kb, torch.from_numpy(np.ascontiguousarray(logit)), 0))
    idx = lineage.long()
    return lineage, [torch.gather(c, 1, idx) for c in cols]


# ---- exact smoothers ---------------------------------------------------------------------------------------------------
def lgssm_rts(y):
    """float64 Kalman filter + Rauch-Tung-Striebel smoother of the LinearGaussianSSM defaults -> (mean[T], var[T])."""
    y = np.asarray(y, dtype=np.float64)
    T = y.size
    a, q2, r2 = A, Q * Q, R * R
    mf, pf, mp, pp = np.empty(T), np.empty(T), np.empty(T), np.empty(T)
    m_pred, p_pred = W.LGSSM["x0_loc"], W.LGSSM["x0_scale"] ** 2
    for t in range(T):
        if t > 0:
            m_pred, p_pred = a * mf[t - 1], a * a * pf[t - 1] + q2
        mp[t], pp[t] = m_pred, p_pred
        k = p_pred / (p_pred + r2)
        mf[t], pf[t] = m_pred + k * (y[t] - m_pred), (1.0 - k) * p_pred
    ms, ps = mf.copy(), pf.copy()
    for t in range(T - 2, -1, -1):
        g = pf[t] * a / pp[t + 1]
        ms[t] = mf[t] + g * (ms[t + 1] - mp[t + 1])
        ps[t] = pf[t] + g * g * (ps[t + 1] - pp[t + 1])
    return ms, ps


def hmm_marginals(trans, emit, init_state, y):
    """float64 forward-backward of the K-state HMM (z_0 is drawn from row `init_state`: gjx.h gjx_hmm) -> P(z_t = k | y)[T, K]."""
    lt = torch.log_softmax(trans.double(), 1).numpy()
    le = torch.log_softmax(emit.double(), 1).numpy()
    T, K = len(y), lt.shape[0]
    al = np.full((T, K), -np.inf)
    al[0] = lt[init_state] + le[:, y[0]]
    for t in range(1, T):
        al[t] = np.logaddexp.reduce(al[t - 1][:, None] + lt, axis=0) + le[:, y[t]]
    be = np.zeros((T, K))
    for t in range(T - 2, -1, -1):
        be[t] = np.logaddexp.reduce(lt + (le[:, y[t + 1]] + be[t + 1])[None, :], axis=1)
    g = al + be
    g -= np.logaddexp.reduce(g, axis=1, keepdims=True)
    return np.exp(g)
