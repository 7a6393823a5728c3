"""Shared pieces of the guided-filter tests (test_guided_cpu.py, test_gpu_guided.py): the models and proposals, and the
two per-step references a guided run is held to — both built from the UNCHANGED CPU oracle, which knows no proposed /
guided sites:

 (a) states and ancestors: a *shadow* bootstrap plan (plain gjx_smc_plan_create) whose sites are the proposal's sites as
     latent sites, at the same table positions and with the same state expressions, stepped by the oracle from the
     device's previous population (tile records rebuilt from the device's log-weights with gjx_tile_weights);
 (b) log-weights: recomputed from the device's states, ancestors and observation with the oracle's log-density entry
     points, composed in f32 in the order include/gjx_guided.h fixes:  w = (0 + (lp_x - lq)) + lp_y.
"""

import contextlib
import math

import numpy as np
import torch

from genjax import gen, gamma, normal
from genjax._amd import abi, workloads as W

A, Q = W.LGSSM["a"], W.LGSSM["q"]


def f32(v) -> torch.Tensor:
    return torch.tensor(float(v), dtype=torch.float32)


@contextlib.contextmanager
def lgssm_r(r: float):
    """The project's LGSSM data recipe / Kalman evidence (workloads.lgssm_data, lgssm_exact_log_z) at observation scale r."""
    old = W.LGSSM["r"]
    W.LGSSM["r"] = r
    try:
        yield
    finally:
        W.LGSSM["r"] = old


def lgssm_setting(r: float, T: int):
    """-> (y f32[T], exact log Z) of the LGSSM with a = 0.9, q = 1 and observation scale r."""
    with lgssm_r(r):
        y = W.lgssm_data(T)
        return y, W.lgssm_exact_log_z(y)


def lgssm_model(r: float):
    """The LGSSM as a user model: latents precede the observed site in both bodies."""

    @gen
    def init():
        x = normal(0.0, 1.0) @ "x"
        normal(x, r) @ "y"
        return x

    @gen
    def step(x):
        x2 = normal(A * x, Q) @ "x"
        normal(x2, r) @ "y"
        return x2

    return init, step


def lgssm_transition_proposals():
    """Proposals that repeat the model's latent sites: the guided filter is then the bootstrap filter, bit for bit."""

    @gen
    def track_q(carry, y):
        normal(A * carry, Q) @ "x"

    @gen
    def start_q(y):
        normal(0.0, 1.0) @ "x"

    return track_q, start_q


def lgssm_optimal(r: float, scale_mult: float = 1.0):
    """The locally optimal proposals p(x_t | x_{t-1}, y_t) and p(x_0 | y_0) (`scale_mult` != 1: deliberately mismatched
    scales).  -> (track_q, start_q, coefficients as Python floats)."""
    s2 = 1.0 / (1.0 / Q ** 2 + 1.0 / r ** 2)
    c1, c2, s = s2 * A / Q ** 2, s2 / r ** 2, math.sqrt(s2) * scale_mult
    p0 = 1.0 / (1.0 + 1.0 / r ** 2)
    k0, s0 = p0 / r ** 2, math.sqrt(p0) * scale_mult

    @gen
    def track_q(carry, y):
        normal(c1 * carry + c2 * y, s) @ "x"

    @gen
    def start_q(y):
        normal(k0 * y, s0) @ "x"

    return track_q, start_q, dict(c1=c1, c2=c2, s=s, k0=k0, s0=s0, r=r)


def two_latent_model():
    """Two latents, a two-component carry, latents before the observed site (host_api_cases.case_general_smc's step3)."""

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

    @gen
    def track_q(c, y):  # the model's latent sites, in the model's order
        p, v = c
        v2 = normal(0.9 * v - 0.1 * p, 0.3) @ "v"
        normal(p + 0.5 * v2, 0.2) @ "p"

    @gen
    def start_q(y):
        normal(0.0, 1.0) @ "p"
        normal(0.0, 0.5) @ "v"

    return init, step, track_q, start_q


def gamma_scale_model():
    """A positive scale that drifts, proposed from a Gamma that looks at the observation."""

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

    @gen
    def track_q(g, y):
        gamma(3.0, 3.0 / (0.5 * g + 0.5 * abs(y) + 0.1)) @ "g"

    @gen
    def start_q(y):
        gamma(2.0, 2.0 / (abs(y) + 0.5)) @ "g"

    return init, step, track_q, start_q


def mixed_model():
    """One guided latent ("x") and one that stays prior-drawn ("z")."""

    @gen
    def init():
        x = normal(0.0, 1.0) @ "x"
        z = normal(0.0, 0.3) @ "z"
        normal(x + z, 0.2) @ "y"
        return x, z

    @gen
    def step(c):
        x, z = c
        z2 = normal(0.5 * z, 0.3) @ "z"
        x2 = normal(0.9 * x, 1.0) @ "x"
        normal(x2 + z2, 0.2) @ "y"
        return x2, z2

    @gen
    def track_q(c, y):
        x, z = c
        normal(0.3 * x + 0.7 * y, 0.25) @ "x"

    return init, step, track_q


def modes(table):
    return [int(s.observed) for s in table]


def distinct_parent_share(ancestors: torch.Tensor) -> float:
    """Mean over steps 1 .. T-1 of the number of distinct parents, as a share of n."""
    anc = ancestors.detach().cpu().numpy()
    return float(np.mean([np.unique(anc[t]).size / anc.shape[1] for t in range(1, anc.shape[0])]))


# ---- (a): the shadow bootstrap plan ---------------------------------------------------------------------------------
def shadow_plan(oracle_ops, guided_plan):
    """The proposal's sites of `guided_plan` (an SmcPlan of build_guided_plan) as a plain bootstrap plan on the oracle:
    same table positions, same state expressions, every site latent.  Every draw of the guided step is a draw of this plan."""

    def latent_prefix(table):
        out = []
        for s in table:
            if s.observed != abi.SITE_PROPOSED:
                break
            c = abi.Site.from_buffer_copy(s)
            c.observed = 0
            out.append(c)
        assert out, "the table has no proposal in front"
        return out

    ti, ts = (latent_prefix(t) for t in guided_plan._tables)
    init_state, next_state = guided_plan._state_args
    for args, table in ((init_state, ti), (next_state, ts)):
        for a in args:  # the carry of these models is made of proposed values only
            assert a.kind == abi.ARG_SITE and a.ref < len(table), "state expression outside the proposal's sites"
    plan = oracle_ops.smc_plan_create(ti, ts, init_state, next_state, guided_plan.n_obs)
    plan._keep = guided_plan  # (expression programs the copied sites point into)
    return plan


def oracle_step_from(oracle_ops, shadow, cfg, t, y_t, prev_states, prev_logw, n):
    """One oracle step of the shadow plan from a given previous population -> (new state columns, ancestors int32[n])."""
    out = oracle_ops.smc_pop(n, [torch.float32] * shadow.n_state, False)
    anc = torch.empty(n, dtype=torch.int32)
    prev = None
    e, q = torch.empty(1, dtype=torch.int32), torch.empty(1, dtype=torch.int64)
    if t > 0:
        qw, recs, subs, _ = oracle_ops.tile_weights(prev_logw.contiguous())
        prev = abi.SmcPop()
        keep = [c.contiguous() for c in prev_states]
        for k, c in enumerate(keep):
            prev.state[k] = c.data_ptr()
        prev.qw, prev.recs, prev.subs = qw.data_ptr(), recs.data_ptr(), subs.data_ptr()
        prev._keep = (keep, qw, recs, subs)
    oracle_ops.smc_plan_step(cfg, shadow, t, np.asarray([y_t], dtype=np.float32), prev, out.struct(),
                             e if t > 0 else None, q if t > 0 else None, anc)
    return out.state, anc


# ---- (b): the LGSSM's guided log-weights, recomputed -----------------------------------------------------------------
def lgssm_log_weights(oracle_ops, co: dict, t: int, y_t: float, x: torch.Tensor, x_prev):
    """The log-weights the guided LGSSM step t must have written, from the new states `x`, the resampled ancestors' states
    `x_prev` (None at t = 0) and the observation: every argument in the f32 steps the lowering emits, every log-density by
    the oracle's entry point, then  w = (0 + (lp_x - lq)) + lp_y  in f32."""
    n = x.numel()
    y = f32(y_t)
    zero = f32(0.0)
    if t == 0:
        loc_q, s_q = (f32(co["k0"]) * y + zero).expand(n).contiguous(), co["s0"]
        loc_p, s_p = 0.0, 1.0
    else:
        loc_q, s_q = (x_prev * f32(co["c1"])) + (y * f32(co["c2"])), co["s"]  # `c1 * carry + c2 * y`: a postfix program
        loc_p, s_p = (f32(A) * x_prev) + zero, Q                               # `A * x`: one affine step
    lq = oracle_ops.logpdf("normal", n, x.contiguous(), loc_q, s_q)
    lp = oracle_ops.logpdf("normal", n, x.contiguous(), loc_p, s_p)
    ly = oracle_ops.logpdf("normal", n, float(y), (f32(1.0) * x) + zero, co["r"])
    w = torch.zeros(n, dtype=torch.float32)
    w = w + (lp - lq)
    return w + ly
