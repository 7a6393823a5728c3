"""Bootstrap-filter models bound to an `Ops`, one class per kind the library has a step for (the hand-written
linear-Gaussian model, the hand-written discrete HMM, a generated plan): the one place that knows how a kind maps onto
the C ABI (include/gjx.h) — model argument, observation dtype, state columns, `gjx_smc_*` symbols, the tables that
travel with them.  The drivers (the whole-run call of `Ops`, the stepwise history filter of smc_fused.py, the sharded
filters of dist.py) are written once against `state_dtypes`, `y` (host observations as the ABI takes them), `T` and

    run(cfg, outputs)                                     gjx_smc_run_*            (outputs: Ops._smc_buffers)
    step(cfg, t, prev, out, prev_e, prev_q, ancestors)    gjx_smc_*_step
    sharded_run(comm, cfg, io)                            gjx_smc_sharded_run_*
    transition_table()                                    f(x_t+1 | x_t) as a site table (include/gjx_backsim.h;
                                                          smc_plan.TransitionTable) and the observation rows that go with it"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from . import abi


class LgssmFilter:
    state_dtypes = [torch.float32]
    workspace_per_filter = True  # F filters in one call: F workspaces of one filter (Ops._smc_buffers)

    def __init__(self, ops, model: abi.Lgssm, y):
        self.ops, self.model = ops, model
        self.y = np.ascontiguousarray(np.asarray(y, dtype=np.float32))  # [T]
        self.T = self.y.size

    def run(self, cfg, outputs):
        o = self.ops
        out_e, out_q, (x,), logw, anc, ws, nb = outputs
        o.lib.call("gjx_smc_run_lgssm", C.byref(cfg), C.byref(self.model), C.c_void_p(self.y.ctypes.data), o._p(out_e),
                   o._p(out_q), o._p(x), o._p(logw), o._p(anc), o._p(ws), nb, o.stream())

    def step(self, cfg, t, prev, out, prev_e, prev_q, ancestors):
        self.ops.smc_lgssm_step(cfg, self.model, t, float(self.y[t]), prev, out, prev_e, prev_q, ancestors)

    def transition_table(self):
        """`normal(a * x, q) @ "x"` constrained to the next state: what a user-written LGSSM lowers to."""
        from .smc_plan import TransitionTable

        site = abi.Site()
        site.dist, site.observed, site.out_col = abi.DIST_NORMAL, 1, -1
        site.arg[0] = abi.Arg(abi.ARG_STATE, 0, self.model.a, 0.0, None)
        site.arg[1] = abi.Arg(abi.ARG_CONST, 0, 0.0, self.model.q, None)
        site.obs = abi.Arg(abi.ARG_NEXT, 0, 1.0, 0.0, None)
        return TransitionTable([site], 1, 0), None

    def sharded_run(self, comm, cfg, io):
        self.ops.lib.call("gjx_smc_sharded_run_lgssm", comm.handle, C.byref(cfg), C.byref(self.model),
                          C.c_void_p(self.y.ctypes.data), C.byref(io), self.ops.stream())


class HmmFilter:
    state_dtypes = [torch.int32]
    workspace_per_filter = True

    def __init__(self, ops, n_states: int, init_state: int, trans_logits: torch.Tensor, obs_logits: torch.Tensor, y):
        """`trans_logits` / `obs_logits`: f32[K, K] on the device (the abi.Hmm keeps them alive)."""
        self.ops, self.model = ops, ops.hmm_model(n_states, init_state, trans_logits, obs_logits)
        self.y = np.ascontiguousarray(np.asarray(y, dtype=np.int32))  # [T]
        self.T = self.y.size

    @functools.cached_property
    def tables(self):
        """gjx_hmm_prepare's (alias table, observation log-probabilities), made when a step-level or sharded driver first asks
        (the whole-run call prepares its own inside the library)."""
        return self.ops.hmm_prepare_model(self.model)

    def run(self, cfg, outputs):
        o = self.ops
        out_e, out_q, (z,), logw, anc, ws, nb = outputs
        o.lib.call("gjx_smc_run_hmm", C.byref(cfg), C.byref(self.model), C.c_void_p(self.y.ctypes.data), o._p(out_e),
                   o._p(out_q), o._p(z), o._p(logw), o._p(anc), o._p(ws), nb, o.stream())

    def step(self, cfg, t, prev, out, prev_e, prev_q, ancestors):
        alias, logp = self.tables
        self.ops.smc_hmm_step(cfg, self.model, t, int(self.y[t]), prev, out, alias, logp, prev_e, prev_q, ancestors)

    def transition_table(self):
        """`categorical(logits=T[z]) @ "z"` constrained to the next state: row = the state, value = the next one (the generated
        kernel reads the transposed log-probability table the plan machinery derives for such a site)."""
        from .smc_plan import TransitionTable

        K = int(self.model.n_states)
        site = abi.Site()
        site.dist, site.observed, site.out_col = abi.DIST_CATEGORICAL, 1, -1
        site.n_cat, site.n_rows, site.cat_mode = K, K, 0
        site.arg[0] = abi.Arg(abi.ARG_STATE, 0, 1.0, 0.0, None)
        site.obs = abi.Arg(abi.ARG_NEXT, 0, 1.0, 0.0, None)
        site.logits = self.model.trans_logits
        return TransitionTable([site], 1, 0, (self.model,)), None

    def sharded_run(self, comm, cfg, io):
        o = self.ops
        alias, logp = self.tables
        o.lib.call("gjx_smc_sharded_run_hmm", comm.handle, C.byref(cfg), C.byref(self.model),
                   C.c_void_p(self.y.ctypes.data), o._p(alias), o._p(logp), C.byref(io), o.stream())


class PlanFilter:
    workspace_per_filter = False  # F filters in one call: one workspace of F * stride particles

    def __init__(self, ops, plan, obs, source=None):
        """`plan`: an SmcPlan (Ops.smc_plan_create); `obs`: the [T, n_obs] observation constants ([T] for a plan without);
        `source`: (StateSpaceModel, observed addresses) the plan was lowered from — what `transition_table` lowers again."""
        self.ops, self.plan, self.state_dtypes = ops, plan, [torch.float32] * plan.n_state
        self.source = source
        self.y = np.ascontiguousarray(np.asarray(obs, dtype=np.float32).reshape(-1, max(plan.n_obs, 1))[:, :plan.n_obs])
        self.T = len(self.y)
        self._obs = C.c_void_p(self.y.ctypes.data) if plan.n_obs else None

    def run(self, cfg, outputs):
        o = self.ops
        out_e, out_q, states, logw, anc, ws, nb = outputs
        cols = (C.c_void_p * len(states))(*[c.data_ptr() for c in states])
        o.lib.call("gjx_smc_run_plan", C.byref(cfg), self.plan.handle, self._obs, o._p(out_e), o._p(out_q), cols,
                   o._p(logw), o._p(anc), o._p(ws), nb, o.stream())

    def step(self, cfg, t, prev, out, prev_e, prev_q, ancestors, retained=None):
        """`retained` (an abi.CsmcPath): the conditional step (include/gjx_csmc.h) — slot n - 1 keeps that path."""
        if retained is not None:
            self.ops.smc_plan_step_conditional(cfg, self.plan, t, self.y[t], prev, out, retained, prev_e, prev_q, ancestors)
            return
        self.ops.smc_plan_step(cfg, self.plan, t, self.y[t], prev, out, prev_e, prev_q, ancestors)

    def transition_table(self):
        from .runtime import use_ops
        from .smc_plan import build_transition_table

        if self.source is None:
            raise ValueError("this plan filter was not bound from a StateSpaceModel: no transition to lower")
        with use_ops(self.ops):
            return build_transition_table(*self.source), (self.y if self.plan.n_obs else None)

    def sharded_run(self, comm, cfg, io):
        self.ops.lib.call("gjx_smc_sharded_run_plan", comm.handle, C.byref(cfg), self.plan.handle, self._obs, C.byref(io),
                          self.ops.stream())
