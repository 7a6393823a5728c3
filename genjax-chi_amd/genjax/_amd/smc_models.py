"""Bootstrap-filter models bound to an `Ops`, one class per kind the library has a step for (the hand-written
linear-Gaussian model, the hand-written discrete HMM, a generated plan): the one place that knows how a kind maps onto
the C ABI (include/gjx.h) — model argument, observation dtype, state columns, `gjx_smc_*` symbols, the tables that
travel with them.  The drivers (the whole-run call of `Ops`, the stepwise history filter of smc_fused.py, the sharded
filters of dist.py) are written once against `state_dtypes`, `y` (host observations as the ABI takes them), `T` and

    run(cfg, outputs)                                     gjx_smc_run_*            (outputs: Ops._smc_buffers)
    step(cfg, t, prev, out, prev_e, prev_q, ancestors)    gjx_smc_*_step
    sharded_run(comm, cfg, io)                            gjx_smc_sharded_run_*"""

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

    def sharded_run(self, comm, cfg, io):
        o = self.ops
        alias, logp = self.tables
        o.lib.call("gjx_smc_sharded_run_hmm", comm.handle, C.byref(cfg), C.byref(self.model),
                   C.c_void_p(self.y.ctypes.data), o._p(alias), o._p(logp), C.byref(io), o.stream())


class PlanFilter:
    workspace_per_filter = False  # F filters in one call: one workspace of F * stride particles

    def __init__(self, ops, plan, obs):
        """`plan`: an SmcPlan (Ops.smc_plan_create); `obs`: the [T, n_obs] observation constants ([T] for a plan without)."""
        self.ops, self.plan, self.state_dtypes = ops, plan, [torch.float32] * plan.n_state
        self.y = np.ascontiguousarray(np.asarray(obs, dtype=np.float32).reshape(-1, max(plan.n_obs, 1))[:, :plan.n_obs])
        self.T = len(self.y)
        self._obs = C.c_void_p(self.y.ctypes.data) if plan.n_obs else None

    def run(self, cfg, outputs):
        o = self.ops
        out_e, out_q, states, logw, anc, ws, nb = outputs
        cols = (C.c_void_p * len(states))(*[c.data_ptr() for c in states])
        o.lib.call("gjx_smc_run_plan", C.byref(cfg), self.plan.handle, self._obs, o._p(out_e), o._p(out_q), cols,
                   o._p(logw), o._p(anc), o._p(ws), nb, o.stream())

    def step(self, cfg, t, prev, out, prev_e, prev_q, ancestors):
        self.ops.smc_plan_step(cfg, self.plan, t, self.y[t], prev, out, prev_e, prev_q, ancestors)

    def sharded_run(self, comm, cfg, io):
        self.ops.lib.call("gjx_smc_sharded_run_plan", comm.handle, C.byref(cfg), self.plan.handle, self._obs, C.byref(io),
                          self.ops.stream())
