"""Bootstrap SMC on the fused state-space kernels (`gjx_smc_run_lgssm` / `gjx_smc_run_hmm`).

The reference's SMC module has no resampling step or SMC loop; the north star
asks for bootstrap SMC with systematic resampling and an ancestor gather.  This is that driver:
one call enqueues the whole T-step filter — per step one fused resample+gather+propagate+weight
kernel and one tile-sum kernel — with no host synchronisation.  The model classes are the
fixed-structure equivalents of the `@scan`/`@gen` kernels

    x' = normal(a * x, q) @ "x";  normal(x', r) @ "y"                  (LinearGaussianSSM)
    z' = categorical(T[z, :]) @ "z";  categorical(O[z', :]) @ "x"      (DiscreteHMM, exact_testbed.py:62-68)
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import abi, prng
from .choicemap import ChoiceMap
from .runtime import get_ops, use_ops
from .smc_plan import StateSpaceModel, build_smc_plan, observation_matrix


@dataclass(frozen=True)
class LinearGaussianSSM:
    x0_loc: float = 0.0
    x0_scale: float = 1.0
    a: float = 0.9
    q: float = 1.0
    r: float = 0.5


@dataclass(frozen=True)
class DiscreteHMM:
    trans_logits: torch.Tensor  # [K, K], row = previous state
    obs_logits: torch.Tensor  # [K, K], row = state
    init_state: int = 0


@dataclass
class SMCResult:
    log_marginal_likelihood: float  # float64 from the exact per-step (max, fixed-point sum) pairs
    step_e: torch.Tensor  # int32[T]: per-step merged anchor e_t (lse_t = e_t ln 2 + log(q_t 2^-30))
    step_q: torch.Tensor  # i64[T]
    particles: torch.Tensor  # final-step particles [n] (a tuple of columns for a multi-component carry)
    log_weights: torch.Tensor  # their incremental log-weights [n]
    ancestors: torch.Tensor | None  # int32[T, n] (row 0 = identity)
    resampled: torch.Tensor | None = None  # int32[T] (ESS-adaptive filters): 1 where a step began with a resampling
    # `record_history=True`: every step's particles [T, n] (a tuple of columns for a multi-component carry; dtype as
    # `particles`) and the log-weights every step wrote, f32[T, n] (the accumulated ones in ESS-adaptive filters).  Row t
    # of `history` is the filtering population of step t: E[f(x_t) | y_1:t] ~ sum_j softmax(log_weight_history[t])_j
    # f(history[t][j]).  Rows are views into buffers whose rows are padded to whole tiles.
    history: torch.Tensor | tuple | None = None
    log_weight_history: torch.Tensor | None = None

    def get_log_marginal_likelihood_estimate(self) -> float:
        return self.log_marginal_likelihood

    def trajectories(self, key: prng.PRNGKey | None = None, n_paths: int | None = None,
                     with_log_weights: bool = False) -> "Trajectories":
        """Particle trajectories x_0:T-1, traced back through the ancestor table in ONE kernel launch (gjx_paths_trace).
        `key` given: the leaves are `n_paths` (default n) systematic-resampling draws from the final weights, so the paths
        are EQUALLY weighted draws from the particle approximation of p(x_0:T-1 | y) and `mean()` / `var()` are
        smoothing moments.  `key=None`: one path per final particle, weighted by `Trajectories.log_weights`.
        `with_log_weights`: the log-weight each path's particle had at every step, as one more traced column."""
        if self.history is None or self.log_weight_history is None or self.ancestors is None:
            raise ValueError("trajectories() needs the per-step states: run the filter with BootstrapSMC(..., record_history=True)")
        ops = get_ops()
        cols = list(self.history) if isinstance(self.history, tuple) else [self.history]
        n_state = len(cols)
        if with_log_weights:
            cols.append(self.log_weight_history)
        leaves = None
        if key is not None:
            n = self.log_weights.numel()
            leaves, _, _ = ops.resample("systematic", key.literal(), self.log_weights.contiguous(), n_paths or n)
        elif n_paths is not None:
            raise ValueError("n_paths needs a key: without one there is exactly one path per final particle")
        out = ops.paths_trace(self.ancestors, cols, leaves, sums=True, unique=True, leaves_ordered=True)
        paths = out["paths"]
        return Trajectories(paths[0] if n_state == 1 else tuple(paths[:n_state]), out["lineage"], out["unique"],
                            None if key is not None else self.log_weights,
                            paths[n_state] if with_log_weights else None, out["sum"][:n_state], out["sumsq"][:n_state],
                            [c.dtype == torch.float32 for c in cols[:n_state]])


@dataclass
class Trajectories:
    """What `SMCResult.trajectories` returns.  Path j is (paths[0][j], ..., paths[T-1][j]); `lineage[t][j]` is the index of
    its particle in step t's population."""
    paths: torch.Tensor | tuple  # [T, m] (a tuple of columns for a multi-component carry)
    lineage: torch.Tensor  # int32[T, m]
    unique_ancestors: torch.Tensor  # int64[T]: distinct particles of step t among the paths (path degeneracy)
    log_weights: torch.Tensor | None  # f32[m] final log-weights of WEIGHTED paths (no key); None: equally weighted
    log_weight_paths: torch.Tensor | None  # f32[T, m] with `with_log_weights`
    _sum: torch.Tensor  # float64[n_state, T], from the kernel
    _sumsq: torch.Tensor
    _is_f32: list

    def _moments(self):
        if self.log_weights is not None:
            raise ValueError("mean() / var() are defined for equally weighted paths: pass a key to trajectories()")
        m = self.lineage.shape[1]
        mean = self._sum.cpu() / m
        var = self._sumsq.cpu() / m - mean * mean
        return mean, var

    def _pick(self, x):
        outs = [x[k] if f else None for k, f in enumerate(self._is_f32)]  # (integer state columns have no moments)
        return outs[0] if not isinstance(self.paths, tuple) else tuple(outs)

    def mean(self):
        """float64[T] per f32 component (a tuple for a multi-component carry): the smoothing mean E[x_t | y_1:T]."""
        return self._pick(self._moments()[0])

    def var(self):
        """float64[T] per f32 component: sumsq / m - mean^2, evaluated in float64 on the host."""
        return self._pick(self._moments()[1])


def run_with_history(ops, model, observations, n: int, key: prng.PRNGKey, ess_threshold: float = 0.0, plan=None) -> SMCResult:
    """The bootstrap filter of `BootstrapSMC.run`, driven STEP BY STEP through `ops` so that every step's population stays:
    step t writes its state columns and log-weights into row t of `[T, stride]` buffers and step t + 1 reads them there — the
    history costs no copy and no kernel of its own.  The per-step scratch (fixed-point weights, tile records) ping-pongs
    between two populations.  Rows have a stride of whole tiles (16-byte aligned rows whatever n is: the steps' 16-byte
    stores stay 16-byte stores and inside their row).  Every field the whole-run call also returns is bit-equal to it.
    `observations`: as for BootstrapSMC.  `plan`: (SmcPlan, n_state, observation matrix) of a StateSpaceModel built earlier.
    One filter on one device: filter batches (`run_many`) and the sharded drivers do not record history."""
    n = int(n)
    dev = ops.device()
    hmm_tables = None
    if isinstance(model, LinearGaussianSSM):
        y = np.asarray(observations).astype(np.float32)
        mdl, sdt, n_state = abi.Lgssm(model.x0_loc, model.x0_scale, model.a, model.q, model.r), torch.float32, 1
    elif isinstance(model, DiscreteHMM):
        y = np.asarray(observations).astype(np.int32)
        tl = torch.as_tensor(model.trans_logits, dtype=torch.float32).to(dev).contiguous()
        ol = torch.as_tensor(model.obs_logits, dtype=torch.float32).to(dev).contiguous()
        mdl, sdt, n_state = ops.hmm_model(int(tl.shape[0]), int(model.init_state), tl, ol), torch.int32, 1
        hmm_tables = ops.hmm_prepare_model(mdl)
    elif isinstance(model, StateSpaceModel):
        if plan is None:
            addrs = [a for a, _ in observations.leaves()]
            with use_ops(ops):
                pl, n_state = build_smc_plan(model, addrs)
            plan = (pl, n_state, observation_matrix(observations, addrs))
        mdl, n_state, y = plan
        sdt = torch.float32
    else:
        raise TypeError(f"no fused SMC kernel for {type(model).__name__}")
    T = len(y)
    sk, rk = smc_key_schedule(key, T)
    cfg = ops.smc_config(key.impl, n, 0, n, sk, rk, ess_threshold)
    stride = ops.num_tiles(n) * ops.tile
    # each buffer once, uninitialised: 4 T stride bytes per column
    hist = [ops.empty((T, stride), sdt) for _ in range(n_state)]
    lw = ops.empty((T, stride), torch.float32)
    anc = ops.empty((T, stride), torch.int32)
    out_e, out_q = ops.empty(T, torch.int32), ops.empty(T, torch.int64)
    pops = [ops.smc_pop(n, [], cfg._adaptive, want_logw=False) for _ in range(2)]
    structs = []
    for t in range(T):  # the population of step t: scratch of parity t, state / log-weights in row t
        p = pops[t & 1].struct()
        for k in range(n_state):
            p.state[k] = hist[k][t].data_ptr()
        p.logw = lw[t].data_ptr()
        structs.append(p)
    # (views made once, outside the loop of launches: the loop is host-bound)
    anc_rows, e_rows, q_rows = anc.unbind(0), out_e.split(1), out_q.split(1)
    for t in range(T):
        prev = structs[t - 1] if t else None
        pe, pq = (e_rows[t - 1], q_rows[t - 1]) if t else (None, None)
        if isinstance(model, LinearGaussianSSM):
            ops.smc_lgssm_step(cfg, mdl, t, float(y[t]), prev, structs[t], pe, pq, anc_rows[t])
        elif isinstance(model, DiscreteHMM):
            ops.smc_hmm_step(cfg, mdl, t, int(y[t]), prev, structs[t], hmm_tables[0], hmm_tables[1], pe, pq, anc_rows[t])
        else:
            ops.smc_plan_step(cfg, mdl, t, y[t], prev, structs[t], pe, pq, anc_rows[t])
    ops.smc_finish(cfg, pops[(T - 1) & 1].recs, e_rows[T - 1], q_rows[T - 1])
    cols = [h[:, :n] for h in hist]
    history = cols[0] if n_state == 1 else tuple(cols)
    last = cols[0][T - 1] if n_state == 1 else tuple(c[T - 1] for c in cols)
    flags = cfg._flags
    return SMCResult(ops.log_z_from_pairs(out_e, out_q, n, flags), out_e, out_q, last, lw[T - 1, :n], anc[:, :n], flags,
                     history, lw[:, :n])


def smc_key_schedule(key: prng.PRNGKey, T: int):
    """step t propagates with fold_in(key, 2t) and resamples with fold_in(key, 2t+1) (fresh lane-0 keys;
    for threefry the same words as split(key, 2T)[2t], [2t+1])."""
    w = prng.fold_words(key, 2 * T)
    return w[0::2].copy(), w[1::2].copy()


class BootstrapSMC:
    """Bootstrap particle filter with systematic resampling: at every step (default), or — `ess_threshold` in (0, 1) —
    only when the effective sample size of the current weights falls below `ess_threshold * n_particles`; between
    resamplings the log-weights accumulate (gjx.h: gjx_smc_config.ess_threshold)."""

    def __init__(self, model, observations, n_particles: int, record_ancestors: bool = False, ess_threshold: float = 0.0,
                 record_history: bool = False):
        """`record_history`: `run()` also returns every step's particles and log-weights (`SMCResult.history`,
        `.log_weight_history`; the ancestor table is then always recorded) — what `SMCResult.trajectories` traces back.
        Memory: 4 T n bytes per state column, the log-weights and the ancestors (T=100, n=1e6: 0.4 GB each).  Such a run
        is a stream of per-step launches (`run_with_history`), bit-equal to the default whole-run call in everything both
        return; `run_many` then runs its filters one at a time."""
        self.model, self.n, self.record_ancestors = model, int(n_particles), record_ancestors
        self.record_history = bool(record_history)
        self.ess_threshold = float(ess_threshold)
        self._plan = None
        if isinstance(model, StateSpaceModel):
            if not isinstance(observations, ChoiceMap):
                raise TypeError("observations for a StateSpaceModel are a ChoiceMap of length-T sequences")
            self._obs_chm = observations
            self.observations = None
        else:
            self.observations = np.asarray(observations)

    def get_num_particles(self):
        return self.n

    def run(self, key: prng.PRNGKey) -> SMCResult:
        ops = get_ops()
        if self.record_history:
            if isinstance(self.model, StateSpaceModel):
                if self._plan is None:
                    self._obs_addrs = [a for a, _ in self._obs_chm.leaves()]
                    self._plan, self._n_state = build_smc_plan(self.model, self._obs_addrs)
                    self._obs = observation_matrix(self._obs_chm, self._obs_addrs)
                return run_with_history(ops, self.model, None, self.n, key, self.ess_threshold,
                                        plan=(self._plan, self._n_state, self._obs))
            return run_with_history(ops, self.model, self.observations, self.n, key, self.ess_threshold)
        if self.observations is not None:
            T = len(self.observations)
            sk, rk = smc_key_schedule(key, T)
        if isinstance(self.model, LinearGaussianSSM):
            m = self.model
            out = ops.smc_run_lgssm(key.impl, self.n, sk, rk, abi.Lgssm(m.x0_loc, m.x0_scale, m.a, m.q, m.r),
                                    self.observations.astype(np.float32), self.record_ancestors,
                                    ess_threshold=self.ess_threshold, want_flags=True)
        elif isinstance(self.model, DiscreteHMM):
            m = self.model
            dev = ops.device()
            tl = torch.as_tensor(m.trans_logits, dtype=torch.float32).to(dev).contiguous()
            ol = torch.as_tensor(m.obs_logits, dtype=torch.float32).to(dev).contiguous()
            out = ops.smc_run_hmm(key.impl, self.n, sk, rk, int(tl.shape[0]), int(m.init_state), tl, ol,
                                  self.observations.astype(np.int32), self.record_ancestors,
                                  ess_threshold=self.ess_threshold, want_flags=True)
        elif isinstance(self.model, StateSpaceModel):
            if self._plan is None:
                self._obs_addrs = [a for a, _ in self._obs_chm.leaves()]
                self._plan, self._n_state = build_smc_plan(self.model, self._obs_addrs)
                self._obs = observation_matrix(self._obs_chm, self._obs_addrs)
            T = self._obs.shape[0]
            sk, rk = smc_key_schedule(key, T)
            om, oq, states, logw, anc, fl = ops.smc_run_plan(self._plan, key.impl, self.n, sk, rk, self._obs,
                                                             self.record_ancestors, ess_threshold=self.ess_threshold,
                                                             want_flags=True)
            out = (om, oq, states[0] if self._n_state == 1 else tuple(states), logw, anc, fl)
        else:
            raise TypeError(f"no fused SMC kernel for {type(self.model).__name__}")
        step_e, step_q, state, logw, anc, flags = out
        return SMCResult(ops.log_z_from_pairs(step_e, step_q, self.n, flags), step_e, step_q, state, logw, anc, flags)

    def run_many(self, keys) -> list:
        """`vmap(self.run)(keys)`: one independent filter per key.  Up to 16 filters step in the same kernel launches
        (`gjx_smc_config.n_filters`: a 1e6-particle step alone is under one round of an MI355X), for the hand-written
        models and for generated ones alike; element b equals `self.run(keys[b])` bit for bit."""
        keys = list(keys)
        if self.record_history or not isinstance(self.model, (LinearGaussianSSM, DiscreteHMM, StateSpaceModel)) or len(keys) < 2:
            return [self.run(k) for k in keys]
        ops, out = get_ops(), []
        if isinstance(self.model, StateSpaceModel) and self._plan is None:
            self.run(keys[0])  # builds the plan and the observation matrix
        T = len(self.observations) if self.observations is not None else self._obs.shape[0]
        ess = dict(ess_threshold=self.ess_threshold, want_flags=True)
        for lo in range(0, len(keys), 16):
            chunk = keys[lo:lo + 16]
            if len(chunk) == 1:
                out.append(self.run(chunk[0]))
                continue
            try:
                out.extend(self._run_chunk(ops, chunk, T, ess))
            except abi.GjxError as e:
                # populations too large for a filter batch (more than 2048 tiles per filter, or a workspace the
                # device cannot hold): the documented contract is "element b equals self.run(keys[b])" — run them so
                if e.code not in (-2, -3):  # GJX_ERR_UNSUPPORTED, GJX_ERR_WORKSPACE
                    raise
                out.extend(self.run(k) for k in chunk)
        return out

    def _run_chunk(self, ops, chunk, T, ess) -> list:
        out = []
        pairs = [smc_key_schedule(k, T) for k in chunk]
        sk, rk = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        m, impl = self.model, chunk[0].impl
        if isinstance(m, StateSpaceModel):
            om, oq, states, logw, anc, fl = ops.smc_run_plan(self._plan, impl, self.n, sk, rk, self._obs,
                                                             self.record_ancestors, **ess)
            for f in range(len(chunk)):
                cols = [c[f, :self.n] for c in states]
                ff = None if fl is None else fl[f]
                out.append(SMCResult(ops.log_z_from_pairs(om[f], oq[f], self.n, ff), om[f], oq[f],
                                     cols[0] if self._n_state == 1 else tuple(cols), logw[f, :self.n],
                                     None if anc is None else anc[:, f, :self.n], ff))
            return out
        if isinstance(m, LinearGaussianSSM):
            res = ops.smc_run_lgssm(impl, self.n, sk, rk, abi.Lgssm(m.x0_loc, m.x0_scale, m.a, m.q, m.r),
                                    self.observations.astype(np.float32), self.record_ancestors, **ess)
        else:
            dev = ops.device()
            tl = torch.as_tensor(m.trans_logits, dtype=torch.float32).to(dev).contiguous()
            ol = torch.as_tensor(m.obs_logits, dtype=torch.float32).to(dev).contiguous()
            res = ops.smc_run_hmm(impl, self.n, sk, rk, int(tl.shape[0]), int(m.init_state), tl, ol,
                                  self.observations.astype(np.int32), self.record_ancestors, **ess)
        step_e, step_q, state, logw, anc, fl = res
        for f in range(len(chunk)):
            ff = None if fl is None else fl[f]
            out.append(SMCResult(ops.log_z_from_pairs(step_e[f], step_q[f], self.n, ff), step_e[f], step_q[f],
                                 state[f, :self.n], logw[f, :self.n], None if anc is None else anc[:, f, :self.n], ff))
        return out

    def log_marginal_likelihood_estimate(self, key: prng.PRNGKey) -> float:
        return self.run(key).log_marginal_likelihood
