"""Bootstrap SMC on the fused state-space kernels (`gjx_smc_run_*` / `gjx_smc_*_step`: the hand-written
linear-Gaussian model and discrete HMM, and the generated plan of a user-written `StateSpaceModel`).

The reference's SMC module has no resampling step or SMC loop; the north star
asks for bootstrap SMC with systematic resampling and an ancestor gather.  This is that driver:
one call enqueues the whole T-step filter — per step one fused resample+gather+propagate+weight
kernel and one tile-sum kernel — with no host synchronisation.  `_bind_model` turns a model class into
the bound filter model (smc_models.py) that the whole-run call and the stepwise history filter run; it is
the only place here that tells the kinds apart.  The model classes are the fixed-structure equivalents of
the `@scan`/`@gen` kernels

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
from .smc_models import HmmFilter, LgssmFilter, PlanFilter
from .smc_plan import StateSpaceModel, build_guided_plan, build_smc_plan, check_conditional, observation_matrix
from .workloads import smc_key_schedule


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
        return Trajectories(_columns(paths[:n_state]), out["lineage"], out["unique"],
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


def _columns(cols):
    """State columns as results carry them: the tensor itself for one column, a tuple for a multi-component carry."""
    return cols[0] if len(cols) == 1 else tuple(cols)


def _obs_addrs(observations: ChoiceMap) -> list:
    return [a for a, _ in observations.leaves()]


def _build_plan(ops, model: StateSpaceModel, observations: ChoiceMap, theta=None):
    """-> (SmcPlan, observation matrix [T, n_obs]) of a user-written model and its observed sequences.  `theta`: where a
    model with parameters is traced (smc_plan.build_smc_plan)."""
    addrs = _obs_addrs(observations)
    with use_ops(ops):
        plan, _ = build_smc_plan(model, addrs, theta)
    return plan, observation_matrix(observations, addrs)


def _bind_model(ops, model, observations, plan=None):
    """The model bound to `ops` (smc_models.py) that every driver below runs; the uploads of a fixed model happen here,
    per call.  `observations`: as for BootstrapSMC.  `plan`: what `_build_plan` returned for a StateSpaceModel earlier."""
    if isinstance(model, LinearGaussianSSM):
        return LgssmFilter(ops, abi.Lgssm(model.x0_loc, model.x0_scale, model.a, model.q, model.r), observations)
    if isinstance(model, DiscreteHMM):
        dev = ops.device()
        tl = torch.as_tensor(model.trans_logits, dtype=torch.float32).to(dev).contiguous()
        ol = torch.as_tensor(model.obs_logits, dtype=torch.float32).to(dev).contiguous()
        return HmmFilter(ops, int(tl.shape[0]), int(model.init_state), tl, ol, observations)
    if isinstance(model, StateSpaceModel):
        plan, obs = plan or _build_plan(ops, model, observations)
        return PlanFilter(ops, plan, obs, source=(model, _obs_addrs(observations)))
    raise TypeError(f"no fused SMC kernel for {type(model).__name__}")


def run_with_history(ops, model, observations, n: int, key: prng.PRNGKey, ess_threshold: float = 0.0) -> SMCResult:
    """The bootstrap filter of `BootstrapSMC.run`, driven STEP BY STEP through `ops` so that every step's population stays:
    step t writes its state columns and log-weights into row t of `[T, stride]` buffers and step t + 1 reads them there — the
    history costs no copy and no kernel of its own.  The per-step scratch (fixed-point weights, tile records) ping-pongs
    between two populations.  Rows have a stride of whole tiles (16-byte aligned rows whatever n is: the steps' 16-byte
    stores stay 16-byte stores and inside their row).  Every field the whole-run call also returns is bit-equal to it.
    `observations`: as for BootstrapSMC.  One filter on one device: filter batches (`run_many`) and the sharded drivers do not record history."""
    return _history_run(ops, _bind_model(ops, model, observations), n, key, ess_threshold)


def _history_run(ops, model, n: int, key: prng.PRNGKey, ess_threshold: float, retained=None, log_z: bool = True) -> SMCResult:
    """`run_with_history` of a bound model.  `retained` (an abi.CsmcPath, plan filters only): every step is the conditional
    step (include/gjx_csmc.h) — slot n - 1 carries that path through the run.  `log_z=False`: `log_marginal_likelihood`
    stays None — its float64 sum is formed on the host, the one host read of a run."""
    n, T = int(n), model.T
    how = {} if retained is None else {"retained": retained}
    sk, rk = smc_key_schedule(key, T)
    cfg = ops.smc_config(key.impl, n, 0, n, sk, rk, ess_threshold)
    stride = ops.num_tiles(n) * ops.tile
    # each buffer once, uninitialised: 4 T stride bytes per column
    hist = [ops.empty((T, stride), dt) for dt in model.state_dtypes]
    lw = ops.empty((T, stride), torch.float32)
    anc = ops.empty((T, stride), torch.int32)
    out_e, out_q = ops.empty(T, torch.int32), ops.empty(T, torch.int64)
    pops = [ops.smc_pop(n, [], cfg._adaptive, want_logw=False) for _ in range(2)]
    structs = []
    for t in range(T):  # the population of step t: scratch of parity t, state / log-weights in row t
        p = pops[t & 1].struct()
        for k, h in enumerate(hist):
            p.state[k] = h[t].data_ptr()
        p.logw = lw[t].data_ptr()
        structs.append(p)
    # (views made once, outside the loop of launches: the loop is host-bound)
    anc_rows, e_rows, q_rows = anc.unbind(0), out_e.split(1), out_q.split(1)
    model.step(cfg, 0, None, structs[0], None, None, anc_rows[0], **how)
    for t in range(1, T):
        model.step(cfg, t, structs[t - 1], structs[t], e_rows[t - 1], q_rows[t - 1], anc_rows[t], **how)
    ops.smc_finish(cfg, pops[(T - 1) & 1].recs, e_rows[T - 1], q_rows[T - 1])
    cols = [h[:, :n] for h in hist]
    flags = cfg._flags
    return SMCResult(ops.log_z_from_pairs(out_e, out_q, n, flags) if log_z else None, out_e, out_q, _columns([c[T - 1] for c in cols]),
                     lw[T - 1, :n], anc[:, :n], flags, _columns(cols), lw[:, :n])


def _result(ops, n: int, out, f: int | None = None) -> SMCResult:
    """One filter's result from what the whole-run call returned (Ops._smc_run); `f`: filter f of an `[F, stride]` batch."""
    step_e, step_q, states, logw, anc, flags = out
    if f is not None:
        step_e, step_q, states, logw = step_e[f], step_q[f], [c[f, :n] for c in states], logw[f, :n]
        anc, flags = None if anc is None else anc[:, f, :n], None if flags is None else flags[f]
    return SMCResult(ops.log_z_from_pairs(step_e, step_q, n, flags), step_e, step_q, _columns(states), logw, anc, flags)


class BootstrapSMC:
    """Bootstrap particle filter with systematic resampling: at every step (default), or — `ess_threshold` in (0, 1) —
    only when the effective sample size of the current weights falls below `ess_threshold * n_particles`; between
    resamplings the log-weights accumulate (gjx.h: gjx_smc_config.ess_threshold)."""

    def __init__(self, model, observations, n_particles: int, record_ancestors: bool = False, ess_threshold: float = 0.0,
                 record_history: bool = False, params=None):
        """`params`: the default parameter row theta of a `StateSpaceModel(..., params=names)` (a sequence in declaration
        order); `run(key, params=...)` / `run_many(keys, params=...)` take a row (or one per key) for that call.  The plan
        is compiled once, whatever theta is; a row is rounded to f32 and that is what the filter runs.

        `record_history`: `run()` also returns every step's particles and log-weights (`SMCResult.history`,
        `.log_weight_history`; the ancestor table is then always recorded) — what `SMCResult.trajectories` traces back.
        Memory: 4 T n bytes per state column, the log-weights and the ancestors (T=100, n=1e6: 0.4 GB each).  Such a run
        is a stream of per-step launches (`run_with_history`), bit-equal to the default whole-run call in everything both
        return; `run_many` then runs its filters one at a time."""
        self.model, self.n, self.record_ancestors = model, int(n_particles), record_ancestors
        self.record_history = bool(record_history)
        self.ess_threshold = float(ess_threshold)
        self._plan = None  # (SmcPlan, observation matrix) of a StateSpaceModel, built at the first run
        self._transition = None  # (BacksimPlan, observation rows) of `backward_simulate`, built at its first call
        self.params = None if params is None else np.asarray(params, dtype=np.float64).reshape(-1)
        self._parameterised = isinstance(model, StateSpaceModel) and bool(model.params)
        if params is not None and not self._parameterised:
            raise ValueError("params=... needs a StateSpaceModel that declares parameters (StateSpaceModel(init, step, params=(...)))")
        if self.params is not None and len(self.params) != len(model.params):
            raise ValueError(f"the model declares {len(model.params)} parameters {model.params}, got {len(self.params)} values")
        if isinstance(model, StateSpaceModel) and not isinstance(observations, ChoiceMap):
            raise TypeError("observations for a StateSpaceModel are a ChoiceMap of length-T sequences")
        self.observations = observations if isinstance(observations, ChoiceMap) else np.asarray(observations)

    def get_num_particles(self):
        return self.n

    def _bind(self, ops, theta=None):
        """The filter model bound to `ops`: per call for a fixed model (its tensors may change between runs); the plan and
        the observation matrix of a StateSpaceModel are built once and kept (`theta`: where a model with parameters is
        traced that once)."""
        if isinstance(self.model, StateSpaceModel) and self._plan is None:
            self._plan = _build_plan(ops, self.model, self.observations, theta)
        return _bind_model(ops, self.model, self.observations, self._plan)

    def _thetas(self, params, n_keys: int | None = None):
        """The theta rows of a call, f64[1 or n_keys, P] (None for a model without parameters): `params`, else the default."""
        if not self._parameterised:
            if params is not None:
                raise ValueError("params=... needs a StateSpaceModel that declares parameters")
            return None
        th = self.params if params is None else np.asarray(params, dtype=np.float64)
        if th is None:
            raise ValueError(f"the model declares the parameters {self.model.params}: pass params=... to the filter or to this call")
        P = len(self.model.params)
        th = th.reshape(1, -1) if th.ndim < 2 else th
        if th.ndim != 2 or th.shape[1] != P or th.shape[0] not in ((1,) if n_keys is None else (1, n_keys)):
            raise ValueError(f"params: one row of {P} values" + ("" if n_keys is None else f", or an array [{n_keys}, {P}] (one row per key)")
                             + f"; got shape {tuple(np.shape(params if params is not None else self.params))}")
        return th

    def _set_rows(self, model, thetas):
        """The slot rows of `thetas` (smc_plan.ParamSpace: theta, then the values the bodies derive from it on the host) into
        the plan, for the launches that follow."""
        if thetas is not None:
            model.plan.set_params(model.plan._space.rows(thetas))

    def _check_conditional(self, ops):
        """What `run(retained=...)` asks of the filter itself, before anything is bound."""
        if not isinstance(self.model, StateSpaceModel):
            raise ValueError(f"run(retained=...): the conditional filter runs generated plans only — {type(self.model).__name__} is "
                             "a fixed model: write it as a StateSpaceModel")
        if not self.record_history:
            raise ValueError("run(retained=...) needs the per-step states: build the filter with record_history=True")
        if 0.0 < self.ess_threshold < 1.0:
            raise ValueError("run(retained=...): ESS-adaptive conditional filters are out of scope (ess_threshold must be 0)")
        if self.n < 2:
            raise ValueError("run(retained=...): at least 2 particles (the last slot is the retained one)")
        ops.lib.require("csmc", "gjx_smc_plan_step_conditional")

    def _retained_columns(self, ops, model, retained) -> list:
        """`retained` as the conditional step takes it: one contiguous f32[T] device tensor per carry component."""
        check_conditional(model.plan)
        cols = list(retained) if isinstance(retained, (tuple, list)) else [retained]
        if len(cols) != model.plan.n_state:
            raise ValueError(f"run(retained=...): the carry has {model.plan.n_state} component(s), got {len(cols)} path column(s)")
        out = []
        for k, c in enumerate(cols):
            c = torch.as_tensor(c)
            if c.numel() != model.T or c.dim() > 2 or (c.dim() == 2 and c.shape[0] != model.T):
                raise ValueError(f"run(retained=...): component {k} must be a path of T = {model.T} values ([T], or a [T, 1] column "
                                 f"of a Trajectories), got shape {tuple(c.shape)}")
            out.append(c.to(device=ops.device(), dtype=torch.float32).reshape(-1).contiguous())
        return out

    def run(self, key: prng.PRNGKey, params=None, retained=None) -> SMCResult:
        """`retained`: a path x*_0:T-1 — a tensor [T], or a tuple of them for a multi-component carry (a column of a
        `Trajectories` with one path qualifies) — makes the run a CONDITIONAL particle filter: the last
        particle, slot n - 1, carries x* at every step and is its own ancestor; slots 0 .. n - 2 are resampled by a comb of
        n - 1 teeth over all n particles.  An ordinary `SMCResult` (`trajectories`, `backward_simulate` work on it
        unchanged).  Needs `record_history=True`, a `StateSpaceModel` whose sampled sites are exactly its carry components
        (`PlanUnsupported` otherwise) and `ess_threshold == 0`."""
        return self._run(key, params, retained)

    def _run(self, key: prng.PRNGKey, params=None, retained=None, log_z: bool = True) -> SMCResult:
        """`run`; `log_z=False` (ParticleGibbs' sweeps and the timing tools, record_history filters only): the float64 sum of
        log Z is not formed — it is the one host read of a stepwise run — and `log_marginal_likelihood` is None; `step_e` /
        `step_q` hold the exact pairs on the device."""
        ops = get_ops()
        if retained is not None:
            self._check_conditional(ops)
        thetas = self._thetas(params)
        model = self._bind(ops, None if thetas is None else thetas[0])
        if retained is not None:
            path = ops.csmc_path(self._retained_columns(ops, model, retained))
            self._set_rows(model, thetas)
            return _history_run(ops, model, self.n, key, 0.0, path, log_z)
        self._set_rows(model, thetas)
        if self.record_history:
            return _history_run(ops, model, self.n, key, self.ess_threshold, log_z=log_z)
        sk, rk = smc_key_schedule(key, model.T)
        return _result(ops, self.n, ops._smc_run(model, key.impl, self.n, sk, rk, self.record_ancestors, self.ess_threshold))

    def backward_simulate(self, result: SMCResult, key: prng.PRNGKey, n_paths: int, max_workgroups: int = 0,
                          n_moves: int | None = None) -> "Trajectories":
        """Backward-simulation smoothing: `n_paths` trajectories x_0:T-1, each drawn afresh from the recorded
        populations of `result` (a `record_history=True` run of THIS filter) — x_T-1 from the final weights, then x_t from
        all n particles of step t with weights w_t^i f(x_t+1 | x_t^i) — in one library call of T + 1 stream-ordered launches
        (gjx_backsim_run; no [n_paths, n] array exists anywhere).  Unlike `SMCResult.trajectories` it does not follow the
        genealogy, so early steps keep as many distinct particles as the weights allow.  Equally weighted paths:
        `mean()` / `var()` are smoothing moments; the lineage rows are not ordered.

        The transition density is the model's own (`GuidedSMC`: the underlying StateSpaceModel's; proposals play no part).
        `PlanUnsupported` when the carry is not exactly the step's latent draws (a degenerate transition);
        `abi.BacksimUnavailable` on a library without include/gjx_backsim.h; `ValueError` without recorded history.

        `n_moves=K` (an int, 0 .. 256) selects the MCMC backward sampler instead (Bunch & Godsill 2013): every
        path starts a step at its genealogical ancestor and makes K Metropolis-Hastings moves proposed from that step's
        filter weights (gjx_backmove_run) — n_paths K (T - 1) transition densities whatever n is, so it runs at the filter's
        own size; K = 0 is trace-back from multinomial leaves, and a few moves already undo the genealogy's collapse.  It
        reads `result.ancestors` (`ValueError` without); `abi.BackmoveUnavailable` on a library without
        include/gjx_backmove.h.  `n_moves=None`: the exact method above."""
        if self._parameterised:
            from .plan import PlanUnsupported

            raise PlanUnsupported(f"backward_simulate() of a model with parameters {self.model.params}: transition tables hold "
                                  "constants only — build the model at a fixed θ to smooth")
        if result.history is None or result.log_weight_history is None:
            raise ValueError("backward_simulate() needs the per-step states: run the filter with BootstrapSMC(..., record_history=True)")
        if n_moves is not None:
            if isinstance(n_moves, bool) or not isinstance(n_moves, (int, np.integer)) or not 0 <= int(n_moves) <= abi.BACKMOVE_MAX_MOVES:
                raise ValueError(f"backward_simulate(): n_moves must be None or an int in 0 .. {abi.BACKMOVE_MAX_MOVES}, got {n_moves!r}")
            if result.ancestors is None:
                raise ValueError("backward_simulate(n_moves=...) starts every path at its genealogical ancestor: the result has no ancestor table")
        ops = get_ops()
        if n_moves is not None:
            ops.lib.require("backmove", "gjx_backmove_run")
        ops.lib.require("backsim", "gjx_backsim_run")
        if self._transition is None:
            table, obs = self._bind(ops).transition_table()
            self._transition = (ops.backsim_plan_create(table), obs)
        plan, obs = self._transition
        cols = list(result.history) if isinstance(result.history, tuple) else [result.history]
        m = int(n_paths)
        if n_moves is None:
            out = ops.backsim_run(plan, key, cols, result.log_weight_history, obs, m, max_workgroups=max_workgroups)
        else:
            out = ops.backmove_run(plan, key, cols, result.log_weight_history, result.ancestors, obs, m, int(n_moves),
                                   max_workgroups=max_workgroups)
        paths, lin = out["paths"], out["lineage"]
        # float64 moments and distinct counts from the returned columns (T m elements: small against the n m T pass)
        is_f32 = [c.dtype == torch.float32 for c in paths]
        zero = torch.zeros(lin.shape[0], dtype=torch.float64, device=lin.device)
        sums = torch.stack([p.double().sum(1) if f else zero for p, f in zip(paths, is_f32)])
        sumsq = torch.stack([(p.double() * p.double()).sum(1) if f else zero for p, f in zip(paths, is_f32)])
        srt = lin.sort(dim=1).values
        unique = 1 + (srt[:, 1:] != srt[:, :-1]).sum(1)
        return Trajectories(_columns(paths), lin, unique.to(torch.int64), None, None, sums, sumsq, is_f32)

    def run_many(self, keys, params=None, retained=None) -> list:
        """`vmap(self.run)(keys)`: one independent filter per key.  Up to 16 filters step in the same kernel launches
        (`gjx_smc_config.n_filters`: a 1e6-particle step alone is under one round of an MI355X), for the hand-written
        models and for generated ones alike; element b equals `self.run(keys[b])` bit for bit.
        `params` (a model with parameters): one theta row for every key, or an array [len(keys), P] with one row per key —
        a BANK of filters, filter b at theta_b in the same launches; element b equals `self.run(keys[b], params=rows[b])`."""
        if retained is not None:
            raise ValueError("run_many(retained=...): conditional filters run one at a time — call run(key, retained=...) per key")
        keys = list(keys)
        thetas = self._thetas(params, len(keys))
        row = (lambda b: None) if thetas is None else (lambda b: thetas[b if len(thetas) > 1 else 0])
        if self.record_history or len(keys) < 2:
            return [self.run(k, row(b)) for b, k in enumerate(keys)]
        ops, out = get_ops(), []
        model = self._bind(ops, row(0))
        for lo in range(0, len(keys), 16):
            chunk = keys[lo:lo + 16]
            if len(chunk) == 1:
                out.append(self.run(chunk[0], row(lo)))
                continue
            try:
                self._set_rows(model, None if thetas is None else (thetas if len(thetas) == 1 else thetas[lo:lo + 16]))
                out.extend(self._run_chunk(ops, chunk, model.T, model))
            except abi.GjxError as e:
                # populations too large for a filter batch (more than 2048 tiles per filter, or a workspace the
                # device cannot hold): the documented contract is "element b equals self.run(keys[b])" — run them so
                if e.code not in (-2, -3):  # GJX_ERR_UNSUPPORTED, GJX_ERR_WORKSPACE
                    raise
                out.extend(self.run(k, row(lo + b)) for b, k in enumerate(chunk))
        return out

    def log_marginal_likelihoods(self, keys, params=None) -> np.ndarray:
        """float64[len(keys)]: the log-marginal-likelihood estimate of every filter of `run_many(keys, params)` — with one
        theta row per key, up to 16 points of a likelihood surface per launch."""
        return np.asarray([r.log_marginal_likelihood for r in self.run_many(keys, params)], dtype=np.float64)

    def _run_chunk(self, ops, chunk, T, model) -> list:
        pairs = [smc_key_schedule(k, T) for k in chunk]
        sk, rk = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        out = ops._smc_run(model, chunk[0].impl, self.n, sk, rk, self.record_ancestors, self.ess_threshold)
        return [_result(ops, self.n, out, f) for f in range(len(chunk))]

    def log_marginal_likelihood_estimate(self, key: prng.PRNGKey, params=None) -> float:
        return self.run(key, params).log_marginal_likelihood


class GuidedSMC(BootstrapSMC):
    """Particle filter of a `StateSpaceModel` whose latent sites are drawn from USER PROPOSALS instead of the model's own
    transition (a bootstrap filter collapses when the observations are sharp against the transition noise):

        @gen
        def track_q(carry, y):               # (the carry as `step` receives it, this step's observations)
            normal(c1 * carry + c2 * y, s) @ "x"

        GuidedSMC(StateSpaceModel(init, step), C["y"].set(ys), n, step_proposal=track_q).run(key)

    `y` is a scalar when one address is observed and a tuple in the order of the observation ChoiceMap's leaves when several
    are; a proposal's return value is ignored.  A proposal site is paired with the model's body-level latent site of the
    same address: the model's site takes the proposed value and the step's weight is multiplied by p(x_t | x_{t-1}) /
    q(x_t | x_{t-1}, y_t).  Model latents without a partner keep being drawn from the model.  Without
    `init_proposal(y)` step 0 is the bootstrap filter's.  `PlanUnsupported` (naming the address): a proposal site without
    a model partner or on an observed address, an integer-valued site paired with a float-valued one, a nested `@gen`
    call inside a proposal or in the model's bodies.

    Everything else is `BootstrapSMC`: the lowering gives an ordinary generated plan, so `run`, `run_many`, `ess_threshold`,
    `record_history`, `SMCResult.trajectories` and one-launch-per-step / graph replay work unchanged.  The two site modes
    exist in libgjx_hip.so only (include/gjx_guided.h): on other libraries `abi.GuidedUnavailable`.  Guided plans in the
    sharded drivers (`ShardedSMC`) are out of scope: nothing there has been run or tested with them."""

    def __init__(self, model: StateSpaceModel, observations, n_particles: int, step_proposal, init_proposal=None,
                 record_ancestors: bool = False, ess_threshold: float = 0.0, record_history: bool = False, params=None):
        """A model with parameters (`StateSpaceModel(..., params=...)`): the proposals take theta last,
        `step_proposal(carry, y, theta)` and `init_proposal(y, theta)`; `params` as for BootstrapSMC."""
        if not isinstance(model, StateSpaceModel):
            raise TypeError("GuidedSMC guides a StateSpaceModel (the hand-written models have no proposal sites)")
        super().__init__(model, observations, n_particles, record_ancestors, ess_threshold, record_history, params)
        self.step_proposal, self.init_proposal = step_proposal, init_proposal

    def _bind(self, ops, theta=None):
        if self._plan is None:
            addrs = [a for a, _ in self.observations.leaves()]
            with use_ops(ops):
                plan, _ = build_guided_plan(self.model, addrs, self.step_proposal, self.init_proposal, theta)
            self._plan = (plan, observation_matrix(self.observations, addrs))
        return PlanFilter(ops, *self._plan, source=(self.model, _obs_addrs(self.observations)))


class ParticleMH:
    """Particle-marginal Metropolis-Hastings over the parameters of a `StateSpaceModel(..., params=...)`: `n_chains`
    (<= 16) independent random-walk chains whose particle filters step as ONE filter bank — one `run_many` per iteration,
    the proposal of chain c in row c — so an iteration costs the launches of a single filter run.

        pmmh = ParticleMH(BootstrapSMC(model, obs, n, params=theta0), log_prior, step_scale=0.15, n_chains=8)
        samples, log_likelihood, accepted = pmmh.run(key, theta0, n_iters)

    `log_prior(theta row f32[P]) -> float` (-inf outside the support); `step_scale`: a number or a length-P sequence.
    `run` returns `samples float64[n_iters + 1, C, P]`, `log_likelihood float64[n_iters + 1, C]` (the estimate the chain
    holds) and `accepted bool[n_iters, C]`.  Fully specified, so a run can be replayed:

      rng = np.random.default_rng([k0, k1]) (the key's two words); the filter key of iteration i (0: the initial state)
      and chain c is fold_in(fold_in(key, i), c); per iteration z = rng.standard_normal((C, P)), then u = rng.random(C);
      the proposal is theta + step_scale * z rounded to f32 and stored as such (the stored theta is what the filter ran);
      accept iff log(u) < (ll' + lp') - (ll + lp).  A proposal with log_prior == -inf is rejected: its bank row runs the
      chain's CURRENT theta and the result is discarded — no value outside the support (a negative scale) ever reaches a
      kernel and the launch shape never changes.

    `log_likelihood=` (a callable `rows f32[C, P] -> float64[C]`) replaces the bank (`smc` may then be None): the tests
    that run without a GPU drive the sampler with an exact likelihood through it."""

    def __init__(self, smc, log_prior, step_scale, n_chains: int = 8, log_likelihood=None):
        if not 1 <= int(n_chains) <= 16:
            raise ValueError("ParticleMH: n_chains in 1 .. 16 (the filters of one launch)")
        if log_likelihood is None:
            if not isinstance(smc, BootstrapSMC) or not smc._parameterised:
                raise TypeError("ParticleMH needs a BootstrapSMC / GuidedSMC over a StateSpaceModel(..., params=...), or log_likelihood=")
            if smc.record_history:
                raise ValueError("ParticleMH: a record_history filter runs one filter at a time; build the filter without it")
        self.smc, self.log_prior, self.n_chains, self.log_likelihood = smc, log_prior, int(n_chains), log_likelihood
        self.step_scale = np.asarray(step_scale, dtype=np.float64)

    def _bank(self, key: prng.PRNGKey, i: int, rows: np.ndarray) -> np.ndarray:
        if self.log_likelihood is not None:
            return np.asarray(self.log_likelihood(rows), dtype=np.float64).reshape(self.n_chains)
        ki = prng.fold_in(key, i)
        return self.smc.log_marginal_likelihoods([prng.fold_in(ki, c) for c in range(self.n_chains)], rows)

    def run(self, key: prng.PRNGKey, theta0, n_iters: int):
        C = self.n_chains
        theta0 = np.asarray(theta0, dtype=np.float32).reshape(-1)
        P = theta0.size
        lp0 = float(self.log_prior(theta0))
        if not np.isfinite(lp0):
            raise ValueError("ParticleMH.run: log_prior(theta0) must be finite")
        rng = np.random.default_rng([key.k0, key.k1])
        theta = np.tile(theta0, (C, 1))  # f32[C, P]: what the filters ran
        lp = np.full(C, lp0, dtype=np.float64)
        ll = self._bank(key, 0, theta)
        samples = np.empty((n_iters + 1, C, P), dtype=np.float64)
        lls = np.empty((n_iters + 1, C), dtype=np.float64)
        accepted = np.zeros((n_iters, C), dtype=bool)
        samples[0], lls[0] = theta, ll
        for i in range(1, n_iters + 1):
            z = rng.standard_normal((C, P))
            u = rng.random(C)
            prop = (theta.astype(np.float64) + self.step_scale * z).astype(np.float32)
            lp_new = np.asarray([float(self.log_prior(prop[c])) for c in range(C)], dtype=np.float64)
            live = lp_new > -np.inf
            ll_new = self._bank(key, i, np.where(live[:, None], prop, theta))
            acc = live & (np.log(u) < (ll_new + lp_new) - (ll + lp))
            theta = np.where(acc[:, None], prop, theta)
            ll, lp = np.where(acc, ll_new, ll), np.where(acc, lp_new, lp)
            samples[i], lls[i], accepted[i - 1] = theta, ll, acc
        return samples, lls, accepted


@dataclass
class ParticleGibbsResult:
    paths: torch.Tensor | tuple  # f32[n_sweeps, T] (a tuple of columns for a multi-component carry): the path after every sweep
    thetas: np.ndarray | None  # float64[n_sweeps, P]: the parameter row after every sweep (a model with parameters)


class ParticleGibbs:
    """Particle Gibbs (Andrieu, Doucet & Holenstein 2010) on the conditional filter: every sweep runs `smc` with the current
    path retained in its last slot (`run(key, retained=path)`), draws ONE final particle by its weight and takes that
    particle's path as the new one.  It needs no more than a handful of particles (>= 2) to keep moving where PMMH stalls.

    How exact it is (profiles/csmc_summary.md): the free slots are resampled by a systematic comb in FIXED slot
    order, under which a free slot's ancestor does not have the weights as its marginal law, and the sweep relabels the path
    it selected as the last slot.  With `refresh="trace"` the chain's stationary law is therefore close to, not exactly,
    p(x_0:T-1 | y, theta): a float64 restatement of the sampler measures smoothing means off by about 0.02 posterior
    standard deviations at n = 4 .. 8 on the linear-Gaussian model (multinomial resampling of the free slots: none).
    `refresh="backward"` draws the path from the recorded populations without following the slots' genealogy; prefer it
    where that matters.

        pg = ParticleGibbs(BootstrapSMC(model, obs, 8, record_history=True), refresh="trace")
        paths = pg.run(key, n_sweeps=2000).paths            # [n_sweeps, T]

    `refresh="trace"`: the drawn leaf is traced back through the ancestor table (gjx_paths_trace, one launch);
    `refresh="backward"`: the path is drawn afresh by backward simulation over the recorded populations
    (`backward_simulate(..., n_paths=1)`: particle Gibbs with backward simulation, which mixes over early steps even with
    very few particles) — not available for a model with parameters (`PlanUnsupported`: transition tables hold constants).
    `param_update(key, path, theta) -> theta`: the user's Gibbs / Metropolis update of theta given the path, run on the
    host between sweeps; its result (rounded to f32 by the filter) is the next sweep's row.

    Fully specified, so a run can be replayed sweep by sweep: with k_s = fold_in(key, s), the filter of sweep s runs under
    fold_in(k_s, 0), the leaf is `categorical_index(fold_in(k_s, 1), final log-weights)` (a Gumbel-max draw by the
    weights — not a fixed slot of a systematic comb, which is not distributed by the weights), the backward pass runs
    under fold_in(k_s, 2) (it draws its own leaf from the final weights) and `param_update` gets fold_in(k_s, 3).  Sweep 0
    is an UNCONDITIONAL run when `init` is None.  The path stays on the device from sweep to sweep: no host read happens
    inside a sweep unless `param_update` makes one."""

    def __init__(self, smc: BootstrapSMC, refresh: str = "trace", param_update=None):
        if not isinstance(smc, BootstrapSMC) or not isinstance(smc.model, StateSpaceModel):
            raise TypeError("ParticleGibbs needs a BootstrapSMC / GuidedSMC over a StateSpaceModel (a fixed model: write it as a StateSpaceModel)")
        if refresh not in ("trace", "backward"):
            raise ValueError(f"ParticleGibbs: refresh is 'trace' or 'backward', got {refresh!r}")
        if not smc.record_history:
            raise ValueError("ParticleGibbs needs the per-step states: build the filter with record_history=True")
        if 0.0 < smc.ess_threshold < 1.0:
            raise ValueError("ParticleGibbs: ESS-adaptive conditional filters are out of scope (ess_threshold must be 0)")
        if refresh == "backward" and smc._parameterised:
            from .plan import PlanUnsupported

            raise PlanUnsupported(f"ParticleGibbs(refresh='backward') of a model with parameters {smc.model.params}: transition "
                                  "tables hold constants only — use refresh='trace'")
        if param_update is not None and not smc._parameterised:
            raise ValueError("ParticleGibbs(param_update=...) needs a StateSpaceModel that declares parameters")
        self.smc, self.refresh, self.param_update = smc, refresh, param_update

    def sweep(self, k_s: prng.PRNGKey, path, theta=None):
        """One sweep under its key k_s = fold_in(key, s) -> the new path, a list of contiguous f32[T] device tensors.
        `path`: the retained path (None: an unconditional run)."""
        ops = get_ops()
        res = self.smc._run(prng.fold_in(k_s, 0), theta, None if path is None else tuple(path), log_z=False)
        if self.refresh == "backward":
            new = self.smc.backward_simulate(res, prng.fold_in(k_s, 2), 1).paths
            return [c.reshape(-1).contiguous() for c in (new if isinstance(new, tuple) else (new,))]
        leaf = ops.categorical_index(prng.fold_in(k_s, 1).literal(), res.log_weights.contiguous()).to(torch.int32)
        cols = list(res.history) if isinstance(res.history, tuple) else [res.history]
        out = ops.paths_trace(res.ancestors, cols, leaf, lineage=False)
        return [c.reshape(-1).contiguous() for c in out["paths"]]

    def run(self, key: prng.PRNGKey, n_sweeps: int, init=None, params=None) -> ParticleGibbsResult:
        """`init`: the first retained path (as `run(retained=...)` takes it); None: sweep 0 is an unconditional run.
        `params`: the first parameter row of a model with parameters (default: the filter's)."""
        thetas = self.smc._thetas(params)
        theta = None if thetas is None else np.asarray(thetas[0], dtype=np.float32).astype(np.float64)
        path = None if init is None else (list(init) if isinstance(init, (tuple, list)) else [init])
        kept, rows = [], []
        for s in range(int(n_sweeps)):
            k_s = prng.fold_in(key, s)
            path = self.sweep(k_s, path, theta)
            if self.param_update is not None:
                new = self.param_update(prng.fold_in(k_s, 3), _columns(path), theta.copy())
                theta = np.asarray(new, dtype=np.float32).astype(np.float64).reshape(-1)
            kept.append(path)
            if theta is not None:
                rows.append(theta.copy())
        paths = _columns([torch.stack([p[k] for p in kept]) for k in range(len(kept[0]))]) if kept else None
        return ParticleGibbsResult(paths, np.stack(rows) if rows else None)
