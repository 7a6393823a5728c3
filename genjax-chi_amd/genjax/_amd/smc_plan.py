"""Lowering a user-written state-space model to the fused bootstrap-SMC kernels.

    @gen
    def init():                       # x_0 and its observation
        x = normal(0.0, 1.0) @ "x"
        normal(x, 0.5) @ "y"
        return x

    @gen
    def step(x):                      # one transition: kernel(carry) -> carry'
        x2 = normal(0.9 * x, 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    smc = BootstrapSMC(StateSpaceModel(init, step), C["y"].set(ys), n_particles=1_000_000)

Both bodies are run once with symbolic values (the same tracer as `plan.py`): the carry becomes
`GJX_ARG_STATE` references to the resampled ancestor's state columns, addresses present in the
observations become observed sites whose values are this step's observation constants
(`GJX_ARG_OBS`), and the returned carry becomes the next state expressions.  `gjx_smc_plan_create`
+ `gjx_smc_run_plan` then generate and run one fused resample+propagate+weight kernel per step.
The same restrictions as for importance plans apply (supported distributions, affine arguments).

A model that declares PARAMETERS, `StateSpaceModel(init, step, params=("a", "q", "r"))`, has bodies `init(theta)` and
`step(carry, theta)` (`theta`: a tuple in declaration order) and lowers to a parameterised plan (include/gjx_smc_params.h):
its kernels hold no value of theta, read a row of launch parameters instead, and up to 16 filters of one launch take a
row each (`BootstrapSMC.run_many(keys, params=rows)`).  The semantics are `plan.ParamVal`'s: arithmetic among parameters
and numbers happens on the HOST, per row, in the operands' own Python types — what the same number written as a literal
in the body would have gone through, hence bit-equal to it — and every distinct result that reaches a site argument, an
observed value, a carry expression or a postfix program is one SLOT of the row: slots 0 .. P-1 are theta itself, derived
ones follow in first-use order (`ParamSpace`).  `a * x` with a traced `x` is a postfix program with a parameter leaf."""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import abi
from .choicemap import ChoiceMap
from .lang import GenerativeFunction, StaticGenerativeFunction
from .plan import ParamVal, PlanTracer, PlanUnsupported, Sym, _IntSym, _Table
from .runtime import get_ops


@dataclass(frozen=True)
class StateSpaceModel:
    """x_0 ~ init();  x_t ~ step(x_{t-1}).  `init` takes no arguments and returns the first carry;
    `step` takes the carry (a scalar or a tuple of up to 4 scalars) and returns the next one.
    `params`: names of the model's scalar parameters; the bodies are then `init(theta)` and `step(carry, theta)` with
    `theta` a tuple in this order (a GuidedSMC's proposals: `step_proposal(carry, y, theta)`, `init_proposal(y, theta)`)."""

    init: GenerativeFunction
    step: GenerativeFunction
    params: tuple = ()

    def __post_init__(self):
        names = (self.params,) if isinstance(self.params, str) else tuple(self.params)
        if len(set(names)) != len(names) or not all(isinstance(k, str) for k in names):
            raise ValueError("StateSpaceModel(params=...): distinct parameter names")
        if len(names) > abi.MAX_PARAMS:
            raise ValueError(f"StateSpaceModel(params=...): at most {abi.MAX_PARAMS} parameters")
        object.__setattr__(self, "params", names)


class ParamSpace:
    """The row of a parameterised plan: slots 0 .. P-1 are theta, then one slot per derived value in first-use order,
    shared by the tracers of init, step and the proposals.  `row(theta)` evaluates every slot's derivation."""

    def __init__(self, names: tuple, theta):
        theta = [float(np.float32(v)) for v in np.asarray(theta, dtype=np.float64).reshape(-1)]
        if len(theta) != len(names):
            raise ValueError(f"the model declares {len(names)} parameters {names}, got {len(theta)} values")
        self.names = names
        self.theta = tuple(ParamVal(v, (lambda th, k=k: th[k]), name) for k, (v, name) in enumerate(zip(theta, names)))
        self.derivs = [t.deriv for t in self.theta]
        self.values = list(theta)
        for k, t in enumerate(self.theta):
            t.slot = k

    def slot(self, pv: ParamVal) -> int:
        if pv.slot is None:
            if pv.deriv is None:
                raise PlanUnsupported("a launch parameter that is not derived from the model's parameters")
            if len(self.derivs) >= abi.MAX_PARAMS:
                raise PlanUnsupported(f"too many parameter slots (theta and values derived from it: at most {abi.MAX_PARAMS})")
            self.derivs.append(pv.deriv)
            self.values.append(_f32_of(pv.value))
            pv.slot = len(self.derivs) - 1
        return pv.slot

    @property
    def n_slots(self) -> int:
        return len(self.derivs)

    def row(self, theta) -> np.ndarray:
        """f32[n_slots] for one theta (rounded to f32 first: the stored theta is what the filter runs)."""
        th = tuple(float(np.float32(v)) for v in np.asarray(theta, dtype=np.float64).reshape(-1))
        if len(th) != len(self.names):
            raise ValueError(f"the model declares {len(self.names)} parameters {self.names}, got {len(th)} values")
        return np.asarray([_f32_of(d(th)) for d in self.derivs], dtype=np.float32)

    def rows(self, thetas) -> np.ndarray:
        th = np.asarray(thetas, dtype=np.float64)
        th = th.reshape(1, -1) if th.ndim < 2 else th
        return np.stack([self.row(t) for t in th])


def _f32_of(v) -> float:
    return float(torch.as_tensor(float(v) if not isinstance(v, torch.Tensor) else v, dtype=torch.float32))


class _SmcTracer(PlanTracer):
    """PlanTracer whose observed sites read per-step observation constants."""

    def __init__(self, obs_index: dict, space: ParamSpace | None = None):
        super().__init__(ChoiceMap.empty(), 1, use_params=space is not None)
        self.obs_index = obs_index  # full address (the calls' addresses, then the site's) -> observation column
        self.space = space  # a parameterised model's slots (shared by its tracers)

    def param_slot(self, pv: ParamVal) -> int:
        if self.space is None:
            raise PlanUnsupported("a launch parameter in a model that declares none")
        return self.space.slot(pv)

    def theta_args(self) -> tuple:
        """What the bodies of a parameterised model take after their own arguments."""
        return () if self.space is None else (self.space.theta,)

    def _arg(self, v) -> abi.Arg:
        if isinstance(v, Sym) and v.src[0] == "state":
            return abi.Arg(abi.ARG_STATE, v.src[1], v.scale, v.offset, None)
        if isinstance(v, Sym) and v.src[0] == "obs":
            return abi.Arg(abi.ARG_OBS, v.src[1], v.scale, v.offset, None)
        if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.numel() > 1:
            raise PlanUnsupported("per-particle tensors cannot enter an SMC plan")
        return super()._arg(v)

    def _callee_constraint(self, a: tuple) -> ChoiceMap:
        return ChoiceMap.empty()  # (observed sites are recognised by their full address, see handle_trace)

    def handle_trace(self, addr, gen_fn, args):
        from .lang import Distribution

        local = addr if isinstance(addr, tuple) else (addr,)
        key = self.prefix + local
        if isinstance(gen_fn, Distribution) and key in self.obs_index:
            # constrain with a placeholder, then point the site's observed value at the obs vector
            self.constraint = ChoiceMap.entry(0.0, *local)
            up, self.use_params = self.use_params, False  # (the placeholder is no launch parameter)
            try:
                out = super().handle_trace(addr, gen_fn, args)
            finally:
                self.use_params = up
            k = self.obs_index[key]
            self.sites[-1].obs = abi.Arg(abi.ARG_OBS, k, 1.0, 0.0, None)
            self.constraint = ChoiceMap.empty()
            is_int = self.meta[-1]["is_int"]
            return Sym(self, ("obs", k), is_int=is_int)
        self.constraint = ChoiceMap.empty()
        out = super().handle_trace(addr, gen_fn, args)
        if isinstance(gen_fn, Distribution):  # (a nested call's own sites have passed through here already)
            self.sites[-1].out_col = -1  # SMC plans keep state columns, not per-site columns
        return out


def _state_args(tracer: _SmcTracer, ret, n_expected: int | None):
    vals = ret if isinstance(ret, (tuple, list)) else (ret,)
    if n_expected is not None and len(vals) != n_expected:
        raise PlanUnsupported("init and step must return carries of the same length")
    if not 1 <= len(vals) <= abi.SMC_MAX_STATE:
        raise PlanUnsupported(f"the carry must have 1..{abi.SMC_MAX_STATE} components")
    out = []
    for v in vals:
        if isinstance(v, _Table):
            raise PlanUnsupported("a table lookup cannot be a carry component")
        out.append(tracer._arg(v))  # (an expression over sites / the carry / observations is a postfix program)
    return out


def build_smc_plan(model: StateSpaceModel, obs_addrs: list[tuple], theta=None):
    """-> (SmcPlan, n_state).  obs_addrs: addresses (tuples) observed at every step, in the column
    order of the observation matrix.  `theta`: for a model with parameters, the values the bodies are traced at (any
    point of the parameter space: the plan's structure does not depend on it); the plan then carries `_space`
    (ParamSpace) and takes rows through `SmcPlan.set_params`."""
    if not isinstance(model.init, StaticGenerativeFunction) or not isinstance(model.step, StaticGenerativeFunction):
        raise TypeError("StateSpaceModel needs `@gen` functions")
    if len(obs_addrs) > abi.SMC_MAX_OBS:
        raise PlanUnsupported(f"at most {abi.SMC_MAX_OBS} observed addresses per step")
    obs_index = {a: k for k, a in enumerate(obs_addrs)}
    space = _param_space(model, theta)
    if space is not None:
        get_ops().lib.require("smc_params", "gjx_smc_plan_create_params")  # (before any table is built)
    ti = _SmcTracer(obs_index, space)
    init_ret = ti.run(model.init.source, ti.theta_args())
    init_state = _state_args(ti, init_ret, None)
    ts = _SmcTracer(obs_index, space)
    carry = tuple(Sym(ts, ("state", k)) for k in range(len(init_state)))
    step_ret = ts.run(model.step.source, ((carry[0],) if len(carry) == 1 else (carry,)) + ts.theta_args())
    next_state = _state_args(ts, step_ret, len(init_state))
    seen = {m["path"] for m in ti.meta + ts.meta}
    missing = [a for a in obs_addrs if a not in seen]
    if missing:
        raise ValueError(f"observed addresses not visited by the model: {missing}")
    plan = get_ops().smc_plan_create(ti.sites, ts.sites, init_state, next_state, len(obs_addrs),
                                     init_scopes=[tuple(k) for k in ti.scopes], step_scopes=[tuple(k) for k in ts.scopes],
                                     n_params=space.n_slots if space is not None else 0)
    plan._keep = (ti.keep, ts.keep)  # constant tables the site tables point into
    plan._space = space
    plan._tables = (ti.sites, ts.sites)
    plan._state_args = (init_state, next_state)
    plan._nested = bool(ti.scopes or ts.scopes)
    return plan, len(init_state)


def check_conditional(plan) -> None:
    """The model condition of the conditional step (include/gjx_csmc.h) on a lowered plan: flat bodies, and
    in both of them every sampled site (latent or proposed) is, by itself, exactly one carry component and every carry
    component is such a site — the rule `build_transition_table` enforces for backward simulation.  `PlanUnsupported`."""
    if getattr(plan, "_nested", False):
        raise PlanUnsupported("a retained path in a model with nested `@gen` calls: the conditional step needs flat bodies "
                              "(every sampled site a carry component)")
    for body, sites, state in zip(("init", "step"), plan._tables, plan._state_args):
        component_of: dict = {}
        for c, a in enumerate(state):
            plain = (a.kind == abi.ARG_SITE and a.scale == 1.0 and a.offset == 0.0 and 0 <= a.ref < len(sites)
                     and sites[a.ref].observed in (0, abi.SITE_PROPOSED))
            if not plain:
                raise PlanUnsupported(f"carry component {c} of `{body}` is not one of the body's sampled sites by itself: a retained "
                                      "path does not determine the step (the conditional filter needs every carry component to be "
                                      "a latent draw)")
            if a.ref in component_of:
                raise PlanUnsupported(f"site {a.ref} of `{body}` is returned twice (carry components {component_of[a.ref]} and {c})")
            component_of[a.ref] = c
        for q, site in enumerate(sites):
            if site.observed in (0, abi.SITE_PROPOSED) and q not in component_of:
                raise PlanUnsupported(f"the latent site {q} of `{body}` is not returned in the carry: a retained path does not "
                                      "determine it (the conditional filter needs every sampled site to be a carry component)")


def _param_space(model: StateSpaceModel, theta) -> ParamSpace | None:
    if not model.params:
        if theta is not None:
            raise ValueError("params were given for a StateSpaceModel that declares none (StateSpaceModel(init, step, params=(...)))")
        return None
    if theta is None:
        raise ValueError(f"the model declares the parameters {model.params}: pass their values (params=...)")
    return ParamSpace(model.params, theta)


class _GuidedTracer(_SmcTracer):
    """One tracer and ONE site table for a proposal and the model body it guides.  The proposal is traced first: its sites
    take table positions 0 .. n_q - 1 as PROPOSED sites (sampled like latent ones; their log-density is kept).  The model
    body is then traced into the same table: at the address of a proposed site it emits a GUIDED site that points at its
    partner, and the value the body sees from there on is the partner's value."""

    def __init__(self, obs_index: dict, space=None):
        super().__init__(obs_index, space)
        self.in_proposal = False
        self.proposed: dict = {}  # address -> table index of the proposal's site, until the model's site has taken it

    def run_proposal(self, proposal, args):
        self.in_proposal = True
        try:
            self.run(proposal.source, args)  # (the proposal's return value is ignored)
        finally:
            self.in_proposal = False
        self.traces = {}  # the model body uses the same addresses again
        self.items = []

    def unpaired(self) -> list:
        return list(self.proposed)

    def _call(self, addr, gen_fn, args):
        if self.in_proposal:
            raise PlanUnsupported(f"nested `@gen` call at address {addr!r} inside a proposal: proposals are flat bodies of distribution sites")
        a = addr if isinstance(addr, tuple) else (addr,)
        inside = [k for k in self.proposed if k[:len(self.prefix + a)] == self.prefix + a]
        if inside:
            raise PlanUnsupported(f"the proposal's site {_show(inside[0])} pairs with a model site inside the callee at {addr!r}: "
                                  "only body-level latent sites can be guided")
        raise PlanUnsupported(f"nested `@gen` call at address {addr!r} in a body of a guided model: guided plans have flat bodies "
                              "(a site inside a callee cannot be guided)")

    def handle_trace(self, addr, gen_fn, args):
        from .lang import Distribution

        if not isinstance(gen_fn, Distribution):
            return self._call(addr, gen_fn, args)
        key = self.prefix + (addr if isinstance(addr, tuple) else (addr,))
        if self.in_proposal:
            if key in self.obs_index:
                raise PlanUnsupported(f"the proposal draws the OBSERVED address {_show(key)}: only latent sites can be proposed")
            out = super().handle_trace(addr, gen_fn, args)
            self.sites[-1].observed = abi.SITE_PROPOSED
            self.proposed[key] = len(self.sites) - 1
            return out
        if key not in self.proposed:
            return super().handle_trace(addr, gen_fn, args)
        partner = self.proposed.pop(key)
        super().handle_trace(addr, gen_fn, args)  # the model's own site: its distribution and arguments
        site, me = self.sites[-1], len(self.sites) - 1
        if self.meta[me]["is_int"] != self.meta[partner]["is_int"]:
            raise PlanUnsupported(f"address {_show(key)}: the proposal's site is "
                                  f"{'integer' if self.meta[partner]['is_int'] else 'float'}-valued and the model's is "
                                  f"{'integer' if self.meta[me]['is_int'] else 'float'}-valued")
        site.observed = abi.SITE_GUIDED
        site.obs = abi.Arg(abi.ARG_SITE, partner, 1.0, 0.0, None)
        return _IntSym(self, ("site", partner)) if self.meta[partner]["is_int"] else Sym(self, ("site", partner))


def _show(key: tuple) -> str:
    return repr(key[0] if len(key) == 1 else key)


def build_guided_plan(model: StateSpaceModel, obs_addrs: list[tuple], step_proposal, init_proposal=None, theta=None):
    """-> (SmcPlan, n_state) of the guided filter: `build_smc_plan` with `step_proposal(carry, y)` (and, if given,
    `init_proposal(y)`) traced in front of the model's bodies.  `y`: this step's observation (a tuple in the order of
    `obs_addrs` when several addresses are observed).  Raises abi.GuidedUnavailable on a library without
    include/gjx_guided.h."""
    gens = [model.init, model.step, step_proposal] + ([init_proposal] if init_proposal is not None else [])
    if not all(isinstance(g, StaticGenerativeFunction) for g in gens):
        raise TypeError("GuidedSMC needs `@gen` functions for the model and the proposals")
    if len(obs_addrs) > abi.SMC_MAX_OBS:
        raise PlanUnsupported(f"at most {abi.SMC_MAX_OBS} observed addresses per step")
    ops = get_ops()
    ops.lib.require("guided", "gjx_smc_plan_create_guided")  # (before any table is built: the oracle would misread the two site modes)
    obs_index = {a: k for k, a in enumerate(obs_addrs)}
    space = _param_space(model, theta)  # (a parameterised model: every body and proposal takes `theta` last)
    if space is not None:
        ops.lib.require("smc_params", "gjx_smc_plan_create_params")

    def obs_arg(tr):
        ys = tuple(Sym(tr, ("obs", k)) for k in range(len(obs_addrs)))
        return ys[0] if len(ys) == 1 else ys

    def close(tr, what):
        if tr.unpaired():
            raise PlanUnsupported(f"the {what} proposal's site {_show(tr.unpaired()[0])} has no partner: "
                                  "the model has no body-level latent site at that address")

    ti = _GuidedTracer(obs_index, space)
    if init_proposal is not None:
        ti.run_proposal(init_proposal, (obs_arg(ti),) + ti.theta_args())
    init_ret = ti.run(model.init.source, ti.theta_args())
    close(ti, "init")
    init_state = _state_args(ti, init_ret, None)
    ts = _GuidedTracer(obs_index, space)
    carry = tuple(Sym(ts, ("state", k)) for k in range(len(init_state)))
    carry_arg = carry[0] if len(carry) == 1 else carry
    ts.run_proposal(step_proposal, (carry_arg, obs_arg(ts)) + ts.theta_args())
    step_ret = ts.run(model.step.source, (carry_arg,) + ts.theta_args())
    close(ts, "step")
    next_state = _state_args(ts, step_ret, len(init_state))
    seen = {m["path"] for m in ti.meta + ts.meta}
    missing = [a for a in obs_addrs if a not in seen]
    if missing:
        raise ValueError(f"observed addresses not visited by the model: {missing}")
    plan = ops.smc_plan_create(ti.sites, ts.sites, init_state, next_state, len(obs_addrs), guided=True,
                               n_params=space.n_slots if space is not None else 0)
    plan._keep = (ti.keep, ts.keep)
    plan._space = space
    plan._tables = (ti.sites, ts.sites)  # the lowered tables (tests and tools read the modes / references from them)
    plan._state_args = (init_state, next_state)
    plan._nested = False
    return plan, len(init_state)


# ---- the transition table of a backward-simulation smoother (include/gjx_backsim.h) --------------------------------
@dataclass
class TransitionTable:
    """f(x_{t+1} | x_t) of a state-space model as a site table: every site constrained — a latent site of the step to
    "next-state component c" (`abi.ARG_NEXT`), an observed one to its observation.  `Ops.backsim_plan_create` takes it."""
    sites: list  # [abi.Site]
    n_state: int
    n_obs: int
    keep: tuple = ()  # device tensors and expression programs the sites point into


class _TransitionTracer(_SmcTracer):
    """The model's `step` alone, flat: a site inside a callee has no carry component of its own."""

    def _call(self, addr, gen_fn, args):
        raise PlanUnsupported(f"nested `@gen` call at address {addr!r} in `step`: backward simulation needs the transition density "
                              "of a flat body (every latent site a carry component)")


def _reads_state(tracer, a: abi.Arg) -> bool:
    if a.kind == abi.ARG_STATE:
        return True
    return a.kind == abi.ARG_EXPR and any(op == abi.EXPR_STATE for op, _, _ in tracer.expr_progs[a.table])


def _renumbered(tracer, a: abi.Arg, new_index: dict, keep: list) -> abi.Arg:
    """`a` with its site references moved to the positions of the shortened table."""
    if a.kind in (abi.ARG_SITE, abi.ARG_TABLE):
        return abi.Arg(a.kind, new_index[a.ref], a.scale, a.offset, a.table)
    if a.kind == abi.ARG_EXPR:
        prog = [(op, new_index[ref] if op == abi.EXPR_SITE else ref, val) for op, ref, val in tracer.expr_progs[a.table]]
        return abi.expr_arg(prog, keep)
    return a


def build_transition_table(model: StateSpaceModel, obs_addrs: list[tuple]) -> TransitionTable:
    """The transition density of `model.step` over the CARRY, as backward simulation needs it: defined only when the carry
    IS the step's latent draws — every returned component a plain reference to a body-level latent site, every latent site
    returned exactly once, no nested calls.  The table is the step's sites with each latent site constrained to its
    next-state component; observed sites stay only if an argument reads the old state (one that depends on the new state
    alone is the same for every candidate and is dropped).  Anything else: `PlanUnsupported`, naming the address or the
    component."""
    if not isinstance(model.init, StaticGenerativeFunction) or not isinstance(model.step, StaticGenerativeFunction):
        raise TypeError("StateSpaceModel needs `@gen` functions")
    if len(obs_addrs) > abi.SMC_MAX_OBS:
        raise PlanUnsupported(f"at most {abi.SMC_MAX_OBS} observed addresses per step")
    if model.params:
        raise PlanUnsupported(f"backward simulation of a model with parameters {model.params}: transition tables hold constants "
                              "only — build the model at a fixed θ to smooth")
    obs_index = {a: k for k, a in enumerate(obs_addrs)}
    # (the carry's length is that of what `init` returns, as in build_smc_plan; the table comes from `step` alone)
    ti = _SmcTracer(obs_index)
    n_state = len(_state_args(ti, ti.run(model.init.source, ()), None))
    tr = _TransitionTracer(obs_index)
    carry = tuple(Sym(tr, ("state", k)) for k in range(n_state))
    ret = tr.run(model.step.source, (carry[0],) if n_state == 1 else (carry,))
    vals = ret if isinstance(ret, (tuple, list)) else (ret,)
    if len(vals) != n_state:
        raise PlanUnsupported("init and step must return carries of the same length")
    component_of: dict = {}  # latent site -> the carry component that returns it
    for c, v in enumerate(vals):
        plain = (isinstance(v, Sym) and v.src[0] == "site" and v.scale == 1.0 and v.offset == 0.0
                 and not v.has_mul and not v.has_add and tr.sites[v.src[1]].observed == 0)
        if not plain:
            raise PlanUnsupported(f"carry component {c} of `step` is an expression, not one of the step's latent draws: the "
                                  "transition is degenerate (it has no density over the carry), so backward simulation is "
                                  "undefined for this model")
        q = v.src[1]
        if q in component_of:
            raise PlanUnsupported(f"the latent site {_show(tr.meta[q]['path'])} is returned twice (carry components "
                                  f"{component_of[q]} and {c}): the transition is degenerate")
        component_of[q] = c
    for q, site in enumerate(tr.sites):
        if site.observed == 0 and q not in component_of:
            raise PlanUnsupported(f"the latent site {_show(tr.meta[q]['path'])} is not returned in the carry: the transition "
                                  "density over the carry would need it integrated out")
    kept = [q for q, site in enumerate(tr.sites)
            if site.observed == 0 or _reads_state(tr, site.arg[0]) or (site.dist != abi.DIST_BERNOULLI and site.dist != abi.DIST_CATEGORICAL
                                                                    and _reads_state(tr, site.arg[1]))]
    new_index = {q: k for k, q in enumerate(kept)}
    keep: list = list(tr.keep)
    sites = []
    for q in kept:
        site = abi.Site.from_buffer_copy(tr.sites[q])
        for k in range(2):
            site.arg[k] = _renumbered(tr, tr.sites[q].arg[k], new_index, keep)
        if site.observed == 0:
            site.observed = 1
            site.obs = abi.Arg(abi.ARG_NEXT, component_of[q], 1.0, 0.0, None)
        site.out_col = -1
        sites.append(site)
    return TransitionTable(sites, n_state, len(obs_addrs), tuple(keep))


def observation_matrix(observations, obs_addrs: list[tuple]) -> np.ndarray:
    """[T, n_obs] float32 from a ChoiceMap whose observed leaves are length-T vectors."""
    cols = []
    for a in obs_addrs:
        v = observations[a if len(a) > 1 else a[0]]
        cols.append(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float32).reshape(-1))
    T = cols[0].shape[0]
    if any(c.shape[0] != T for c in cols):
        raise ValueError("all observed sequences must have the same length")
    return np.stack(cols, axis=1)
