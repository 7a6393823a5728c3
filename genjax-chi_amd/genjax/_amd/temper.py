"""Tempered SMC for static `@gen` models (include/gjx_temper.h).

`TemperedSMC(target, n_particles)` walks a population from the prior of a static model to its posterior through the targets
prior * likelihood^beta: every stage reweights by likelihood^(beta' - beta), resamples systematically and moves each particle
with `n_moves` random-walk Metropolis-Hastings sweeps — the resampling gather and the sweeps are ONE launch
(gjx_temper_move), and the next temperature is chosen from two one-launch ESS ladders (gjx_temper_ess_ladder) instead of a
host bisection.  It needs no gradients and returns posterior samples AND log Z where the prior-proposal estimators
(ImportanceK) have collapsed: a posterior much narrower than the prior."""

from __future__ import annotations

import math

import numpy as np
import torch

from . import abi, prng
from .choicemap import ChoiceMap
from .inference import ParticleCollection, SMCAlgorithm, Target
from .lang import NegativeBinomial, Poisson, bernoulli, split
from .plan import ParamVal, PlanTracer, PlanUnsupported, SymExpr, _DIST_IDS, _make_plan, _needs_eager, is_data_tensor
from .runtime import get_ops

LADDER = 32  # candidates per ladder launch


class GroupTensorRefused(PlanUnsupported):
    """The group tensor of a grouped latent — the values it holds NOW — cannot be lowered: unsorted, out of 0 .. G-1, or not
    of the plate's length.  A PlanUnsupported for `lower()` and `run()`; a held-out target's is reported as a ValueError
    (TemperedSMC._lower_held_out catches this class, not a message)."""


class _GroupVal:
    """The traced value of a GROUPED site (include/gjx_group.h): G components.  It supports exactly one operation, indexing by
    the group tensor — a 1-D integer tensor of the plate length, the group of every data row: `a[g]` is the component of
    the row's group, a program leaf (abi.EXPR_GROUP) of a plated site's arguments."""

    def __init__(self, tracer, ref: int, addr):
        self.tracer, self.ref, self.addr = tracer, ref, addr

    def __getitem__(self, idx):
        if not (isinstance(idx, torch.Tensor) and idx.dim() == 1 and idx.numel() >= 2 and not idx.is_floating_point()
                and not idx.is_complex() and idx.dtype != torch.bool):
            raise PlanUnsupported(f"TemperedSMC: the grouped latent at address {self.addr!r} can only be indexed by a 1-D integer "
                                  "tensor of the plate length (the group of every data row)")
        self.tracer.group_tensor(idx, self.addr)
        return SymExpr(self.tracer, [(abi.EXPR_GROUP, self.ref, 0.0)])

    def _no(self, *a, **k):
        raise PlanUnsupported(f"TemperedSMC: the grouped latent at address {self.addr!r} supports indexing by the group tensor "
                              "only (a[g] inside a plated site)")

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __neg__ = __pow__ = _no
    __lt__ = __le__ = __gt__ = __ge__ = __iter__ = __len__ = __float__ = __bool__ = _no
    exp = log = sqrt = abs = sum = mean = _no

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        next(a for a in args if isinstance(a, _GroupVal))._no()


class _TemperTracer(PlanTracer):
    """PlanTracer that names the address of whatever a tempered plan cannot hold.

    PLATED sites (include/gjx_plate.h).  In a tempered plan a 1-D tensor with two or more elements is always DATA — a
    column of the data table, never a per-particle column (PlanTracer's reading of a length-n tensor does not apply: a
    tempered plan has none).  A tensor becomes a column the first time it meets a traced value (`w * xs`: a program with a
    DATA leaf, plan.SymExpr.program_of) or a site (an argument or the observed value); columns are deduplicated by the
    tensor's memory and version.  A site with a data-dependent argument or value is ONE plated site."""

    def __init__(self, constraint, n, use_params=True):
        super().__init__(constraint, n, use_params)
        self.data: list = []      # the data columns, as the model handed them over (uploaded as f32 at every run)
        self._data_keys: dict = {}
        self.data_rows = None     # D: one length per plan
        # COUNT sites (include/gjx_counts.h): the column after a plated count site's observed column holds log k!,
        # float32 of the float64 lgamma(k + 1) — data, not arithmetic.  lf_cols: that column -> the observed one
        self.lf_cols: dict = {}
        self._count_keys: dict = {}
        # GROUPED sites (include/gjx_group.h): the group tensor (one per plan: NOT a data column), its identity, G
        self.group = None
        self._group_key = None
        self.n_groups = None
        self.n_grouped = 0

    def data_col(self, t: torch.Tensor) -> int:
        # (identity is the memory: the body sees its tensor arguments as SpecTensor views of the caller's)
        key = (t.data_ptr(), t.numel(), t.stride(0), t.dtype, str(t.device), t._version)
        c = self._data_keys.get(key)
        if c is None:
            c = self._data_keys[key] = len(self.data)
            self.data.append(t)
        return c

    @staticmethod
    def log_factorial(t: torch.Tensor, addr=None) -> torch.Tensor:
        """float32 of the float64 lgamma(rint(k) + 1) of a column of observed counts; a count above 2^24 is refused."""
        k = torch.round(t.detach().to(device="cpu", dtype=torch.float64))
        if k.numel() and float(k.max()) > abi.COUNTS_MAX_OBSERVED:
            at = "" if addr is None else f" at address {addr!r}"
            raise PlanUnsupported(f"TemperedSMC: an observed count of {int(k.max())}{at} is above 2^24 (not exact in float32)")
        return torch.lgamma(k.clamp_min(0.0) + 1.0).to(torch.float32)

    def count_cols(self, obs: torch.Tensor, addr) -> int:
        """The observed column of a plated count site, with its log k! column registered directly after it.  (A pair of its
        own even where the tensor is a column already: that column's neighbour is taken.)"""
        key = (obs.data_ptr(), obs.numel(), obs.stride(0), obs.dtype, str(obs.device), obs._version)
        c = self._count_keys.get(key)
        if c is None:
            c = self._count_keys[key] = len(self.data)
            self._data_keys.setdefault(key, c)
            self.data.append(obs)
            self.data.append(self.log_factorial(obs, addr))
            self.lf_cols[c + 1] = c
        return c

    def group_tensor(self, t: torch.Tensor, addr):
        """Registers the tensor the grouped values are indexed by: one per plan (identity is memory plus version, as data_col's)."""
        key = (t.data_ptr(), t.numel(), t.stride(0), t.dtype, str(t.device), t._version)
        if self._group_key is None:
            self.group, self._group_key = t, key
            self.group_offsets(addr)  # (validated here, and again at every run)
        elif key != self._group_key:
            raise PlanUnsupported(f"TemperedSMC: the grouped latent at address {addr!r} is indexed by another group tensor than "
                                  "the one before it (one group tensor per plan)")
        if self.data_rows is not None and self.data_rows != t.numel():
            raise GroupTensorRefused(f"TemperedSMC: the group tensor of the grouped latent at address {addr!r} has {t.numel()} entries, "
                                  f"the plate {self.data_rows} rows")

    def group_offsets(self, addr=None) -> torch.Tensor:
        """The group tensor as it is NOW -> offsets int32 [G + 1] (host): group k owns the rows offsets[k] .. offsets[k + 1] - 1.
        Refused unless non-decreasing with values in 0 .. G - 1; empty groups are legal."""
        if addr is None:
            addr = next(m["addr"] for m in self.meta if m.get("grouped"))
        g = self.group.detach().to(device="cpu", dtype=torch.int64)
        G = self.n_groups
        if int(g.min()) < 0 or int(g.max()) >= G:
            raise GroupTensorRefused(f"TemperedSMC: the group tensor of the grouped latent at address {addr!r} has values outside 0 .. {G - 1}")
        if bool((g[1:] < g[:-1]).any()):
            raise GroupTensorRefused(f"TemperedSMC: the group tensor of the grouped latent at address {addr!r} is not sorted (the rows of "
                                  "a group must be contiguous: non-decreasing group indices)")
        off = torch.zeros(G + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.bincount(g, minlength=G), dim=0)
        return off.to(torch.int32)

    @staticmethod
    def _reads_group(v) -> bool:
        return isinstance(v, SymExpr) and any(op == abi.EXPR_GROUP for op, _, _ in v.prog)

    def _grouped(self, addr, gen_fn, args, obs):
        """One GROUPED site: `dist(*args).repeat(n=G) @ addr`, latent, G i.i.d. components given the scalar latents."""
        inner, G = gen_fn.gen_fn, gen_fn.axis_size
        dist = _DIST_IDS.get(id(inner))
        if dist is None or dist > abi.DIST_BETA:
            raise PlanUnsupported(f"TemperedSMC: the grouped site at address {addr!r} must be normal, gamma or beta (a random-walk "
                                  "move needs a float value)")
        if obs is not None:
            raise PlanUnsupported(f"TemperedSMC: the grouped site at address {addr!r} is observed (a grouped site is a latent)")
        vals = list(args)[:2]
        for v in vals:
            if isinstance(v, _GroupVal) or self._reads_group(v):
                raise PlanUnsupported(f"TemperedSMC: an argument of the grouped site at address {addr!r} reads a grouped latent "
                                      "(grouped sites that depend on each other are not supported)")
            if self._data_cols_of(v) or (isinstance(v, torch.Tensor) and v.dim() >= 1 and v.numel() > 1):
                raise PlanUnsupported(f"TemperedSMC: an argument of the grouped site at address {addr!r} reads data (its components "
                                      "are i.i.d. given the scalar latents)")
        if not isinstance(G, int) or not 1 <= G < abi.GROUP_MAX_GROUPS:
            raise PlanUnsupported(f"TemperedSMC: the grouped site at address {addr!r} has G = {G!r} (1 <= G < 2^24)")
        if self.n_groups is not None and G != self.n_groups:
            raise PlanUnsupported(f"TemperedSMC: the grouped site at address {addr!r} has G = {G}, the one before it G = {self.n_groups} "
                                  "(one G per plan)")
        if self.n_grouped >= abi.GROUP_MAX_SITES:
            raise PlanUnsupported(f"TemperedSMC: more than {abi.GROUP_MAX_SITES} grouped sites at address {addr!r}")
        if len(self.sites) >= abi.MAX_SITES:
            raise PlanUnsupported(f"TemperedSMC: too many sites at address {addr!r}")
        self.n_groups = G
        site = abi.Site()
        site.dist, site.observed, site.out_col = dist, abi.SITE_GROUPED, -1
        for k, v in enumerate(vals):
            site.arg[k] = self._arg(v)
        self.sites.append(site)
        self.items.append(("site", len(self.sites) - 1))
        self.meta.append(dict(addr=addr, gen_fn=gen_fn, args=args, obs=None, out_col=-1, is_int=False, dtype=inner.value_dtype,
                              path=self.prefix + (addr if isinstance(addr, tuple) else (addr,)), grouped=True))
        self.record(addr, None)
        self.n_grouped += 1
        return _GroupVal(self, self.n_grouped - 1, addr)

    def data_columns(self, device) -> list:
        """The columns as float32 device tensors, as they are NOW: read at every run, the log k! columns recomputed."""
        cols = [(self.log_factorial(self.data[self.lf_cols[c]]) if c in self.lf_cols else t.detach()) for c, t in enumerate(self.data)]
        return [t.to(device=device, dtype=torch.float32).contiguous() for t in cols]

    def _lowered(self, kind, v):
        """An argument of a count family on its unconstrained scale as the program the per-site route computes (lang._CountDist):
        log_rate -> exp(v); logits -> 1 / (1 + exp(-v))."""
        if kind in ("rate", "probs"):
            return v
        _, prog = SymExpr.program_of(v, self)
        z = (0, 0.0)
        if kind == "log_rate":
            return SymExpr(self, prog + [(abi.EXPR_EXP, *z)])
        return SymExpr(self, [(abi.EXPR_CONST, 0, 1.0)] + prog + [(abi.EXPR_NEG, *z), (abi.EXPR_EXP, *z), (abi.EXPR_CONST, 0, 1.0),
                                                                   (abi.EXPR_ADD, *z), (abi.EXPR_DIV, *z)])

    def _count_family(self, gen_fn, args):
        """-> (dist id, [a0, a1]) of a Poisson / NegativeBinomial site (canonical arguments), or None."""
        if isinstance(gen_fn, Poisson):
            kind, v = args[0]
            return abi.DIST_POISSON, [self._lowered(kind, v)]
        if isinstance(gen_fn, NegativeBinomial):
            kind, v = args[1]
            return abi.DIST_NEGATIVE_BINOMIAL, [args[0], self._lowered(kind, v)]
        return None

    def _observed_count(self, addr, gen_fn, args, obs):
        """A scalar OBSERVED count site (gjx_counts.h: log k! is evaluated in the kernel, once per particle and sweep)."""
        if len(self.sites) >= abi.MAX_SITES:
            raise PlanUnsupported(f"TemperedSMC: too many sites at address {addr!r}")
        try:
            k = float(obs)
        except Exception:
            raise PlanUnsupported(f"TemperedSMC: the observed count at address {addr!r} must be a number or a 1-D tensor") from None
        if k > abi.COUNTS_MAX_OBSERVED:
            raise PlanUnsupported(f"TemperedSMC: an observed count of {int(k)} at address {addr!r} is above 2^24 (not exact in float32)")
        dist, vals = self._count_family(gen_fn, args)
        site = abi.Site()
        site.dist, site.observed, site.out_col = dist, 1, -1
        for j, v in enumerate(vals):
            site.arg[j] = self._arg(v)
        if self.use_params:
            site.obs = abi.Arg(abi.ARG_PARAM, self.param_slot(ParamVal(k)), 1.0, 0.0, None)
        else:
            site.obs = abi.Arg(abi.ARG_CONST, 0, 0.0, k, None)
        self.sites.append(site)
        self.items.append(("site", len(self.sites) - 1))
        self.meta.append(dict(addr=addr, gen_fn=gen_fn, args=args, obs=obs, out_col=-1, is_int=True, dtype=gen_fn.value_dtype,
                              path=self.prefix + (addr if isinstance(addr, tuple) else (addr,))))
        self.record(addr, None)
        return obs

    def _data_cols_of(self, v) -> set:
        """The data columns the argument / value `v` reads (a raw data tensor is registered here)."""
        if is_data_tensor(v):
            return {self.data_col(v)}
        if isinstance(v, SymExpr):
            return {ref for op, ref, _ in v.prog if op == abi.EXPR_DATA}
        return set()

    def _arg(self, v) -> abi.Arg:
        if is_data_tensor(v):
            return abi.Arg(abi.ARG_DATA, self.data_col(v), 1.0, 0.0, None)
        if isinstance(v, SymExpr) and len(v.prog) == 1 and v.prog[0][0] == abi.EXPR_GROUP:  # (`a[g]` itself: the affine operand)
            return abi.Arg(abi.ARG_GROUP, v.prog[0][1], 1.0, 0.0, None)
        return super()._arg(v)

    def _call(self, addr, gen_fn, args):
        raise PlanUnsupported(f"TemperedSMC: nested generative function at address {addr!r}")

    def _plated(self, addr, gen_fn, args, obs, cols: set):
        """One PLATED site: `gen_fn(*args) @ addr` with data-dependent arguments and / or a data column as its value."""
        if obs is None:
            raise PlanUnsupported(f"TemperedSMC: the latent at address {addr!r} depends on data (a vector-valued latent)")
        if not is_data_tensor(obs):
            raise PlanUnsupported(f"TemperedSMC: the site at address {addr!r} has data-dependent arguments: its observed value "
                                  "must be a 1-D tensor of the same length")
        count = isinstance(gen_fn, (Poisson, NegativeBinomial))
        if count:
            dist, vals = self._count_family(gen_fn, args)
        elif id(gen_fn) in _DIST_IDS:
            dist = _DIST_IDS[id(gen_fn)]
            vals = list(args[:1 if dist == abi.DIST_BERNOULLI else 2])
        elif gen_fn is bernoulli and args[0][0] == "probs":
            dist, vals = abi.DIST_BERNOULLI, [args[0][1]]
        else:
            raise PlanUnsupported(f"TemperedSMC: a plated site at address {addr!r} must be normal, gamma, beta, flip, poisson or "
                                  "negative_binomial (a plated categorical has no table rows per datum)")
        if len(self.sites) >= abi.MAX_SITES:
            raise PlanUnsupported(f"TemperedSMC: too many sites at address {addr!r}")
        # (a count site's observed column brings its log k! column, directly after it: include/gjx_counts.h)
        obs_col = self.count_cols(obs, addr) if count else self.data_col(obs)
        cols = cols | {obs_col}
        lengths = {int(self.data[c].numel()) for c in cols} | ({self.data_rows} if self.data_rows is not None else set())
        if self.group is not None:
            lengths |= {int(self.group.numel())}
        if len(lengths) != 1:
            raise PlanUnsupported(f"TemperedSMC: data columns of different lengths {sorted(lengths)} at address {addr!r} "
                                  "(one plate length per plan)")
        if len(self.data) > abi.PLATE_MAX_COLS:
            raise PlanUnsupported(f"TemperedSMC: {len(self.data)} data columns (at most {abi.PLATE_MAX_COLS}) at address {addr!r}")
        self.data_rows = lengths.pop()
        site = abi.Site()
        site.dist, site.observed, site.out_col = dist, abi.SITE_PLATED, -1
        for k, v in enumerate(vals):
            site.arg[k] = self._arg(v)
        site.obs = abi.Arg(abi.ARG_DATA, obs_col, 1.0, 0.0, None)
        self.sites.append(site)
        self.items.append(("site", len(self.sites) - 1))
        self.meta.append(dict(addr=addr, gen_fn=gen_fn, args=args, obs=obs, out_col=-1, is_int=dist >= abi.DIST_BERNOULLI,
                              dtype=gen_fn.value_dtype, path=self.prefix + (addr if isinstance(addr, tuple) else (addr,)),
                              plated=True))
        self.record(addr, None)
        return obs  # (a constrained value may feed later sites: it is data there too)

    def handle_trace(self, addr, gen_fn, args):
        from .combinators import Vmap
        from .lang import Categorical, Distribution

        flat = [x for v in args for x in (v if isinstance(v, tuple) else (v,))]
        if isinstance(gen_fn, Vmap) and gen_fn.in_axes is None and gen_fn.axis_size is not None and isinstance(gen_fn.gen_fn, Distribution):
            a = addr if isinstance(addr, tuple) else (addr,)
            sub = self.constraint.get_submap(*a)
            return self._grouped(addr, gen_fn, args, None if sub.static_is_empty() and sub.get_value() is None else sub)
        used = next((v for v in flat if isinstance(v, _GroupVal)), None)
        if used is not None:
            raise PlanUnsupported(f"TemperedSMC: the site at address {addr!r} takes the grouped latent at address {used.addr!r} whole; "
                                  "a grouped value can only be read as a[g] inside a plated site")
        if isinstance(gen_fn, Distribution):
            a = addr if isinstance(addr, tuple) else (addr,)
            obs = self.constraint.get_submap(*a).get_value()
            if isinstance(gen_fn, (Poisson, NegativeBinomial)):
                if obs is None:
                    raise PlanUnsupported(f"TemperedSMC: count-valued latent at address {addr!r} (a random-walk move needs a float value)")
                if not is_data_tensor(obs):
                    if set().union(*[self._data_cols_of(v) for v in flat]):
                        return self._plated(addr, gen_fn, args, obs, set())  # (refused there, naming the address)
                    return self._observed_count(addr, gen_fn, args, obs)
            # (a categorical's 1-D tensor argument is its logits / probs vector, not data)
            cols = set().union(*[self._data_cols_of(v) for v in flat]) if flat and not isinstance(gen_fn, Categorical) else set()
            if cols or is_data_tensor(obs) or any(self._reads_group(v) for v in flat):
                return self._plated(addr, gen_fn, args, obs, cols)
        try:
            out = super().handle_trace(addr, gen_fn, args)
        except PlanUnsupported as e:
            if "at address" in str(e):
                raise
            raise PlanUnsupported(f"TemperedSMC: {e} at address {addr!r} (a vector-valued or otherwise unsupported site)") from None
        m = self.meta[-1]
        if m["obs"] is None and m["is_int"]:
            raise PlanUnsupported(f"TemperedSMC: integer-valued latent at address {addr!r} (a random-walk move needs a float value)")
        if self.inputs:
            raise PlanUnsupported(f"TemperedSMC: per-particle column at address {addr!r}")
        return out


def lower(target: Target, n: int):
    """-> the tracer of the target's body as a flat site table (the tracing ImportanceK uses), observations and scalar
    arguments as launch parameters.  PlanUnsupported, naming the address, for what a tempered plan cannot hold."""
    from .lang import StaticGenerativeFunction

    if not isinstance(target.p, StaticGenerativeFunction):
        raise PlanUnsupported("TemperedSMC: the target's model must be a static @gen function")
    if any(_needs_eager(a) and not is_data_tensor(a) for a in target.args):  # (a 1-D tensor is a data column)
        raise PlanUnsupported("TemperedSMC: the target's arguments need the per-site path")
    constraint = target.constraint.merge(ChoiceMap.empty())
    last = None
    for use_params in (True, False):
        tracer = _TemperTracer(constraint, n, use_params)
        try:
            tracer.run(target.p.source, tracer.wrap_args(target.args))
        except PlanUnsupported as e:
            if "at address" in str(e):
                raise
            last = e
            continue
        except Exception as e:  # symbolic values fed to code that expects tensors: retried with constants
            last = PlanUnsupported(f"TemperedSMC: the body is not plan-able ({type(e).__name__}: {e})")
            continue
        addrs = [m["addr"] for m in tracer.meta]
        if not any(m["obs"] is None and not m.get("grouped") for m in tracer.meta):
            raise PlanUnsupported(f"TemperedSMC: no {'scalar ' if tracer.n_grouped else ''}latent site among the addresses {addrs!r}")
        if tracer.n_grouped and tracer.group is None:
            at = next(m["addr"] for m in tracer.meta if m.get("grouped"))
            raise PlanUnsupported(f"TemperedSMC: the grouped latent at address {at!r} is read by no plated site (a[g] in a site observed "
                                  "over a data column)")
        if tracer.n_grouped and tracer.data_rows != tracer.group.numel():
            at = next(m["addr"] for m in tracer.meta if m.get("grouped"))
            raise GroupTensorRefused(f"TemperedSMC: the group tensor of the grouped latent at address {at!r} has {tracer.group.numel()} "
                                  f"entries, the plate {tracer.data_rows} rows")
        if all(m["obs"] is None for m in tracer.meta):
            raise PlanUnsupported(f"TemperedSMC: no observed site among the addresses {addrs!r}")
        if len(tracer.data) > abi.PLATE_MAX_COLS:  # (columns met after the last plated site)
            raise PlanUnsupported(f"TemperedSMC: {len(tracer.data)} data columns (at most {abi.PLATE_MAX_COLS}) at address {addrs[-1]!r}")
        n_lat = sum(m["obs"] is None and not m.get("grouped") for m in tracer.meta)
        if n_lat > abi.TEMPER_MAX_LATENTS:
            raise PlanUnsupported(f"TemperedSMC: {n_lat} latents (at most {abi.TEMPER_MAX_LATENTS}); the last is at address "
                                  f"{[m['addr'] for m in tracer.meta if m['obs'] is None and not m.get('grouped')][-1]!r}")
        return tracer
    raise last


class _PriorTable:
    """What plan._make_plan reads of a tracer: the table of a plated plan without its plated sites."""

    def __init__(self, tracer, sites, expr_progs, keep):
        self.sites, self.expr_progs, self.keep = sites, expr_progs, keep
        self.scopes, self.params, self.n_out = tracer.scopes, tracer.params, tracer.n_out


def prior_table(tracer) -> _PriorTable:
    """The importance table that draws stage 0 of a plated plan: its sites in order, the plated ones left out, every
    reference to an earlier site renumbered (no site reads a plated one: its value is data)."""
    new_of, sites, progs, keep = {}, [], {}, list(tracer.keep)
    for q, s in enumerate(tracer.sites):
        if s.observed in (abi.SITE_PLATED, abi.SITE_GROUPED) or (s.observed and s.dist in abi.COUNT_DISTS):  # (nor an observed count
            continue                                          # site: the importance kernels do not know the ids; nor a grouped one)
        new_of[q] = len(sites)
        c = abi.Site.from_buffer_copy(s)
        for k in range(2):
            a = c.arg[k]
            if a.kind in (abi.ARG_SITE, abi.ARG_TABLE):
                a.ref = new_of[a.ref]
            elif a.kind == abi.ARG_EXPR:
                prog = [(op, new_of[ref] if op == abi.EXPR_SITE else ref, val) for op, ref, val in tracer.expr_progs[a.table]]
                c.arg[k] = abi.expr_arg(prog, keep)
                progs[c.arg[k].table] = tuple(prog)
        sites.append(c)
    return _PriorTable(tracer, sites, progs, keep)


def _reads_value_of(base, other, addr):
    """The address of the first plated site that reads the VALUE of the plated site at `addr` — its observed column itself, or a
    data column computed from it — or None.  `base` and `other`: two lowerings of one body over the same arguments that differ
    in the value observed at `addr` alone: a column that is no site's observed column and differs between them was computed
    from that value."""
    assert len(base.sites) == len(other.sites) and len(base.data) == len(other.data)
    observed = {s.obs.ref: m["addr"] for s, m in zip(base.sites, base.meta) if s.observed == abi.SITE_PLATED}
    tainted = {c for c, a in observed.items() if a == addr}
    # (a count site's log k! column belongs to its observed column: it is not "computed from the value" by the body)
    tainted |= {c for c, (t, u) in enumerate(zip(base.data, other.data))
                if c not in observed and c not in base.lf_cols and not torch.equal(t, u)}
    for s, m in zip(base.sites, base.meta):
        if s.observed != abi.SITE_PLATED or m["addr"] == addr:
            continue
        for k in range(2):
            a = s.arg[k]
            cols = ({a.ref} if a.kind == abi.ARG_DATA else
                    {ref for op, ref, _ in base.expr_progs[a.table] if op == abi.EXPR_DATA} if a.kind == abi.ARG_EXPR else set())
            if cols & tainted:
                return m["addr"]
    return None


def ladder_deltas(beta: float, lo=None, hi=None):
    """The candidates of one ladder launch, float32.  Coarse (lo is None): delta_j = (1 - beta) 2^-(G - 1 - j); fine:
    delta_k = lo + (hi - lo) k / G."""
    G = LADDER
    if lo is None:
        span = np.float32(np.float32(1.0) - np.float32(beta))
        return (span * np.exp2(-np.arange(G - 1, -1, -1, dtype=np.float64))).astype(np.float32)
    return (np.float64(lo) + (np.float64(hi) - np.float64(lo)) * np.arange(G, dtype=np.float64) / G).astype(np.float32)


def ess_of(s1, s2):
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    return np.where(s2 > 0.0, s1 * s1 / np.where(s2 > 0.0, s2, 1.0), 0.0)


def next_beta(beta: float, need: float, ess_fn):
    """The schedule rule: the largest candidate step whose increment keeps ESS >= need, from a coarse
    geometric ladder and a linear one between its bracketing candidates.  `ess_fn(deltas f32[G]) -> ESS float64[G]` is one
    ladder launch.  -> (beta' as a float32 value, its ESS)."""
    b = np.float32(beta)
    coarse = ladder_deltas(beta)
    ess = ess_fn(coarse)
    if ess[-1] >= need:
        return 1.0, float(ess[-1])
    ok = np.nonzero(ess >= need)[0]
    if ok.size == 0:
        step, e = coarse[0], float(ess[0])
    else:
        j = int(ok[-1])
        fine = ladder_deltas(beta, coarse[j], coarse[j + 1])
        ess2 = ess_fn(fine)
        ok2 = np.nonzero(ess2 >= need)[0]
        k = int(ok2[-1]) if ok2.size else 0
        step, e = fine[k], float(ess2[k])
    nb = np.float32(b + np.float32(step))
    if not nb > b:
        nb = np.nextafter(b, np.float32(2.0))
    return (1.0 if nb >= np.float32(1.0) else float(nb)), e


class TemperedResult:
    """What `TemperedSMC.run` returns.  `choices`: the final, equally weighted population's latent columns as a ChoiceMap;
    `lp`, `ll`: its log-prior and log-likelihood columns (f32[n], on the device).  Under `proposal="covariance"`, `factor`:
    the last stage's proposal factor, f32 [L, L], lower-triangular, on the device; `n_degenerate`: per stage, the latents
    whose row of the factor fell back to the diagonal rule (include/gjx_temper_cov.h).  Both None on the diagonal route."""

    def __init__(self, log_marginal_likelihood, betas, ess, accept_rate, choices, lp, ll, columns, factor=None, n_degenerate=None):
        self.log_marginal_likelihood, self.betas, self.ess, self.accept_rate = log_marginal_likelihood, betas, ess, accept_rate
        self.choices, self.lp, self.ll, self.columns = choices, lp, ll, columns
        self.factor, self.n_degenerate = factor, n_degenerate
        # a plan with grouped latents (include/gjx_group.h): per stage, the accepted group moves over n * n_moves * G; the S
        # grouped columns f32 [G, n] (also in `choices`, at their addresses).  None otherwise
        self.accept_rate_groups, self.group_columns = None, None

    def __repr__(self):
        return (f"TemperedResult(log_marginal_likelihood={self.log_marginal_likelihood:.6f}, stages={len(self.betas) - 1}, "
                f"n={self.lp.numel()})")


class PointwiseLikelihood:
    """Per data row d of a plated site, over the n equally weighted particles of a population (include/gjx_pointwise.h):
    `lppd` = log (1/n) sum_i p(y_d | x_i), `mean` and `var` the sample mean and (n - 1) variance of log p(y_d | x_i), `count`
    the particles with a density above 0.  float64 tensors of length D on the device; the scalar properties read them
    from the host ONCE.  WAIC as Watanabe 2010 / Gelman, Hwang & Vehtari 2014 write it: elpd_waic = sum_d (lppd_d - var_d)."""

    def __init__(self, table: torch.Tensor, n: int):
        """`table`: float64 [4, D] — the rows lse, s1, s2, c of gjx_temper_pointwise; `n`: the population size."""
        if table.dim() != 2 or table.shape[0] != 4 or table.dtype != torch.float64:
            raise ValueError("PointwiseLikelihood: a float64 [4, D] tensor expected")
        self.n = int(n)
        if self.n < 1:
            raise ValueError("PointwiseLikelihood: n >= 1")
        lse, s1, s2, self.count = table.unbind(0)
        self.lppd = lse - math.log(self.n)
        self.mean = s1 / self.n
        self.var = (s2 - s1 * s1 / self.n) / (self.n - 1) if self.n > 1 else torch.zeros_like(s1)
        self._host = None

    def _scalars(self):
        if self._host is None:
            h = torch.stack([self.lppd, self.var]).cpu().numpy()  # (the one host read)
            lppd, var = h[0], h[1]
            with np.errstate(invalid="ignore"):
                pw = lppd - var
                D = len(pw)
                se = math.sqrt(D * float(np.var(pw, ddof=1))) if D > 1 else float("nan")
            self._host = dict(lpd=float(lppd.sum()), p_waic=float(var.sum()), elpd=float(pw.sum()), se=se)
        return self._host

    @property
    def log_predictive_density(self) -> float:
        return self._scalars()["lpd"]

    @property
    def p_waic(self) -> float:
        return self._scalars()["p_waic"]

    @property
    def elpd_waic(self) -> float:
        return self._scalars()["elpd"]

    @property
    def waic(self) -> float:
        return -2.0 * self._scalars()["elpd"]

    @property
    def elpd_waic_se(self) -> float:
        """sqrt(D * var_d(lppd_d - var_d)), the sample variance over the rows (NaN for one row)."""
        return self._scalars()["se"]

    def __repr__(self):
        return f"PointwiseLikelihood(rows={self.lppd.numel()}, n={self.n})"


class PSISLOO:
    """Pareto-smoothed importance-sampling leave-one-out cross-validation of a plated site's rows under a population of n
    equally weighted particles (include/gjx_psis.h; Vehtari, Gelman & Gabry 2017).  Per data row d, float64 [D] on the device:
    `elpd_loo` (NaN where the row has a non-finite entry), `khat` — the shape of the generalised Pareto fitted to the row's
    `tail_len` largest importance ratios (+inf where nothing was smoothed: a tail tied with its cutoff, or a non-finite
    entry), `sigma` its scale, `bad` the count of non-finite entries.  `pointwise`: the PointwiseLikelihood of the same
    population (lppd, WAIC).  The scalar properties read the device ONCE: `elpd` = sum_d elpd_loo_d, `se` =
    sqrt(D var_d(elpd_loo_d)), `looic` = -2 elpd, `p_loo` = sum_d (lppd_d - elpd_loo_d), `khat_threshold` =
    min(1 - 1 / log10(n), 0.7) (Vehtari et al. 2024) and `n_high`, the rows whose khat is above it."""

    def __init__(self, table: torch.Tensor, pointwise: PointwiseLikelihood, n: int, tail_len: int):
        """`table`: float64 [7, D] — the rows elpd_loo, khat, sigma, s, tT, B, bad of gjx_temper_psis."""
        if table.dim() != 2 or table.shape[0] != 7 or table.dtype != torch.float64:
            raise ValueError("PSISLOO: a float64 [7, D] tensor expected")
        self.n, self.tail_len, self.pointwise = int(n), int(tail_len), pointwise
        if self.n < 2:
            raise ValueError("PSISLOO: n >= 2")
        self.elpd_loo, self.khat, self.sigma, self.bad = table[0], table[1], table[2], table[6]
        self.khat_threshold = min(1.0 - 1.0 / math.log10(self.n), 0.7)
        self._host = None

    def _scalars(self):
        if self._host is None:
            h = torch.stack([self.elpd_loo, self.khat, self.pointwise.lppd]).cpu().numpy()  # (the one host read)
            e, k, lppd = h[0], h[1], h[2]
            D = len(e)
            with np.errstate(invalid="ignore"):
                se = math.sqrt(D * float(np.var(e, ddof=1))) if D > 1 else float("nan")
                self._host = dict(elpd=float(e.sum()), se=se, p_loo=float((lppd - e).sum()), n_high=int((k > self.khat_threshold).sum()))
        return self._host

    @property
    def elpd(self) -> float:
        return self._scalars()["elpd"]

    @property
    def se(self) -> float:
        return self._scalars()["se"]

    @property
    def looic(self) -> float:
        return -2.0 * self._scalars()["elpd"]

    @property
    def p_loo(self) -> float:
        return self._scalars()["p_loo"]

    @property
    def n_high(self) -> int:
        return self._scalars()["n_high"]

    def __repr__(self):
        return f"PSISLOO(rows={self.elpd_loo.numel()}, n={self.n}, tail_len={self.tail_len})"


class PosteriorPredictive:
    """Replicated data of the plated site(s) under a population of n equally weighted particles
    (include/gjx_predictive.h): y_rep[d, i] ~ p(y | x_i, data_d), one draw per particle and data row.  Every field is a dict
    by the plated sites' addresses, except `index`.

    `mean`, `var`: the sample mean and (n - 1) variance of y_rep over the particles (zeros at n = 1); `pit` =
    (below + 0.5 equal) / n with `below`, `equal` the particles whose draw is below / equal to the observed value — the
    randomisation-free mid-PIT, uniform on a calibrated continuous model; `nan_count`: the draws that are NaN (a latent outside
    its site's parameter range) — they reach `mean` and `var` as NaN and count neither as below nor as equal.  float64 [D] on
    the device.  `pit`, `below`, `equal` are None where there is nothing observed (`TemperedSMC.predictive(args=)`).

    `draws`: float32 [m, D] per address — the draws of the particles `index` (int64 [m]: 0, k, 2 k, ...) — or None when none
    were asked for."""

    FIELDS = ("s1", "s2", "below", "equal", "nan")

    def __init__(self, addrs, table: torch.Tensor, n: int, draws: torch.Tensor | None = None, draw_stride: int = 0,
                 observed: bool = True):
        """`table`: float64 [S, 5, D] — per plated site the rows s1, s2, below, equal, nan of gjx_temper_predictive; `n`: the
        population size; `draws`: float32 [S, m, D] with m = ceil(n / draw_stride), or None."""
        addrs = list(addrs)
        if table.dim() != 3 or table.shape[0] != len(addrs) or table.shape[1] != 5 or table.dtype != torch.float64:
            raise ValueError(f"PosteriorPredictive: a float64 [{len(addrs)}, 5, D] tensor expected")
        self.n, self.addresses = int(n), addrs
        if self.n < 1:
            raise ValueError("PosteriorPredictive: n >= 1")
        k = int(draw_stride)
        if (draws is None) != (k == 0):
            raise ValueError("PosteriorPredictive: draws come with a draw_stride >= 1, and only with one")
        self.mean, self.var, self.nan_count = {}, {}, {}
        self.pit, self.below, self.equal = ({}, {}, {}) if observed else (None, None, None)
        for s, a in enumerate(addrs):
            s1, s2, below, equal, nan = table[s].unbind(0)
            self.mean[a] = s1 / self.n
            self.var[a] = (s2 - s1 * s1 / self.n) / (self.n - 1) if self.n > 1 else torch.zeros_like(s1)
            self.nan_count[a] = nan
            if observed:
                self.below[a], self.equal[a] = below, equal
                self.pit[a] = (below + 0.5 * equal) / self.n
        self.draws, self.index = None, None
        if draws is not None:
            m = -(-self.n // k)
            if draws.dim() != 3 or tuple(draws.shape) != (len(addrs), m, table.shape[2]) or draws.dtype != torch.float32:
                raise ValueError(f"PosteriorPredictive: draws must be float32 [{len(addrs)}, {m}, {table.shape[2]}]")
            self.draws = {a: draws[s] for s, a in enumerate(addrs)}
            self.index = torch.arange(0, self.n, k, dtype=torch.int64, device=draws.device)

    def __repr__(self):
        D = next(iter(self.mean.values())).numel()
        return f"PosteriorPredictive(sites={self.addresses!r}, rows={D}, n={self.n}, draws={0 if self.index is None else self.index.numel()})"


class TemperedSMC(SMCAlgorithm):
    """Adaptive tempered SMC sampler for a static target (Neal 2001; Del Moral, Doucet & Jasra 2006; the adaptive schedule
    of Jasra et al. 2011).

    `n_moves`: Metropolis-Hastings sweeps per stage; `ess_target`: the next temperature is the largest whose increment keeps
    the effective sample size at `ess_target * n_particles`; `betas`: a FIXED increasing schedule ending at 1 instead;
    `scale`: one proposal scale per latent (a number for all) instead of 2.38 / sqrt(L) times the weighted population
    standard deviation; `proposal`: "diagonal" (that random walk, one latent at a time) or "covariance" — x' = x + F eps with
    F = 2.38 / sqrt(L) times the Cholesky factor of the weighted population covariance, built on the device by one launch
    (include/gjx_temper_cov.h): the proposal for a posterior whose latents are correlated.

    The adaptive schedule depends on the particles, so the estimate of Z is consistent but NOT exactly unbiased (Beskos,
    Jasra, Kantas & Thiery 2016); a fixed `betas=` keeps it unbiased.

    Host reads per adaptive stage: the two ladders' results and the proposal scales — three (two at the last stage, where
    the first ladder already reaches beta = 1; one fewer each with `scale=`; none with `betas=` and `scale=`) — and one at
    the end of the run for the accumulated normalising constants and accept counts.  Under `proposal="covariance"` the factor
    never leaves the device: two per adaptive stage, none before the end of the run with `betas=`."""

    def __init__(self, target: Target, n_particles: int, n_moves: int = 2, ess_target: float = 0.5, betas=None, scale=None,
                 proposal: str = "diagonal"):
        if not isinstance(target, Target):
            raise TypeError("TemperedSMC: target must be a Target")
        self.target, self.n_particles, self.n_moves = target, int(n_particles), int(n_moves)
        self.ess_target = float(ess_target)
        if self.n_particles < 1 or not 0 <= self.n_moves <= abi.TEMPER_MAX_MOVES:
            raise ValueError("TemperedSMC: n_particles >= 1 and 0 <= n_moves <= 256")
        if not 0.0 < self.ess_target < 1.0:
            raise ValueError("TemperedSMC: 0 < ess_target < 1")
        self.betas = None
        if betas is not None:
            b = [float(np.float32(x)) for x in betas]
            if b and b[0] == 0.0:
                b = b[1:]
            if not b or b[-1] != 1.0 or any(y <= x for x, y in zip([0.0] + b, b)):
                raise ValueError("TemperedSMC: betas must increase strictly from above 0 to exactly 1")
            self.betas = b
        self.scale = scale
        if proposal not in ("diagonal", "covariance"):
            raise ValueError(f'TemperedSMC: proposal must be "diagonal" or "covariance", got {proposal!r}')
        if proposal == "covariance" and scale is not None:
            raise ValueError('TemperedSMC: scale= sets the diagonal proposal; it cannot be combined with proposal="covariance"')
        self.proposal = proposal
        self._st = None

    def get_num_particles(self):
        return self.n_particles

    def get_final_target(self):
        return self.target

    # -- lowering ----------------------------------------------------------------------------------------------------------
    def _state(self):
        ops = get_ops()
        st = self._st
        if st is not None and st["ops"] is ops:
            return st
        ops.lib.require("temper", "gjx_temper_plan_create")
        if self.proposal == "covariance":
            ops.lib.require("temper_cov", "gjx_temper_move_cov")
        tracer = lower(self.target, self.n_particles)
        latents = [m for m in tracer.meta if m["obs"] is None and not m.get("grouped")]
        if tracer.n_grouped:
            ops.lib.require("group", "gjx_temper_move_grouped")
            if self.proposal == "covariance":
                self._refuse_grouped(tracer, 'proposal="covariance"')
        tplan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
        prior = prior_table(tracer) if tracer.data or any(s.dist in abi.COUNT_DISTS for s in tracer.sites) else None
        st = self._st = dict(ops=ops, tracer=tracer, latents=latents, tplan=tplan, ws=None, prior=prior, ws_cov=None)
        return st

    @staticmethod
    def _refuse_grouped(tracer, what: str):
        m = next(m for m in tracer.meta if m.get("grouped"))
        raise PlanUnsupported(f"TemperedSMC: {what} is not supported with the grouped latent at address {m['addr']!r} "
                              "(include/gjx_group.h: the grouped move is the diagonal random walk of run())")

    # -- a population of a plan with grouped latents (include/gjx_group_checks.h) -----------------------------------------------
    def _split_population(self, what: str, res):
        """`res` -> (the L scalar columns, the S grouped columns [G, n] or None) as given, unchecked but for their count.  A plan
        with grouped latents takes a TemperedResult of a grouped run (`columns` and `group_columns`) or the latent columns in
        table order as `choices` holds them: scalars [n], grouped [G, n].  The L scalar columns alone are refused, naming the
        first grouped address: its [G, n] column is missing.  Raised before anything is asked of the library."""
        st = self._state()
        tracer = st["tracer"]
        if not tracer.n_grouped:
            return (list(res.columns) if isinstance(res, TemperedResult) else list(res)), None
        lat = [m for m in tracer.meta if m["obs"] is None]  # table order, scalar and grouped
        first = next(m["addr"] for m in lat if m.get("grouped"))
        if isinstance(res, TemperedResult):
            if res.group_columns is None:
                raise PlanUnsupported(f"TemperedSMC: {what} needs the [G, n] column of the grouped latent at address {first!r}: the "
                                      "TemperedResult is not one of a run with grouped latents")
            return list(res.columns), list(res.group_columns)
        given = list(res)
        if len(given) == len(st["latents"]):
            raise PlanUnsupported(f"TemperedSMC: {what} got the {len(given)} scalar latent columns alone; the [G, n] column of the grouped "
                                  f"latent at address {first!r} is missing (pass the TemperedResult, or the latent columns in table order as "
                                  "`choices` holds them: scalars [n], grouped [G, n])")
        if len(given) != len(lat):
            raise ValueError(f"TemperedSMC.{what}: {len(lat)} latent columns expected ({[m['addr'] for m in lat]!r}), got {len(given)}")
        return [c for m, c in zip(lat, given) if not m.get("grouped")], [c for m, c in zip(lat, given) if m.get("grouped")]

    def _lower_held_out(self, what: str, target: Target):
        """The lowering of a held-out target of a grouped plan: its own group tensor must be sorted with values in 0 .. G-1 and
        the fitted G (ValueError otherwise: a group that was never fitted has no column)."""
        fitted = self._state()["tracer"]
        try:
            tracer = lower(target, self.n_particles)
        except GroupTensorRefused as e:
            raise ValueError(f"TemperedSMC.{what}: {e} — the rows' groups must be sorted and among the {fitted.n_groups} fitted "
                             "groups (a group that was never fitted has no column)") from None
        if tracer.n_groups != fitted.n_groups:
            at = next(m["addr"] for m in fitted.meta if m.get("grouped"))
            raise ValueError(f"TemperedSMC.{what}: the target has G = {tracer.n_groups} groups, the grouped latent at address {at!r} was "
                             f"fitted with G = {fitted.n_groups}")
        return tracer

    GROUP_SCALE_BYTES = 256 << 20  # the float64 working block of group_scales

    @staticmethod
    def group_scales(z: list, lw: torch.Tensor) -> torch.Tensor:
        """2.38 / sqrt(S) times the weighted standard deviation of every component z[s][g][:] of the S grouped columns
        (float32 [G, n] each): float64 on the device, rounded to float32 -> f32 [S, G], still on the device."""
        w = torch.softmax(lw.double(), dim=0)
        # a block of groups at a time: the float64 temporaries stay at GROUP_SCALE_BYTES whatever G is (a [G, n] float64
        # copy of one site is 8 GB at G = 1000, n = 1e6); the weighted sums are matrix-vector products
        rows = max(1, TemperedSMC.GROUP_SCALE_BYTES // (8 * max(1, lw.numel())))
        out = torch.empty(len(z), z[0].shape[0], dtype=torch.float64, device=lw.device)
        for s, col in enumerate(z):
            for g0 in range(0, col.shape[0], rows):
                c = col[g0:g0 + rows].double()
                c -= (c @ w)[:, None]
                out[s, g0:g0 + rows] = c.square_() @ w
        return (2.38 / math.sqrt(len(z)) * torch.sqrt(out)).to(torch.float32).contiguous()

    def _scales(self, st):
        L = len(st["latents"])
        if self.scale is None:
            return None
        s = np.asarray(self.scale, dtype=np.float32).reshape(-1)
        if s.size == 1:
            s = np.repeat(s, L)
        if s.size != L:
            raise ValueError(f"TemperedSMC: scale must be one number or one per latent ({L})")
        return s

    @staticmethod
    def population_scales(x: list, lw: torch.Tensor) -> torch.Tensor:
        """2.38 / sqrt(L) times the weighted standard deviation of every latent column, float64 on the device, rounded to
        float32 (f32[L], still on the device)."""
        w = torch.softmax(lw.double(), dim=0)
        cols = torch.stack([c.double() for c in x])
        mean = (cols * w).sum(dim=1, keepdim=True)
        var = (((cols - mean) ** 2) * w).sum(dim=1)
        return (2.38 / math.sqrt(len(x)) * torch.sqrt(var)).to(torch.float32)

    # -- the run ---------------------------------------------------------------------------------------------------------------
    def run(self, key) -> TemperedResult:
        """Stage 0 draws the population from the prior (the importance kernel) and fills lp / ll (one move launch with K = 0,
        recompute); stage s >= 1 picks beta', reweights, resamples systematically under fold_in(fold_in(key, s), 0) and
        moves under fold_in(fold_in(key, s), 1) — the last stage (beta' = 1) too, so the population returned is equally
        weighted.  A function of `key` alone: two runs are bit-equal."""
        st = self._state()
        ops, tracer, tplan = st["ops"], st["tracer"], st["tplan"]
        n, L, K = self.n_particles, len(st["latents"]), self.n_moves
        # (sets the importance plan's launch parameters; a plated plan draws from the table WITHOUT its plated sites: they
        # draw nothing, and the importance kernels do not know the mode)
        plan = _make_plan(st["prior"] if st["prior"] is not None else tracer)
        if tracer.params:
            tplan.set_params(tracer.params)
        if tracer.data:  # uploaded at every run: an in-place update of a data tensor is seen
            tplan.set_data(tracer.data_columns(ops.device()))
        dtypes = [torch.float32] * tracer.n_out
        vals = ops.importance_run(plan, prng.split_lazy(prng.fold_in(key, 0), n), n, [], dtypes, want_score=False,
                                  want_max_partials=False)[0]
        x = [vals[m["out_col"]] for m in st["latents"]]
        grouped, z, accepts_z = tracer.n_grouped > 0, None, []
        if grouped:  # the offsets from the group tensor as it is now; the grouped columns from their priors at the scalars drawn
            tplan.set_groups(tracer.group_offsets().to(ops.device()))
            x, z, lp, ll, _, _ = ops.temper_move_grouped(tplan, key, x, None, None, None, 0.0, 0, recompute=True,
                                                         init_key=prng.fold_in(key, 0x7ffffffe), want_accept=False)
        else:
            x, lp, ll, _ = ops.temper_move(tplan, key, x, None, None, 0.0, 0, None, recompute=True, want_accept=False)
        if st["ws"] is None:
            st["ws"] = ops.temper_ladder_workspace(n)
        ws = st["ws"]
        fixed_scales = self._scales(st)
        need = self.ess_target * n
        cov = self.proposal == "covariance"
        if cov and st["ws_cov"] is None:
            st["ws_cov"] = ops.temper_moments_workspace(n, L)
        factor, degenerate = None, []

        def ess_fn(deltas):
            out = ops.temper_ess_ladder(ll, deltas, ws).cpu().numpy()  # (one host read)
            return ess_of(out[0:-1:2], out[1:-1:2])

        beta, betas, ess, pairs, accepts = 0.0, [0.0], [], [], []
        s = 0
        while beta < 1.0:
            s += 1
            ks = prng.fold_in(key, s)
            if self.betas is not None:
                nb = self.betas[s - 1]
                out = ops.temper_ess_ladder(ll, [np.float32(nb) - np.float32(beta)], ws)
                ess.append(out)  # (read at the end of the run)
            else:
                nb, e = next_beta(beta, need, ess_fn)
                ess.append(e)
            delta = float(np.float32(np.float32(nb) - np.float32(beta)))
            lw = ll * delta  # f32: one rounding per particle
            anc, e_s, q_s = ops.resample("systematic", prng.fold_in(ks, 0).literal(), lw)
            if cov:  # the moments of the weighted population BEFORE resampling; the factor stays on the device
                _, factor, _, nd = ops.temper_moments(x, lw, st["ws_cov"])
                degenerate.append(nd)  # (read at the end of the run)
                x, lp, ll, acc = ops.temper_move_cov(tplan, prng.fold_in(ks, 1), x, lp, ll, nb, K, factor, ancestors=anc)
            else:
                sc = fixed_scales
                if sc is None and K > 0:
                    sc = self.population_scales(x, lw).cpu().numpy()  # (one host read)
                if grouped:  # (the grouped scales never leave the device)
                    zsc = self.group_scales(z, lw) if K > 0 else None
                    x, z, lp, ll, acc, accz = ops.temper_move_grouped(tplan, prng.fold_in(ks, 1), x, z, lp, ll, nb, K, sc, zsc, ancestors=anc)
                    accepts_z.append(accz.sum())
                else:
                    x, lp, ll, acc = ops.temper_move(tplan, prng.fold_in(ks, 1), x, lp, ll, nb, K, sc, ancestors=anc)
            pairs.append((e_s, q_s))
            accepts.append(acc.sum())
            beta = nb
            betas.append(nb)
        # one host read for the whole run: the exact (e, q) pair of every stage, the accept counts, fixed-schedule ESS sums
        e_all = torch.cat([p[0] for p in pairs]).cpu().numpy().astype(np.int64)
        q_all = torch.cat([p[1] for p in pairs]).cpu().numpy().astype(np.int64)
        if cov:  # (the stages' degenerate counts ride along with the accept counts)
            tail = torch.cat([torch.stack(accepts).to(torch.int64), torch.cat(degenerate).to(torch.int64)]).cpu().numpy()
            acc_all, degenerate = tail[:len(accepts)], [int(v) for v in tail[len(accepts):]]
        else:  # (a grouped plan's group accept counts ride along)
            acc_all = torch.stack(accepts + accepts_z).to(torch.int64).cpu().numpy()
            acc_all, accz_all = acc_all[:len(accepts)], acc_all[len(accepts):]
        log_z = 0.0
        for e_s, q_s in zip(e_all, q_all):
            if q_s <= 0:
                log_z = float("-inf")
                break
            log_z += int(e_s) * math.log(2.0) + math.log(int(q_s)) - 30 * math.log(2.0) - math.log(n)
        if self.betas is not None:
            ess = [float(ess_of(o[0], o[1])) for o in torch.stack(ess).cpu().numpy()]
        rate = [float(a) / (n * K) if K else 0.0 for a in acc_all]
        if grouped:  # in table order: the scalar columns f32 [n], the grouped ones f32 [G, n]
            xs, zs = iter(x), iter(z)
            pairs_ = [(m["addr"], next(zs) if m.get("grouped") else next(xs)) for m in tracer.meta if m["obs"] is None]
            res = TemperedResult(float(log_z), betas, ess, rate, ChoiceMap.from_mapping(pairs_), lp, ll, x)
            G = tracer.n_groups
            res.accept_rate_groups = [float(a) / (n * K * G) if K else 0.0 for a in accz_all]
            res.group_columns = z
            return res
        choices = ChoiceMap.from_mapping([(m["addr"], c) for m, c in zip(st["latents"], x)])
        if not cov:
            return TemperedResult(float(log_z), betas, ess, rate, choices, lp, ll, x)
        full = torch.zeros(L, L, dtype=torch.float32, device=factor.device)
        rows, cols = torch.tril_indices(L, L, device=factor.device)  # (row-major: the packing of the header)
        full[rows, cols] = factor
        return TemperedResult(float(log_z), betas, ess, rate, choices, lp, ll, x, full, degenerate)

    # -- the SMCAlgorithm interface --------------------------------------------------------------------------------------------
    def run_smc(self, key) -> ParticleCollection:
        """The final population as a ParticleCollection: traces through `Target.importance` with the latent columns as
        constraints, every log-weight f32(log Z-hat), so that logsumexp - log n reproduces the estimate."""
        if self._state()["tracer"].n_grouped:
            self._refuse_grouped(self._state()["tracer"], "run_smc")
        if self._state()["tracer"].data:
            m = next(m for m in self._state()["tracer"].meta if m.get("plated"))
            raise PlanUnsupported(f"TemperedSMC.run_smc: the plated site at address {m['addr']!r} has no per-site trace; use run() "
                                  "or log_marginal_likelihood_estimate()")
        res = self.run(key)
        n = self.n_particles
        sub_keys = split(prng.fold_in(key, 0x7fffffff), n)
        trs, _ = self.target.importance(sub_keys, res.choices)  # (every site is constrained: the keys draw nothing)
        lw = torch.full((n,), float(np.float32(res.log_marginal_likelihood)), dtype=torch.float32, device=res.lp.device)
        out = ParticleCollection(trs, lw, True)
        out.result = res
        return out

    # -- a population against a plated table: what pointwise() and predictive() share ---------------------------------------------
    def _population(self, what: str, noun: str, split, target: Target | None):
        """`split` (_split_population of the caller's population) and `target` (None: the fitted one) -> (tracer, the tempered plan
        with its parameters, data and groups set, the scalar columns as float32 device tensors, the grouped columns [G, n]
        likewise or None).  A `target` of its own gets a plan of its own (same structure: its kernels come out of the JIT
        cache)."""
        st = self._state()
        ops = st["ops"]
        grouped = st["tracer"].n_grouped > 0
        cols, zcols = split
        fitted = [m["addr"] for m in st["latents"]]
        if grouped and len(cols) == len(fitted):  # (before anything is uploaded)
            n, G = int(cols[0].numel()), st["tracer"].n_groups
            for m, c in zip([m for m in st["tracer"].meta if m.get("grouped")], zcols):
                if not isinstance(c, torch.Tensor) or c.dim() != 2 or tuple(c.shape) != (G, n):
                    shape = tuple(c.shape) if isinstance(c, torch.Tensor) else type(c).__name__
                    raise ValueError(f"TemperedSMC.{what}: the column of the grouped latent at address {m['addr']!r} must be [G, n] = "
                                     f"[{G}, {n}] (the fitted G, the population's n), got {shape}")
        if target is None:
            tracer, tplan = st["tracer"], st["tplan"]
        else:
            if not isinstance(target, Target):
                raise TypeError(f"TemperedSMC.{what}: target must be a Target")
            tracer = self._lower_held_out(what, target) if grouped else lower(target, self.n_particles)
            theirs = [m["addr"] for m in tracer.meta if m["obs"] is None]
            ours = [m["addr"] for m in st["tracer"].meta if m["obs"] is None]
            if theirs != ours:
                raise ValueError(f"TemperedSMC.{what}: the target's latent addresses {theirs!r} are not the fitted plan's {ours!r}")
            tplan = None
        if not tracer.data:
            raise PlanUnsupported(f"TemperedSMC.{what}: no plated site among the addresses {[m['addr'] for m in tracer.meta]!r} "
                                  f"({noun} are those of a site observed over a data column)")
        if len(cols) != len(fitted):
            raise ValueError(f"TemperedSMC.{what}: {len(fitted)} latent columns expected ({fitted!r}), got {len(cols)}")
        if tplan is None:
            tplan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
        if tracer.params:
            tplan.set_params(tracer.params)
        tplan.set_data(tracer.data_columns(ops.device()))
        dev = lambda c: c.detach().to(device=ops.device(), dtype=torch.float32).contiguous()
        if not grouped:
            return tracer, tplan, [dev(c) for c in cols], None
        tplan.set_groups(tracer.group_offsets().to(ops.device()))  # (the group tensor as it is now, next to the data)
        return tracer, tplan, [dev(c) for c in cols], [dev(c) for c in zcols]

    # -- pointwise predictive densities (include/gjx_pointwise.h) ------------------------------------------------
    def pointwise(self, res, target: Target | None = None) -> PointwiseLikelihood:
        """The per-row log-likelihood of the plated site(s) under the population `res` — a TemperedResult of `run`, or the L
        latent columns (float32 [n]) in the plan's latent order — reduced over the particles in two launches.
        `target=None` scores the rows the sampler was fitted to; a `Target` over the same model body with OTHER data
        tensors scores held-out rows under the same population (same structure: the kernel comes out of the JIT cache).
        A plan with grouped latents (include/gjx_group_checks.h) takes the TemperedResult of its run, or the latent columns
        in table order as `choices` holds them (scalars [n], grouped [G, n]); row d is scored at the values of ITS group, and
        a held-out target brings its own group tensor: sorted, with values in 0 .. G-1, the fitted G."""
        ops = self._state()["ops"]
        split = self._split_population("pointwise", res)  # (a grouped plan's refusal of scalar columns alone comes first)
        ops.lib.require("pointwise", "gjx_temper_pointwise")
        _, tplan, x, z = self._population("pointwise", "pointwise densities", split, target)
        return PointwiseLikelihood(ops.temper_pointwise(tplan, x, z=z), x[0].numel())

    # -- PSIS-LOO (include/gjx_psis.h) ------------------------------------------------------------------------------
    def loo(self, res, r_eff: float = 1.0) -> PSISLOO:
        """Pareto-smoothed importance-sampling leave-one-out over the rows the sampler was fitted to, under the population
        `res` — a TemperedResult of `run`, or the L latent columns (float32 [n]) in the plan's latent order: per row elpd_loo
        and the diagnostic k-hat (PSISLOO), and the pointwise densities of the same call.  `r_eff`: the relative efficiency of
        the population; as in the `loo` package it enters the tail length min(0.2 n, 3 sqrt(n / r_eff)) alone (capped at 4095:
        include/gjx_psis.h).  A plan with grouped latents: as `pointwise` (rows are left out one at a time, not groups)."""
        ops = self._state()["ops"]
        split = self._split_population("loo", res)
        ops.lib.require("psis", "gjx_temper_psis")
        ops.lib.require("pointwise", "gjx_temper_pointwise")
        _, tplan, x, z = self._population("loo", "leave-one-out densities", split, None)
        n = int(x[0].numel())
        M = int(ops.lib.call("gjx_psis_tail_len", n, float(r_eff)))
        if M == 0:
            raise ValueError(f"TemperedSMC.loo: a population of n = {n} at r_eff = {r_eff} has no tail to fit (n >= 25 and a positive finite r_eff)")
        table, _ = ops.temper_psis(tplan, x, M, z=z)
        return PSISLOO(table, PointwiseLikelihood(ops.temper_pointwise(tplan, x, z=z), n), n, M)

    # -- posterior predictive draws (include/gjx_predictive.h) ---------------------------------------------------
    def _unobserved_target(self, st, args) -> Target:
        """The fitted model at the arguments `args` with nothing observed at its plated sites: every plated address is
        constrained to zeros of the data length (a tensor of its own each: the columns of the table stay those of the fitted
        plan), every other observed address keeps the fitted constraint."""
        if not isinstance(args, tuple):
            raise TypeError("TemperedSMC.predictive: args must be a tuple")
        rows = {int(a.numel()) for a in args if is_data_tensor(a)}
        if len(rows) != 1:
            raise PlanUnsupported(f"TemperedSMC.predictive: args must hold data columns (1-D tensors) of one length, got lengths {sorted(rows)}")
        D = rows.pop()
        meta = st["tracer"].meta

        def fill(one=None):
            pairs = [(m["addr"], torch.full((D,), 1.0 if m["addr"] == one else 0.0, dtype=torch.float32) if m.get("plated") else m["obs"])
                     for m in meta if m["obs"] is not None]
            return Target(self.target.p, args, ChoiceMap.from_mapping(pairs))

        # A plated site's value that feeds a later site is data (gjx_plate.h) — and here there is none: the fill would be read
        # as if it had been observed.  Found by lowering with another fill at one address at a time: a later site that reads
        # that address's column, or a column computed from it (one that changes with the fill), is refused.
        target = fill()
        plated = [m["addr"] for m in meta if m.get("plated")]
        if len(plated) > 1:
            base = lower(target, self.n_particles)
            for addr in plated:
                reader = _reads_value_of(base, lower(fill(addr), self.n_particles), addr)
                if reader is not None:
                    raise PlanUnsupported(f"TemperedSMC.predictive: args= observes nothing, but the site at address {reader!r} reads the "
                                          f"value of the plated site at address {addr!r} (a plated site's value that feeds a later site "
                                          "is data); pass target= with observed values instead")
        return target

    def predictive(self, res, key, target: Target | None = None, args=None, n_draws: int | None = None,
                   draw_stride: int | None = None) -> PosteriorPredictive:
        """Replicated data of the plated site(s) under the population `res` — a TemperedResult of `run`, or the L latent
        columns (float32 [n]) in the plan's latent order: one draw per particle and data row in two launches, summarised per
        row (PosteriorPredictive).  A function of the columns, the data and `key`: particle i draws under fold_in(key, i).

        `target=None` replicates the rows the sampler was fitted to; a `Target` over the same model body with OTHER data
        tensors replicates held-out rows and places their observed values among the draws; `args=` (the model's arguments,
        new inputs) predicts where nothing is observed — no `pit`.  Same structure: the kernel comes out of the JIT cache.
        `draw_stride=k` also returns the draws of particles 0, k, 2 k, ...; `n_draws=m` is draw_stride = ceil(n / m): at most m
        of them, spread over the population (after resampling, neighbours are copies of one ancestor).
        A plan with grouped latents: `res` as `pointwise` takes it; `target=` and `args=` carry the new rows' group tensor,
        whose groups must be among the fitted ones (a group that was never fitted has no column to draw from)."""
        st = self._state()
        split = self._split_population("predictive", res)
        st["ops"].lib.require("predictive", "gjx_temper_predictive")
        if target is not None and args is not None:
            raise ValueError("TemperedSMC.predictive: target= (held-out rows) or args= (new inputs, nothing observed), not both")
        if n_draws is not None and draw_stride is not None:
            raise ValueError("TemperedSMC.predictive: n_draws= or draw_stride=, not both")
        if n_draws is not None and int(n_draws) < 1:
            raise ValueError("TemperedSMC.predictive: n_draws >= 1")
        if draw_stride is not None and int(draw_stride) < 1:
            raise ValueError("TemperedSMC.predictive: draw_stride >= 1")
        if args is not None:
            target = self._unobserved_target(st, args)
        tracer, tplan, x, z = self._population("predictive", "replicated data", split, target)
        n = int(x[0].numel())
        k = -(-n // int(n_draws)) if n_draws is not None else int(draw_stride or 0)
        table, draws = st["ops"].temper_predictive(tplan, key, x, k, z=z)
        addrs = [m["addr"] for m in tracer.meta if m.get("plated")]
        return PosteriorPredictive(addrs, table, n, draws, k, observed=args is None)

    def log_marginal_likelihood_estimate(self, key, target: Target | None = None):
        if target is not None:
            return super().log_marginal_likelihood_estimate(key, target)
        res = self.run(key)
        return torch.tensor(float(np.float32(res.log_marginal_likelihood)), dtype=torch.float32, device=res.lp.device)
