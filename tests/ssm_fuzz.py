"""Random and mixed state-space bodies against a float64 replay of their own source text.

Every suite that pins the state-space kernels (the fused bootstrap step, the guided step, the parameter bank, the conditional
step, backward simulation) builds its reference from the TRACER's site tables: a lowering mistake (a state reference to the
wrong carry component, two observation columns swapped, an operand on the wrong side of a subtraction in a carry program, a
site reference not renumbered) is in the kernel and in the replay alike.  This module is the reference that shares nothing with
the lowering.  `replay64` executes the source text of `init` and `step` step by step over a RECORDED run — `history`,
`ancestors`, `log_weight_history`, `resampled` of an `SMCResult` — with small distribution objects of its own over torch
float64 tensors: at step t the old carry is history[t-1][ancestors[t]], a latent site returns history[t][its component], an
observed site returns obs[t].  That determines the step's log-weight, every carry component that is not a latent draw, and the
law of every latent draw given its parents.  `check_run` compares with a tolerance DERIVED as in temper_fuzz.Reference (the
pinned bounds of every log-density plus FLOOR_FACTOR times the case's own f32 floor, measured on the replay alone), and holds
the laws to bounds that are derived, not measured (DKW at alpha = 1e-6; 5 standard errors of a standardised residual).
Only the last section imports the package.  Used by tests/test_ssm_fuzz_cpu.py (oracle) and tests/test_gpu_ssm_fuzz.py (HIP)."""

import math
import operator
import re

import numpy as np
import torch

from dist_range_ref import beta_tolerance, gamma_tolerance
from fuzz_models import _expr, _pos
from temper_fuzz import COND_REL, FLOOR_FACTOR, MIN_FINITE, bernoulli_tolerance, misses, normal_tolerance

SMC_MAX_STATE = 4            # include/gjx.h: GJX_SMC_MAX_STATE (restated: this section imports nothing of the package)
THETA = ("a", "q", "r")      # a parameterised body's theta: `a` in (-0.9, 0.9), `q` and `r` in (0.5, 1.5)
# host arithmetic on theta (derived slots of the ParamSpace): real-valued, positive, and at least 1 (latent Gamma / Beta shapes)
T_REAL = ("a", "(a * 0.5 + q)", "(q - r)", "(-a)")
T_POS = ("q", "r", "(q * 1.5)", "(a * a + r)")
T_SHAPE = ("(q + 1.0)", "(q + r)")
# The constants that keep a run off the edges with the reference alone: every argument that reads a traced value is either
# affine with a slope of at most 0.9 or clamped — locations to +-LOC, Normal scales to SCALE, the shapes and rates of LATENT
# Gamma / Beta sites to SHAPE / RATE (shapes of 1 and more: no mass piles up at 0 or 1, so no f32 draw lands on the edge of the
# support), those of observed ones to OBS_SHAPE — and an expression component of the carry is clamped to +-EXPR or contracts.
# The carry is then bounded in law at every step, whatever T is.
LOC, SCALE, SHAPE, RATE, OBS_SHAPE, EXPR = 2.5, (0.3, 2.0), (1.0, 4.0), (0.5, 3.0), (0.5, 4.0), 3.0
ALPHA_LOG = math.log(2e6)    # DKW: P(D > eps) <= 2 exp(-2 N eps^2) = 1e-6
Z_BOUND = 5.0

_NAME = re.compile(r"\b[cxy]\d\b")


def _has(e):
    return bool(_NAME.search(e))


def _lit(rng, lo, hi):
    return repr(round(float(rng.uniform(lo, hi)), 3))


def random_theta(rng):
    return np.asarray([rng.uniform(-0.9, 0.9), rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5)], dtype=np.float32)


# ---- the generator ---------------------------------------------------------------------------------------------------------
def _loc(rng, reals, th):
    if reals and rng.random() < 0.35:  # affine in one traced value: a plain argument reference (GJX_ARG_STATE / _SITE / _OBS)
        k = str(rng.choice(T_REAL)) if th and rng.random() < 0.4 else _lit(rng, -0.9, 0.9)
        return f"({k} * {rng.choice(reals)} + {_lit(rng, -1.0, 1.0)})"
    e = _expr(rng, reals, list(T_REAL) if th else [])
    return f"torch.clamp({e}, min={-LOC}, max={LOC})" if _has(e) else e


def _positive(rng, reals, poss, th, bounds, affine=False):
    lo, hi = bounds
    if th and rng.random() < 0.25:
        return str(rng.choice(T_SHAPE if lo >= 1.0 else T_POS))
    e = _pos(rng, reals, poss, [])
    if not _has(e):
        return _lit(rng, lo, min(hi, 3.0))
    if affine and re.fullmatch(r"\(\w+ \* [\d.]+ \+ [\d.]+\)", e):
        return e  # a positive affine function of a Gamma value, whose own law is bounded
    return f"torch.clamp({e}, min={lo}, max={hi})"


def _sites(rng, order, reals, poss, th, indent="    "):
    """The lines of the sites `order` [(name, kind, role)]; `reals` / `poss`: what they may read to begin with."""
    reals, poss, lines, reads_old = list(reals), list(poss), [], {}
    for name, kind, role in order:
        lat = role == "latent"
        if kind == "normal":
            call = f"normal({_loc(rng, reals, th)}, {_positive(rng, reals, poss, th, SCALE, affine=True)})"
        elif kind == "gamma":
            call = f"gamma({_positive(rng, reals, poss, th, SHAPE if lat else OBS_SHAPE)}, {_positive(rng, reals, poss, th, RATE)})"
        elif kind == "beta":
            b = SHAPE if lat else OBS_SHAPE
            call = f"beta({_positive(rng, reals, poss, th, b)}, {_positive(rng, reals, poss, th, b)})"
        else:
            e = _loc(rng, reals, th)
            # (torch.sigmoid of a number is no tensor operation: a logit without a traced value is a literal p)
            call = f"flip(torch.sigmoid({e}))" if _has(e) else f"flip({_lit(rng, 0.1, 0.9)})"
        lines.append(f"{indent}{name} = {call} @ '{name}'")
        reads_old[name] = bool(re.search(r"\bc\d\b", call))
        if kind != "flip":
            reals.append(name)
            if kind == "gamma":
                poss.append(name)
    return lines, reads_old


def random_ssm(rng, flat=False, params=False, cheap=False):
    """-> (source of `init`, source of `step`, description).  The carry has 1 .. SMC_MAX_STATE components; every latent site
    (normal, gamma, beta) is returned in the carry by itself; where room is left (not `flat`) further components are an
    expression over latents, the old carry and observed values, a pass-through of an old component, an observed value or a
    literal.  1 to 3 observed addresses (normal, gamma, beta, flip(sigmoid(.))); later sites may read an earlier observed
    site's value; the site order is random.  `params`: the bodies take theta = (a, q, r), which reaches arguments by itself and
    through host arithmetic.  `cheap`: Normal latents and at most one Gamma one (the GPU suite's threefry bodies: a latent Gamma
    site costs a threefry kernel seconds of compilation, a Beta site twice that).  description: lat / obs [(name, kind)],
    comps [(what, detail)], reads_old {site: bool} of step."""
    n_lat = int(rng.integers(1, 5 if flat else 4))
    lat = [(f"x{i}", str(rng.choice(["normal", "normal", "gamma", "beta"]))) for i in range(n_lat)]
    if cheap:
        lat = [(name, "normal") for name, _ in lat]
        if rng.random() < 0.5:
            k = int(rng.integers(n_lat))
            lat[k] = (lat[k][0], "gamma")
    obs = [(f"y{j}", str(rng.choice(["normal", "normal", "gamma", "beta", "flip"]))) for j in range(int(rng.integers(1, 4)))]
    comps = [("latent", name) for name, _ in lat]
    if not flat:
        for _ in range(int(rng.integers(0, SMC_MAX_STATE - n_lat + 1))):
            comps.append((str(rng.choice(["expr", "expr", "pass", "obs", "lit"])), None))
    comps = [comps[k] for k in rng.permutation(len(comps))]
    kind_of = dict(lat)
    old = [f"c{k}" for k in range(len(comps))]
    old_poss = [f"c{k}" for k, (w, d) in enumerate(comps) if w == "latent" and kind_of[d] == "gamma"]
    real_obs = [name for name, kind in obs if kind != "flip"]

    def body(is_step):
        both = [(n_, k_, "latent") for n_, k_ in lat] + [(n_, k_, "observed") for n_, k_ in obs]
        order = [both[k] for k in rng.permutation(len(both))]
        lines, reads_old = _sites(rng, order, old if is_step else [], old_poss if is_step else [], params)
        pool = [n_ for n_, k_ in lat] + real_obs + (old if is_step else [])
        ret = []
        for k, (what, d) in enumerate(comps):
            if what == "latent":
                ret.append(d)
            elif what == "expr":
                if is_step and rng.random() < 0.3:  # a contracting accumulator
                    ret.append(f"({rng.choice(old)} * {_lit(rng, 0.2, 0.9)} - {_lit(rng, 0.1, 0.9)} * {lat[0][0]})")
                else:
                    e = next((e for e in (_expr(rng, pool, list(T_REAL) if params else []) for _ in range(20)) if _has(e)), lat[0][0] + " * 0.5")
                    ret.append(f"torch.clamp({e}, min={-EXPR}, max={EXPR})")
            elif what == "pass":
                ret.append(str(rng.choice(old)) if is_step else _lit(rng, -1.0, 1.0))
            elif what == "obs" and real_obs:
                comps[k] = ("obs", d or str(rng.choice(real_obs)))
                ret.append(comps[k][1])
            else:
                comps[k] = ("lit", d or _lit(rng, -1.5, 1.5))
                ret.append(comps[k][1])
        return lines, ret, reads_old

    th = "    a, q, r = theta\n" if params else ""
    il, ir, _ = body(False)
    sl, sr, reads_old = body(True)
    tup = lambda r: r[0] if len(r) == 1 else "(" + ", ".join(r) + ")"  # noqa: E731
    init_src = f"def init({'theta' if params else ''}):\n{th}" + "\n".join(il) + f"\n    return {tup(ir)}\n"
    unpack = f"    {', '.join(old)} = carry\n" if len(old) > 1 else "    c0 = carry\n"
    step_src = f"def step(carry{', theta' if params else ''}):\n{unpack}{th}" + "\n".join(sl) + f"\n    return {tup(sr)}\n"
    return init_src, step_src, dict(lat=lat, obs=obs, comps=comps, reads_old=reads_old, params=params, flat=flat)


def random_proposal(rng, sites):
    """-> {"step": source of `step_proposal(carry, y[, theta])`, "init": source of `init_proposal(y[, theta])` or None,
    "step_sites" / "init_sites": the proposed addresses}: a random non-empty subset of the body-level latents, each proposed
    from its own family with arguments that read the carry and `y`."""
    lat, obs, params = sites["lat"], sites["obs"], sites["params"]
    ys = [n_ for n_, _ in obs]
    y_reals = [n_ for n_, k_ in obs if k_ != "flip"] + [f"({n_} * 0.7)" for n_, k_ in obs if k_ == "flip"]
    y_poss = [n_ for n_, k_ in obs if k_ == "gamma"]
    old = [f"c{k}" for k in range(len(sites["comps"]))]
    old_poss = [f"c{k}" for k, (w, d) in enumerate(sites["comps"]) if w == "latent" and dict(lat)[d] == "gamma"]
    th = "    a, q, r = theta\n" if params else ""
    yun = f"    {', '.join(ys)} = y\n" if len(ys) > 1 else f"    {ys[0]} = y\n"

    def subset():
        pick = [s for s in lat if rng.random() < 0.6]
        return pick or [lat[int(rng.integers(len(lat)))]]

    out = {}
    pick = subset()
    lines, _ = _sites(rng, [(n_, k_, "latent") for n_, k_ in pick], old + y_reals, old_poss + y_poss, params)
    unpack = f"    {', '.join(old)} = carry\n" if len(old) > 1 else "    c0 = carry\n"
    out["step"] = f"def step_proposal(carry, y{', theta' if params else ''}):\n{unpack}{yun}{th}" + "\n".join(lines) + "\n"
    out["step_sites"] = [n_ for n_, _ in pick]
    out["init"], out["init_sites"] = None, []
    if rng.random() < 0.5:
        pick = subset()
        lines, _ = _sites(rng, [(n_, k_, "latent") for n_, k_ in pick], y_reals, y_poss, params)
        out["init"] = f"def init_proposal(y{', theta' if params else ''}):\n{yun}{th}" + "\n".join(lines) + "\n"
        out["init_sites"] = [n_ for n_, _ in pick]
    return out


def random_observations(rng, obs, T):
    """{address: f32 [T]} (a flip's as 0 / 1)."""
    draw = {"normal": lambda: rng.standard_normal(T), "gamma": lambda: rng.gamma(2.0, 0.5, T) + 0.05,
            "beta": lambda: rng.uniform(0.05, 0.95, T), "flip": lambda: rng.integers(0, 2, T)}
    return {name: draw[kind]().astype(np.float32) for name, kind in obs}


# ---- the fixed body: what the generator does not draw ---------------------------------------------------------------------------
# A callee (`outer`) that calls another callee (`inner`); `inner`'s latent comes back through both into the carry; `outer` holds an
# observed site at the nested address ("h", "o"); an integer-valued (flip) latent `k` is a carry component; `z`, an observation,
# and the constant 1.5 are carry components.
_MIXED_CALLEES = '''@gen
def inner(m):
    w = normal(m * 0.5, 0.8) @ "w"
    return w

@gen
def outer(m, s):
    w = inner(m + 0.1) @ "in"
    normal(w * 0.9, s) @ "o"
    return w

'''
MIXED = (_MIXED_CALLEES + '''def init():
    k = flip(0.4) @ "k"
    w = outer(0.3, 0.7) @ "h"
    z = normal(w, 0.6) @ "z"
    return (w, k, z, 1.5)
''', '''def step(carry):
    w0, k0, z0, c = carry
    k = flip(torch.sigmoid(w0 * 0.8 - 0.2)) @ "k"
    w = outer(w0 * 0.7 + k0 * 0.5 - z0 * 0.1, 0.5 + 0.1 * c) @ "h"
    z = normal(w + k * 0.3, 0.6) @ "z"
    return (w, k, z, 1.5)
''')
MIXED_OBS = (("h", "o"), ("z",))


# ---- one execution of a body ---------------------------------------------------------------------------------------------------
class Th:
    """A theta entry or a value the body derives from theta on the host: Python float arithmetic, as written.  `log` receives
    the value whenever it leaves the host (meets a traced value or reaches a site argument)."""

    def __init__(self, v, log):
        self.v, self.log = float(v), log

    def use(self):
        self.log.append(self.v)
        return self.v

    def _bin(self, o, op, swap=False):
        if isinstance(o, Th):
            return Th(op(o.v, self.v) if swap else op(self.v, o.v), self.log)
        if isinstance(o, (int, float)):
            return Th(op(o, self.v) if swap else op(self.v, o), self.log)
        return op(o, self.use()) if swap else op(self.use(), o)

    def __neg__(self):
        return Th(-self.v, self.log)


for _n, _op in (("add", operator.add), ("sub", operator.sub), ("mul", operator.mul), ("truediv", operator.truediv)):
    setattr(Th, f"__{_n}__", (lambda op: lambda s, o: s._bin(o, op))(_op))
    setattr(Th, f"__r{_n}__", (lambda op: lambda s, o: s._bin(o, op, True))(_op))


class _Fresh(dict):
    """Latent values of the discovery pass: one fresh in-support tensor per address."""

    def __missing__(self, k):
        self[k] = torch.full((1,), 0.5, dtype=torch.float64)
        return self[k]


def _addr(a):
    return a if isinstance(a, tuple) else (a,)


def _log_density(kind, a, x, latent, dtype):
    import torch.distributions as TD

    nan, ninf = torch.full((), float("nan"), dtype=dtype), torch.full((), float("-inf"), dtype=dtype)
    if kind == "normal":
        return torch.where(a[1] > 0, TD.Normal(a[0], a[1], validate_args=False).log_prob(x), nan)
    if kind in ("gamma", "beta"):
        D = TD.Gamma if kind == "gamma" else TD.Beta
        inside = (x > 0) if kind == "gamma" else ((x > 0) & (x < 1))
        xs = torch.where(inside, x, torch.full((), 0.5, dtype=dtype))
        lp = torch.where((a[0] > 0) & (a[1] > 0), D(a[0], a[1], validate_args=False).log_prob(xs), nan)
        return torch.where(inside, lp, ninf if latent else nan)
    p = a[0]
    return torch.where((p >= 0) & (p <= 1), torch.where(x != 0, torch.log(p), torch.log1p(-p)), nan)


def _tolerance(kind, a, x, lp):
    xs_, as_ = x.numpy(), [v.numpy() for v in a]
    tol = (normal_tolerance(xs_, *as_) if kind == "normal" else gamma_tolerance(xs_, *as_) if kind == "gamma" else
           beta_tolerance(xs_, *as_) if kind == "beta" else bernoulli_tolerance(lp.numpy()))
    return np.nan_to_num(np.asarray(tol, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0)


def _law(kind, a, x):
    """('pit', u) for Normal / Gamma, ('z', standardised residual) for Beta / flip — float64 arguments."""
    import torch.distributions as TD

    if kind == "normal":
        return "pit", TD.Normal(a[0], a[1], validate_args=False).cdf(x)
    if kind == "gamma":
        return "pit", torch.special.gammainc(a[0] + torch.zeros_like(x), a[1] * x)
    if kind == "beta":
        s = a[0] + a[1]
        return "z", (x - a[0] / s) / torch.sqrt(a[0] * a[1] / (s * s * (s + 1.0)))
    return "z", ((x != 0).to(x.dtype) - a[0]) / torch.sqrt(a[0] * (1.0 - a[0]))


def namespace(*sources):
    """The namespace the sources are executed in: `normal(..) @ addr` and a `@gen` callee `f(..) @ addr` go through the `run`
    the namespace holds at the time (run_body installs it)."""
    ns = {"torch": torch, "_run": None}

    class Dist:
        def __init__(self, kind, a):
            self.kind, self.a = kind, a

        def __matmul__(self, addr):
            return ns["_run"].site(self.kind, self.a, addr)

    class Call:
        def __init__(self, fn, a):
            self.fn, self.a = fn, a

        def __matmul__(self, addr):
            return ns["_run"].call(self.fn, self.a, addr)

    for kind in ("normal", "gamma", "beta", "flip"):
        ns[kind] = (lambda k: lambda *a: Dist(k, a))(kind)
    ns["gen"] = lambda fn: (lambda *a: Call(fn, a))
    for s in sources:
        if s:
            exec(s, ns)  # noqa: S102 - the body under test, executed as written
    return ns


class Run:
    """One execution of `ns[name](*args)`: `sites` in order — address, kind, role, arguments, value, log-density (and, in
    float64, its specification bound) — and `ret`.  `values[address]`: a latent site's value; `observed[address]`: an observed
    one's."""

    def __init__(self, ns, name, args, values, observed, dtype=torch.float64, discover=False):
        self.dtype, self.values, self.observed, self.discover = dtype, values, observed, discover
        self.sites, self.prefix = [], ()
        ns["_run"] = self
        with torch.no_grad():
            self.ret = ns[name](*args)
        ns["_run"] = None

    def tensor(self, v):
        if isinstance(v, Th):
            v = v.use()
        return v.to(self.dtype) if isinstance(v, torch.Tensor) else torch.as_tensor(float(v), dtype=self.dtype)

    def call(self, fn, a, addr):
        outer, self.prefix = self.prefix, self.prefix + _addr(addr)
        try:
            return fn(*a)
        finally:
            self.prefix = outer

    def site(self, kind, a, addr):
        full = self.prefix + _addr(addr)
        latent = full not in self.observed
        a = [self.tensor(v) for v in a]
        if self.discover and latent:
            x = self.values[full]
            self.sites.append(dict(addr=full, kind=kind, latent=True, a=a, x=x))
            return x
        x = self.tensor(self.values[full] if latent else self.observed[full])
        lp = _log_density(kind, a, x, latent, self.dtype)
        s = dict(addr=full, kind=kind, latent=latent, a=a, x=x, lp=lp)
        if self.dtype == torch.float64:
            s["tol"] = _tolerance(kind, a, x, lp)
        self.sites.append(s)
        return x


def _theta_arg(theta, log):
    return () if theta is None else (tuple(Th(float(np.float32(v)), log) for v in np.asarray(theta).reshape(-1)),)


def components(ns, name, n_args_carry, observed, theta):
    """{latent address: carry component} of one body, by identity of what it returns (a discovery pass over fresh values)."""
    fresh = _Fresh()
    carry = ()
    if n_args_carry:
        c = tuple(torch.full((1,), 0.5, dtype=torch.float64) for _ in range(n_args_carry))
        carry = (c[0] if n_args_carry == 1 else c,)
    run = Run(ns, name, carry + _theta_arg(theta, []), fresh, {k: 0.5 for k in observed}, discover=True)
    ret = run.ret if isinstance(run.ret, (tuple, list)) else (run.ret,)
    comp = {addr: c for addr, v in fresh.items() for c, r in enumerate(ret) if r is v}
    missing = [s["addr"] for s in run.sites if s["latent"] and s["addr"] not in comp]
    assert not missing, f"latent sites {missing} of `{name}` are not carry components: the history does not determine them"
    return comp, len(ret)


def theta_uses(init_src, step_src, obs_addrs, theta, proposals=None):
    """Every value derived from `theta` on the host that reaches a traced value or a site argument, in order of use, over one
    execution of init and step (and the proposals): float64 arithmetic on the f32 theta, not yet rounded."""
    p = proposals or {}
    ns = namespace(init_src, step_src, p.get("step"), p.get("init"))
    observed = {_addr(a): 0.5 for a in obs_addrs}
    log = []
    _, n_state = components(ns, "init", 0, observed, theta)
    one = lambda: torch.full((1,), 0.5, dtype=torch.float64)  # noqa: E731
    carry = tuple(one() for _ in range(n_state))
    carry = carry[0] if n_state == 1 else carry
    y = tuple(one() for _ in observed)
    y = y[0] if len(y) == 1 else y
    fresh = _Fresh()
    if p.get("init"):
        Run(ns, "init_proposal", (y,) + _theta_arg(theta, log), fresh, observed)
    Run(ns, "init", _theta_arg(theta, log), fresh, observed)
    if p.get("step"):
        Run(ns, "step_proposal", (carry, y) + _theta_arg(theta, log), fresh, observed)
    Run(ns, "step", (carry,) + _theta_arg(theta, log), fresh, observed)
    return log


class Replay:
    """What `replay64` leaves: inc [T, n] the steps' own log-weights, lw [T, n] what the filter records (accumulated where a
    step did not resample), tol [T, n] the summed specification bounds, comps {component: [T, n]} the carry components that are
    not latent draws, laws {address: [(kind, values [n]) per step]}, proposed {address: [bool per step]}."""


def replay64(init_src, step_src, history, ancestors, log_weights, resampled, obs, theta=None, proposals=None, dtype=torch.float64):
    """`history`: [T, n] (a tuple of them for a multi-component carry; an int32 column is read as its value); `ancestors`
    int32 [T, n]; `log_weights` f32 [T, n], the RECORDED ones (a row that did not resample accumulates onto them);
    `resampled` [T] or None (every step resampled); `obs` {address: [T]}; `theta`: the row of a parameterised body;
    `proposals`: random_proposal's result for a guided filter."""
    hist = [np.asarray(h) for h in (history if isinstance(history, (tuple, list)) else (history,))]
    anc, lwr = np.asarray(ancestors).astype(np.int64), np.asarray(log_weights, dtype=np.float32)
    T, n = lwr.shape
    res = np.ones(T, dtype=bool) if resampled is None else np.asarray(resampled).astype(bool).reshape(-1)
    obs = {_addr(k): np.asarray(v) for k, v in obs.items()}
    p = proposals or {}
    ns = namespace(init_src, step_src, p.get("step"), p.get("init"))
    comp_i, n_state = components(ns, "init", 0, obs, theta)
    comp_s, n_step = components(ns, "step", n_state, obs, theta)
    assert n_state == n_step == len(hist), (n_state, n_step, len(hist))
    t64 = lambda v: torch.from_numpy(np.ascontiguousarray(v).astype(np.float64)).to(dtype)  # noqa: E731
    out = Replay()
    out.inc, out.lw, out.tol = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
    out.comps, out.laws, out.proposed, out.theta_log = {}, {}, {}, []
    want = dtype == torch.float64
    for t in range(T):
        comp = comp_i if t == 0 else comp_s
        values = {a: t64(hist[c][t]) for a, c in comp.items()}
        observed = {a: float(v[t]) for a, v in obs.items()}
        th = _theta_arg(theta, out.theta_log)
        ys = tuple(torch.as_tensor(float(v[t]), dtype=dtype) for v in obs.values())
        ys = (ys[0] if len(ys) == 1 else ys,)
        carry = ()
        if t > 0:
            old = tuple(t64(h[t - 1][anc[t]]) for h in hist)
            carry = (old[0] if n_state == 1 else old,)
        q = {}
        prop = p.get("init" if t == 0 else "step")
        if prop:
            q = {s["addr"]: s for s in Run(ns, "init_proposal" if t == 0 else "step_proposal", carry + ys + th, values, observed, dtype).sites}
        run = Run(ns, "init" if t == 0 else "step", carry + th, values, observed, dtype)
        inc, tol = torch.zeros(n, dtype=dtype), np.zeros(n)
        for s in run.sites:
            terms = [(s, 1.0)] if not s["latent"] else ([(s, 1.0), (q[s["addr"]], -1.0)] if s["addr"] in q else [])
            for u, sign in terms:
                inc = inc + sign * u["lp"]
                tol = tol + (u["tol"] if want else 0.0)
            if s["latent"] and want:
                law = q.get(s["addr"], s)
                kind, v = _law(law["kind"], law["a"], law["x"])
                out.laws.setdefault(s["addr"], []).append((kind, (v + torch.zeros(n, dtype=dtype)).numpy()))
                out.proposed.setdefault(s["addr"], []).append(s["addr"] in q)
        inc = inc.numpy().astype(np.float64)
        out.inc[t], out.tol[t] = inc, tol
        if t > 0 and not res[t]:
            with np.errstate(invalid="ignore"):
                out.lw[t] = (lwr[t - 1][anc[t]].astype(np.float64) + inc) if want else (lwr[t - 1][anc[t]] + inc.astype(np.float32))
            out.tol[t] = out.tol[t] + 2.0 ** -24 * np.nan_to_num(np.abs(out.lw[t]), nan=0.0, posinf=0.0)
        else:
            out.lw[t] = inc
        ret = run.ret if isinstance(run.ret, (tuple, list)) else (run.ret,)
        for c, r in enumerate(ret):
            if c not in comp.values():
                r = r.use() if isinstance(r, Th) else r
                r = r.to(dtype) if isinstance(r, torch.Tensor) else torch.as_tensor(float(r), dtype=dtype)
                out.comps.setdefault(c, np.zeros((T, n)))[t] = (r + torch.zeros(n, dtype=dtype)).numpy()
    out.latent_components = (comp_i, comp_s)
    return out


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def ks_distance(u):
    u = np.sort(np.asarray(u, dtype=np.float64).reshape(-1))
    k = np.arange(1, u.size + 1)
    return float(max(np.max(k / u.size - u), np.max(u - (k - 1) / u.size)))


def ks_bound(N):
    return math.sqrt(ALPHA_LOG / (2.0 * N))


class Reference:
    """float64 truth of one recorded run, its tolerances and whether the case is conditioned well enough to be compared.
    tol = the summed pinned bounds + FLOOR_FACTOR * floor; floor = max |replay64(float32) - replay64(float64)| over the finite
    entries, per quantity ("lw", and "c<k>" per carry component that is not a latent draw: no pinned bound applies to those,
    and FLOOR_FACTOR roundings of the result, 2^-24 |ref| each, stand for the final rounding of a program the floor of a
    trivial expression does not see).  Neither replay touches project code."""

    def __init__(self, result, init_src, step_src, obs, theta=None, proposals=None):
        a = (init_src, step_src, _np(result.history), _np(result.ancestors), _np(result.log_weight_history), _np(result.resampled), obs)
        r64 = replay64(*a, theta=theta, proposals=proposals)
        r32 = replay64(*a, theta=theta, proposals=proposals, dtype=torch.float32)
        self.r64 = r64
        self.ref, self.tol, self.floor, self.reasons = {}, {}, {}, []
        items = [("lw", r64.lw, r32.lw, r64.tol)]
        items += [(f"c{c}", r64.comps[c], r32.comps[c], FLOOR_FACTOR * 2.0 ** -24 * np.abs(r64.comps[c])) for c in sorted(r64.comps)]
        for what, x64, x32, spec in items:
            fin = np.isfinite(x64) & np.isfinite(x32)
            with np.errstate(invalid="ignore"):
                floor = float(np.abs(x32 - x64)[fin].max()) if fin.any() else 0.0
            tol = spec + FLOOR_FACTOR * floor
            self.ref[what], self.tol[what], self.floor[what] = x64, tol, floor
            ok = np.isfinite(x64)
            if ok.mean() < MIN_FINITE:
                self.reasons.append(f"{what}: the reference is finite on {ok.mean():.2f} of the entries")
            elif tol[ok].max() > COND_REL * max(1.0, float(np.median(np.abs(x64[ok])))):
                self.reasons.append(f"{what}: tol {tol[ok].max():.3g} above {COND_REL} * max(1, median |ref| = "
                                    f"{np.median(np.abs(x64[ok])):.3g}) (f32 floor {floor:.3g})")
        self.kept = not self.reasons


def _np(v):
    if v is None:
        return None
    if isinstance(v, (tuple, list)):
        return tuple(_np(x) for x in v)
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def law_samples(ref, free=None):
    """{(address, 'init' | 'step'): (kind, values)} of one run: step 0 over its n draws, steps 1 .. T-1 pooled.  `free`: the
    slots that were drawn (a conditional run: all but the last)."""
    out = {}
    for addr, rows in ref.r64.laws.items():
        cut = [(k, v[free] if free is not None else v) for k, v in rows]
        out[(addr, "init")] = (cut[0][0], cut[0][1])
        if len(cut) > 1:
            assert len({k for k, _ in cut[1:]}) == 1
            out[(addr, "step")] = (cut[1][0], np.concatenate([v for _, v in cut[1:]]))
    return out


def check_laws(samples, context=""):
    """`samples`: law_samples of one run or several (pooled per key).  A PIT's Kolmogorov distance stays below
    sqrt(ln(2e6) / (2 N)) (DKW at alpha = 1e-6), |sum r| / sqrt(N) of a standardised residual below 5.
    -> {"ks": largest distance / bound, "z": largest |z| / bound}."""
    pooled = {}
    for s in samples if isinstance(samples, (list, tuple)) else [samples]:
        for k, (kind, v) in s.items():
            pooled.setdefault(k, (kind, []))[1].append(v)
    worst = {"ks": 0.0, "z": 0.0, "ks_abs": 0.0, "z_abs": 0.0}
    for k, (kind, vs) in pooled.items():
        v = np.concatenate(vs)
        assert np.isfinite(v).all(), f"law of {k}: the reference is not finite\n{context}"
        if kind == "pit":
            d, b = ks_distance(v), ks_bound(v.size)
            worst["ks"], worst["ks_abs"] = max(worst["ks"], d / b), max(worst["ks_abs"], d)
            assert d <= b, f"law of {k}: Kolmogorov distance {d:.4f} of {v.size} draws given their parents, bound {b:.4f}\n{context}"
        else:
            z = abs(float(v.sum())) / math.sqrt(v.size)
            worst["z"], worst["z_abs"] = max(worst["z"], z / Z_BOUND), max(worst["z_abs"], z)
            assert z <= Z_BOUND, f"law of {k}: |sum r| / sqrt(N) = {z:.2f} over {v.size} draws given their parents, bound {Z_BOUND}\n{context}"
    return worst


def check_run(result, init_src=None, step_src=None, obs=None, theta=None, proposals=None, ref=None, laws=True, free=None, context=""):
    """An `SMCResult` with history against the float64 replay of the source text: the recorded log-weights of every step, the
    carry components that are not latent draws and (`laws`) every latent's law given its parents.  Infinite reference entries
    must match exactly; a NaN is allowed only where the reference is NaN.  -> {"lw": worst err / tol, "expr": ..., "ks", "z"}.
    `ref`: a Reference of this very result, when the caller has built it to decide whether the case is compared."""
    ref = Reference(result, init_src, step_src, obs, theta, proposals) if ref is None else ref
    hist = _np(result.history)
    hist = hist if isinstance(hist, tuple) else (hist,)
    stats = {"lw": 0.0, "expr": 0.0}
    for what in ref.ref:
        got = np.asarray(_np(result.log_weight_history) if what == "lw" else hist[int(what[1:])], dtype=np.float64)
        r, tol = ref.ref[what], ref.tol[what]
        assert got.shape == r.shape, (what, got.shape, r.shape)
        bad = misses(got, r, tol)
        fin = np.isfinite(r) & np.isfinite(got)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(fin & (tol > 0), np.abs(got - r) / tol, 0.0)
        if bad.any():
            k = np.unravel_index(int(np.argmax(np.where(bad, np.where(fin, np.abs(got - r), np.inf), -1.0))), r.shape)
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries miss the float64 reference; at (step, particle) {k}: "
                                 f"got {got[k]!r}, reference {r[k]!r}, tol {tol[k]:.3g} (f32 floor {ref.floor[what]:.3g})\n{context}")
        key = "lw" if what == "lw" else "expr"
        stats[key] = max(stats[key], float(ratio.max()) if ratio.size else 0.0)
    if laws:
        stats.update(check_laws(law_samples(ref, free), context))
    return stats


# ---- the project's side of a case (the only part that imports the package) -----------------------------------------------------
def build_model(init_src, step_src, params=False):
    from genjax import beta, flip, gamma, gen, normal
    from genjax._amd.smc_plan import StateSpaceModel

    ns = {"normal": normal, "gamma": gamma, "beta": beta, "flip": flip, "torch": torch, "gen": gen}
    exec(init_src + "\n" + step_src, ns)  # noqa: S102 - generated by random_ssm above, or MIXED
    return StateSpaceModel(gen(ns["init"]), gen(ns["step"]), params=THETA if params else ())


def build_proposals(proposals):
    """-> (step_proposal, init_proposal or None) as `@gen` functions."""
    from genjax import beta, flip, gamma, gen, normal

    ns = {"normal": normal, "gamma": gamma, "beta": beta, "flip": flip, "torch": torch}
    exec(proposals["step"] + "\n" + (proposals["init"] or ""), ns)  # noqa: S102 - generated by random_proposal above
    return gen(ns["step_proposal"]), (gen(ns["init_proposal"]) if proposals["init"] else None)


def observations_of(obs):
    """{address: [T]} -> the ChoiceMap a filter takes (leaves in the dictionary's order)."""
    from genjax import ChoiceMap

    chm = None
    for a, v in obs.items():
        e = ChoiceMap.entry(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)), *_addr(a))
        chm = e if chm is None else chm | e
    return chm
