"""Random and interleaved tempered bodies against a float64 evaluation of their own source text.

The replays the tempered suites pin the kernels to (temper_ref.Assess, plate_ref.Assess, pointwise_ref.terms) are built from
the TRACER's site table: a lowering mistake (an operand on the wrong side of a subtraction, a reference to the wrong latent,
two data columns swapped) is in the kernel and in the replay alike.  This module is the reference that shares nothing with
the lowering: `evaluate64` executes the body's source text with small distribution objects of its own over torch float64
tensors — no PlanTracer, no SymExpr, no ABI, no oracle, no kernel — and `check64` compares with a tolerance DERIVED from the
bounds the suite already pins for the spec's arithmetic and from the f32 rounding floor of the very case, measured on the
reference alone.  Used by tests/test_temper_fuzz_cpu.py (oracle backend) and tests/test_gpu_temper_fuzz.py (HIP backend).
The same execution gives the LAW of every replicated draw of a plated site (include/gjx_predictive.h): `predictive_laws` holds
the draws of the predictive replay and kernels to it, at ssm_fuzz's derived bounds (tests/test_predictive_fuzz_cpu.py,
tests/test_gpu_predictive_fuzz.py)."""

import math
import re

import numpy as np
import torch

from dist_range_ref import beta_tolerance, gamma_tolerance
from fuzz_models import _expr, _pos

DATA = ("xs", "zs", "ps")   # real, real and positive data columns; `s` is a positive scalar argument, `t` a real one
GAMMA_OUTSIDE = (-0.5, 0.0, -1e-30)
BETA_OUTSIDE = (-0.25, 0.0, 1.0, 1.5)
COND_REL = 1e-3             # a case is kept while tol <= COND_REL * max(1, median |reference|) ...
MIN_FINITE = 0.9            # ... and the reference is finite on this share of its entries
FLOOR_FACTOR = 4.0          # the spec's 2-ulp exp / log against libm's, and another legal operation order


# ---- the generator ---------------------------------------------------------------------------------------------------------
# (reads the TEXT of the two `where` templates of fuzz_models._expr: reword them there and here together)
_WHERE = re.compile(r"torch\.where\(\(?(\w+) [<>] (\w+)?")


def _lowers_by_design(e, data_names):
    """False for what temper.lower refuses BY DESIGN in a plated argument: a `where` whose condition holds a data column (an
    untraced tensor condition; `|` of a traced comparison and a data comparison is `|` on a non-condition)."""
    return not any(g in data_names for m in _WHERE.finditer(e) for g in m.groups() if g)


def _draw(rng, make, data_names):
    for _ in range(20):
        e = make()
        if _lowers_by_design(e, data_names):
            return e
    return repr(round(float(rng.uniform(0.3, 1.5)), 3))


def _names(e):
    return set(re.findall(r"\b(?:v\d+|xs|zs|ps)\b", e))


def random_tempered_model(rng):
    """-> (source of `def model(xs, zs, ps, s, t): ...`, sites as (name, role, kind)): 3 to 8 sites in any order of roles.
    role 'latent' (normal, gamma, beta), 'scalar' (an observed site with a scalar value: the three and flip(sigmoid(.))),
    'plated' (the same four kinds, observed over a data column of its own; its arguments may read xs, zs, ps and the VALUES of
    earlier plated sites).  Arguments are fuzz_models' expressions; positive arguments are positive by construction."""
    lines, sites = [], []
    reals, poss, units = [], [], []   # latents by kind
    d_reals, d_poss = list(DATA), ["ps"]  # what a plated site may read next to them
    n_sites = int(rng.integers(3, 9))
    for q in range(n_sites):
        name = f"v{q}"
        r = rng.random()
        role = "latent" if q == 0 or r < 0.4 else ("scalar" if r < 0.6 else "plated")
        if q == n_sites - 1 and not any(ro != "latent" for _, ro, _ in sites):
            role = "plated"  # (at least one observed site)
        kind = str(rng.choice(["normal", "normal", "gamma", "beta"] if role == "latent" else ["normal", "normal", "gamma", "beta", "flip"]))
        pool = reals + poss + units
        if role == "plated":
            pool, ppool, dn = pool + d_reals, poss + d_poss, set(d_reals)
        else:
            ppool, dn = list(poss), set()
        ex = lambda: _draw(rng, lambda: _expr(rng, pool, ["t"]), dn)            # noqa: E731
        po = lambda: _draw(rng, lambda: _pos(rng, pool, ppool, ["s"]), dn)      # noqa: E731
        if kind == "normal":
            call = f"normal({ex()}, {po()})"
        elif kind in ("gamma", "beta"):
            call = f"{kind}({po()}, {po()})"
        else:
            e = ex()
            # (torch.sigmoid of a Python float is no tensor operation: a logit without a latent or a column is a literal p)
            call = f"flip(torch.sigmoid({e}))" if _names(e) else f"flip({round(float(rng.uniform(0.1, 0.9)), 3)})"
        lines.append(f"    {name} = {call} @ '{name}'")
        sites.append((name, role, kind))
        if role == "latent":
            {"normal": reals, "gamma": poss, "beta": units}[kind].append(name)
        elif role == "plated" and kind != "flip":
            d_reals.append(name)
            if kind == "gamma":
                d_poss.append(name)
    return "def model(xs, zs, ps, s, t):\n" + "\n".join(lines) + "\n", sites


INTERLEAVED = '''def model(xs, zs, ps, s, t):
    a = normal(0.0, 1.5) @ "a"
    y1 = normal(a * xs + 0.25, s) @ "y1"
    g = gamma(2.0, 1.5) @ "g"
    normal(a + 0.5, 0.7) @ "o1"
    b = normal(a * 0.5 - 0.2, 0.2 + 0.1 * g) @ "b"
    gamma(g * 1.5 + 0.2, torch.exp(b * zs * 0.3)) @ "y2"
    u = beta(g + 0.5, 2.0 + b * b) @ "u"
    flip(torch.sigmoid(b * xs - u)) @ "y3"
    beta(u * ps + 0.5, 1.0 + y1 * y1) @ "y4"
'''
# latent, plate, latent, scalar observed, latent (declared after a plate; reads `a`, whose position stays, and `g`, whose position
# temper.prior_table CHANGES: its conditional law is checked on stage 0), plate (a Gamma with a latent shape and a data-dependent
# rate), latent (a Beta whose arguments read `g` affinely and `b` inside a PROGRAM: both references are renumbered), plate,
# plate (a Beta; reads an earlier plate's VALUE as data).
INTERLEAVED_SITES = (("a", "latent", "normal"), ("y1", "plated", "normal"), ("g", "latent", "gamma"), ("o1", "scalar", "normal"),
                     ("b", "latent", "normal"), ("y2", "plated", "gamma"), ("u", "latent", "beta"), ("y3", "plated", "flip"),
                     ("y4", "plated", "beta"))


def random_inputs(rng, sites, D):
    """-> (args (xs, zs, ps, s, t), observed {name: value}): f32 numpy columns of D rows, Python scalars."""
    f = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    args = (f(rng.uniform(-1.0, 1.0, D)), f(0.8 * rng.standard_normal(D)), f(rng.uniform(0.3, 2.0, D)),
            round(float(rng.uniform(0.3, 2.0)), 3), round(float(rng.uniform(-1.5, 1.5)), 3))
    obs = {}
    for name, role, kind in sites:
        if role == "scalar":
            obs[name] = (bool(rng.integers(2)) if kind == "flip" else
                         round(float({"normal": rng.uniform(-2, 2), "gamma": rng.uniform(0.2, 3.0), "beta": rng.uniform(0.1, 0.9)}[kind]), 3))
        elif role == "plated":
            obs[name] = (rng.integers(0, 2, D).astype(bool) if kind == "flip" else
                         f({"normal": rng.standard_normal(D), "gamma": rng.gamma(2.0, 0.5, D) + 0.05, "beta": rng.uniform(0.05, 0.95, D)}[kind]))
    return args, obs


def latent_columns(rng, sites, n, outside=False, centred=False):
    """{name: f32 [n]} per latent.  `outside`: every fourth value of a Gamma / Beta latent outside its support (negative, zero
    and, for Beta, 1 and above); `centred`: a tenth of a unit wide around one centre per latent (pointwise_ref.centred_columns'
    reason: a row's terms then spread a few nats, below pointwise_ref.LSE_MAX_SPREAD)."""
    out = {}
    for name, role, kind in sites:
        if role != "latent":
            continue
        if centred:
            c = {"normal": rng.uniform(-0.5, 0.5), "gamma": rng.uniform(0.6, 1.5), "beta": rng.uniform(0.3, 0.7)}[kind]
            z = 0.1 * rng.standard_normal(n)
            col = c + z if kind == "normal" else (c * np.exp(z) if kind == "gamma" else np.clip(c + 0.3 * z, 0.02, 0.98))
        else:
            col = {"normal": lambda: rng.standard_normal(n), "gamma": lambda: rng.gamma(2.0, 0.5, n) + 0.01,
                   "beta": lambda: np.clip(rng.beta(2.0, 2.0, n), 0.01, 0.99)}[kind]()
        col = col.astype(np.float32)
        if outside and kind in ("gamma", "beta"):
            bad = np.asarray(GAMMA_OUTSIDE if kind == "gamma" else BETA_OUTSIDE, dtype=np.float32)
            col[::4] = bad[np.arange(len(col[::4])) % len(bad)]
        out[name] = col
    return out


def inside(sites, latents):
    """bool [n]: the particles whose Gamma / Beta latents all lie in their open support."""
    ok = np.ones(len(next(iter(latents.values()))), dtype=bool)
    for name, role, kind in sites:
        if role == "latent" and kind == "gamma":
            ok &= latents[name] > 0
        elif role == "latent" and kind == "beta":
            ok &= (latents[name] > 0) & (latents[name] < 1)
    return ok


# ---- the specification bounds of one log-density ---------------------------------------------------------------------------
# Arrays of any (broadcast) shape.  Gamma and Beta: dist_range_ref.gamma_tolerance / beta_tolerance at the float64 arguments.  Normal
# and Bernoulli: the same construction from the same pins (test_oracle_pinning.py test_math_spec_accuracy):
# 1e-6 * (sum |terms| + sum |their coefficients|).
#   Normal     -z^2 / 2 - log(scale) - log(2 pi) / 2, z = (x - loc) / scale.  log is pinned to 2e-7 * max(1, |log|): the term
#              log(scale), coefficient 1, is off by at most 2e-7 * (1 + |log scale|); z^2 / 2 carries the f32 roundings of the
#              difference, the quotient, the square and the halving (6e-8 relative each, the square doubling the first two):
#              below 4e-7 * z^2 / 2; the two adds round the partial sums (6e-8 of them).  Together below
#              1e-6 * (z^2 / 2 + |log scale| + log(2 pi) / 2 + 1).
#   Bernoulli  log p (value 1) or log(1 - p) (value 0): 2e-7 * max(1, |log|) for the logarithm and 6e-8 absolute for the f32
#              rounding of 1 - p (dist_range_ref.check_bernoulli_logpdf): below 1e-6 * (|log| + 1).

def normal_tolerance(x, loc, scale):
    x, loc, scale = (np.asarray(v, dtype=np.float64) for v in (x, loc, scale))
    with np.errstate(all="ignore"):
        z = (x - loc) / scale
        return 1e-6 * (0.5 * z * z + np.abs(np.log(scale)) + 0.5 * math.log(2.0 * math.pi) + 1.0)


def bernoulli_tolerance(logp):
    return 1e-6 * (np.abs(np.asarray(logp, dtype=np.float64)) + 1.0)


# ---- the float64 evaluator -----------------------------------------------------------------------------------------------
class Evaluation:
    """What one execution of a body leaves: lp, ll [n]; per plated site its [n, D] table; with the float64 dtype also the
    summed specification bounds of every entry (`tol_*`) and the probability-integral transform of every Normal and Gamma
    latent given its parents (`pit`)."""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        self.lp, self.ll = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
        self.tol_lp, self.tol_ll = np.zeros(n), np.zeros(n)
        self.tables, self.tol_tables, self.pit, self.order = {}, {}, {}, []
        self.laws, self.kinds = {}, {}  # plated address: (kind, float64 arguments [n, D]); latent address: kind

    def terms(self):
        """[D, n]: the f32 sum, in table order, of the plated sites' tables (pointwise_ref.terms' composition), and the sum of
        their bounds."""
        out, tol = None, 0.0
        with np.errstate(invalid="ignore", over="ignore"):
            for name in self.order:
                t = self.tables[name].numpy().T.astype(np.float32)
                out = t if out is None else (out + t).astype(np.float32)
                tol = tol + (self.tol_tables[name].T if name in self.tol_tables else 0.0)
        return out.astype(np.float64), tol


def evaluate64(source, latents, observed, args, dtype=torch.float64):
    """Execute `source` (`def model(xs, zs, ps, s, t)`) in a namespace of its own.  `latents` {address: f32 [n]},
    `observed` {address: scalar or [D] column}, `args` the five model arguments (columns as arrays).  A site's `@ address`
    looks its value up — a latent column as [n, 1], a scalar, a data column as [1, D] — adds its log-density (torch.distributions
    in `dtype`; Bernoulli as log p / log1p(-p)) to lp or ll, and returns the value.  The support rule of include/gjx_temper.h
    is restated: a latent Gamma value <= 0 or a Beta value outside (0, 1) gives the term -inf.  A distribution argument outside
    its domain (scale, shape, rate <= 0, p outside [0, 1]) makes the reference NaN there: no truth to compare with.
    Per plated address `laws` keeps the site's kind and its arguments broadcast to [n, D]: the law of the replicated draw
    y_rep[d, i] of include/gjx_predictive.h.  That header's SHADOW rule is restated by what `@` returns: a plated site that reads
    an earlier plated site's value reads the OBSERVED column (the value returned here), never that site's replicated draw."""
    import torch.distributions as TD

    n = len(next(iter(latents.values())))
    ev = Evaluation(n, dtype)
    want_tol = dtype == torch.float64

    def tensor(v):
        if isinstance(v, torch.Tensor):
            return v.to(dtype)
        return torch.as_tensor(np.asarray(v, dtype=np.float64)).to(dtype)

    def site(kind, a, addr):
        if addr in latents:
            role, x = "latent", tensor(latents[addr]).reshape(n, 1)
        else:
            v = np.asarray(observed[addr])
            role, x = ("plated", tensor(v).reshape(1, -1)) if v.ndim == 1 else ("scalar", tensor(v))
        a = [tensor(v) for v in a]
        nan = torch.full((), float("nan"), dtype=dtype)
        if kind == "normal":
            lp = torch.where(a[1] > 0, TD.Normal(a[0], a[1], validate_args=False).log_prob(x), nan)
        elif kind == "gamma":
            lp = torch.where((a[0] > 0) & (a[1] > 0), TD.Gamma(a[0], a[1], validate_args=False).log_prob(x), nan)
        elif kind == "beta":
            lp = torch.where((a[0] > 0) & (a[1] > 0), TD.Beta(a[0], a[1], validate_args=False).log_prob(x), nan)
        else:
            p = a[0]
            lp = torch.where((p >= 0) & (p <= 1), torch.where(x != 0, torch.log(p), torch.log1p(-p)), nan)
        shape = (n, x.shape[1] if role == "plated" else 1)
        lp = lp + torch.zeros(shape, dtype=dtype)
        if role == "latent":
            if kind == "gamma":
                lp = torch.where(x > 0, lp, torch.full((), float("-inf"), dtype=dtype))
            elif kind == "beta":
                lp = torch.where((x > 0) & (x < 1), lp, torch.full((), float("-inf"), dtype=dtype))
        tol = None
        if want_tol:
            xs_, as_ = x.numpy(), [v.numpy() for v in a]
            tol = (normal_tolerance(xs_, *as_) if kind == "normal" else gamma_tolerance(xs_, *as_) if kind == "gamma" else
                   beta_tolerance(xs_, *as_) if kind == "beta" else bernoulli_tolerance(lp.numpy()))
            tol = np.nan_to_num(np.broadcast_to(tol, shape).astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
        if role == "latent":
            ev.kinds[addr] = kind
        elif role == "plated":
            ev.laws[addr] = (kind, [np.broadcast_to(v.to(torch.float64).numpy(), shape) for v in a[:1 if kind == "flip" else 2]])
        if role == "latent":
            ev.lp = ev.lp + lp[:, 0]
            if want_tol:
                ev.tol_lp = ev.tol_lp + tol[:, 0]
                if kind == "normal":
                    ev.pit[addr] = (TD.Normal(a[0], a[1], validate_args=False).cdf(x) + torch.zeros(shape, dtype=dtype))[:, 0].numpy()
                elif kind == "gamma":
                    ev.pit[addr] = (torch.special.gammainc(a[0] + torch.zeros(shape, dtype=dtype), a[1] * x))[:, 0].numpy()
        elif role == "scalar":
            ev.ll = ev.ll + lp[:, 0]
            if want_tol:
                ev.tol_ll = ev.tol_ll + tol[:, 0]
        else:
            ev.ll = ev.ll + lp.sum(dim=1)
            ev.tables[addr], ev.order = lp, ev.order + [addr]
            if want_tol:
                ev.tol_ll = ev.tol_ll + tol.sum(axis=1)
                ev.tol_tables[addr] = tol
        return x

    class Dist:
        def __init__(self, kind, a):
            self.kind, self.a = kind, a

        def __matmul__(self, addr):
            return site(self.kind, self.a, addr)

    ns = {"torch": torch}
    for kind in ("normal", "gamma", "beta", "flip"):
        ns[kind] = (lambda k: lambda *a: Dist(k, a))(kind)
    exec(source, ns)  # noqa: S102 - the body under test, executed as written
    with torch.no_grad():
        ns["model"](*[tensor(v).reshape(1, -1) if np.ndim(v) == 1 else float(v) for v in args])
    return ev


class Reference:
    """float64 truth of one case, its tolerance and whether the case is conditioned well enough to be compared.

    tol (per entry) = the summed specification bounds + FLOOR_FACTOR * floor, floor = max |evaluate64(float32) -
    evaluate64(float64)| over the case's finite entries — per quantity (lp, ll, the pointwise terms); neither evaluation touches
    project code.  `live` [n]: the particles whose conditioning counts (all, unless latents were planted outside their
    support)."""

    def __init__(self, source, latents, observed, args, live=None):
        e64 = evaluate64(source, latents, observed, args)
        e32 = evaluate64(source, latents, observed, args, dtype=torch.float32)
        self.e64 = e64
        n = e64.n
        live = np.ones(n, dtype=bool) if live is None else live
        self.ref, self.tol, self.floor, self.reasons = {}, {}, {}, []
        items = [("lp", e64.lp.numpy(), e32.lp.numpy(), e64.tol_lp, live), ("ll", e64.ll.numpy(), e32.ll.numpy(), e64.tol_ll, live)]
        if e64.tables:
            t64, ttol = e64.terms()
            items.append(("terms", t64, e32.terms()[0], ttol, np.broadcast_to(live, t64.shape)))
        for what, r64, r32, spec, lv in items:
            r64, r32 = np.asarray(r64, dtype=np.float64), np.asarray(r32, dtype=np.float64)
            fin = np.isfinite(r64) & np.isfinite(r32)
            with np.errstate(invalid="ignore"):
                floor = float(np.abs(r32 - r64)[fin].max()) if fin.any() else 0.0
            tol = spec + FLOOR_FACTOR * floor
            self.ref[what], self.tol[what], self.floor[what] = r64, tol, floor
            ok = np.isfinite(r64) & lv
            share = ok.sum() / max(1, lv.sum())
            if share < MIN_FINITE:
                self.reasons.append(f"{what}: the reference is finite on {share:.2f} of the entries")
            elif tol[ok].max() > COND_REL * max(1.0, float(np.median(np.abs(r64[ok])))):
                self.reasons.append(f"{what}: tol {tol[ok].max():.3g} above {COND_REL} * max(1, median |ref| = "
                                    f"{np.median(np.abs(r64[ok])):.3g}) (f32 floor {floor:.3g})")
        self.kept = not self.reasons


def misses(got, ref, tol, factor=1.0):
    """bool per entry: `got` is not within factor * tol of the float64 `ref` — infinite reference entries must match exactly, a
    NaN is allowed only where the reference is NaN (there anything is: the reference has no truth)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        bad = np.where(np.isinf(ref), got != ref, ~(np.abs(got - ref) <= factor * tol))
    return bad & ~np.isnan(ref)


def check64(got, source=None, latents=None, observed=None, args=None, what="ll", ref=None, context=""):
    """`got` (lp, ll [n] or the pointwise terms [D, n] of the code under test) against the float64 evaluation of `source`
    (`ref`: a Reference of the same case, shared among the quantities).  -> the largest err / tol over the finite entries."""
    ref = Reference(source, latents, observed, args) if ref is None else ref
    r, tol = ref.ref[what], ref.tol[what]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == r.shape, (what, got.shape, r.shape)
    bad = misses(got, r, tol)
    fin = np.isfinite(r) & np.isfinite(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(fin, np.abs(got - r) / tol, 0.0)
    if bad.any():
        k = np.unravel_index(int(np.argmax(np.where(bad, np.where(fin, ratio, np.inf), -1.0))), r.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries miss the float64 reference; at {k}: got {got[k]!r}, "
                             f"reference {r[k]!r}, tol {tol[k]:.3g} (f32 floor {ref.floor[what]:.3g})\n{context}")
    return float(ratio.max()) if ratio.size else 0.0


# ---- the law of every replicated draw (include/gjx_predictive.h) -------------------------------------------------------------
LAW_MIN_SHARE = 0.9         # of a site's (live particle, row) entries must have a float64 law to be compared with
LAW_MIN_DRAWS = 16384       # below this many draws per site the DKW bound (0.021 there) is too loose to mean anything


def _law_domain(kind, a):
    """bool [n, D]: the float64 arguments are finite and inside the domain on which the law below is defined (a flip with p of
    exactly 0 or 1 has no standardised residual)."""
    with np.errstate(invalid="ignore"):
        fin = np.all([np.isfinite(v) for v in a], axis=0)
        if kind == "normal":
            return fin & (a[1] > 0)
        if kind in ("gamma", "beta"):
            return fin & (a[0] > 0) & (a[1] > 0)
        return fin & (a[0] > 0) & (a[0] < 1)


def law_coverage(source, latents, observed, args, ev=None):
    """-> ({plated address: (kind, float64 arguments [n, D], bool [n, D] entries with a truth)}, live bool [n], reasons): an
    entry has a truth when its particle lies inside the support of every latent (`inside`) and the site's float64 arguments,
    from the source text, are finite and in their domain.  `reasons` names every site with a truth on less than
    LAW_MIN_SHARE of its live entries: such a case leaves a generator's stream (as Reference.reasons does for the densities)."""
    ev = evaluate64(source, latents, observed, args) if ev is None else ev
    live = inside([(k, "latent", v) for k, v in ev.kinds.items()], latents)
    out, reasons = {}, []
    for addr, (kind, a) in ev.laws.items():
        ok = _law_domain(kind, a) & live[:, None]
        share = ok.sum() / max(1, live.sum() * ok.shape[1])
        if share < LAW_MIN_SHARE:
            reasons.append(f"law of {addr!r} ({kind}): arguments in their domain on {share:.2f} of the live entries")
        out[addr] = (kind, a, ok)
    return out, live, reasons


def predictive_laws(source, latents, observed, args, draws):
    """`draws` {plated address: f32 [n, D]}, y_rep[d, i] as [i, d] — of the replay or of the kernel — against the law the
    body's SOURCE TEXT gives that address at (particle i, row d): -> samples for ssm_fuzz.check_laws, whose bounds are derived
    (DKW at alpha = 1e-6 for a PIT, 5 standard errors for a summed residual).  Per kind:
      Normal, Gamma  the probability-integral transform of each draw under its own float64 parameters (ssm_fuzz._law);
      Beta           the PIT through scipy.special.betainc where scipy is importable (exchanged shapes a ~ b move the mean
                     residual by nothing, the PIT by much), otherwise ssm_fuzz._law's standardised residual;
      flip           the standardised residual r = (y - p) / sqrt(p (1 - p)).
    A marginal law is blind to an error that averages to nothing over the case (a probability or a location read from the wrong
    column of symmetric data; exchanged arguments a ~ b).  So every site is also held CONDITIONALLY: with r the standardised
    residual (of a PIT u: sqrt(12) (u - 1/2), mean 0 and variance 1 under the law) and w a covariate centred and scaled to unit
    mean square over the compared entries, sum r_i w_i / sqrt(N) is as standard as sum r_i / sqrt(N), whatever w is as long as
    it is fixed before the draw — the same 5 standard errors bound it.  Covariates, under the key (address, name): the site's
    own float64 arguments ("arg0", "arg1"; a flip's as its logit), every latent column ("latent", address), every data
    argument of the body ("data", position) and every observed float column ("observed", address).
    Entries without a truth (law_coverage) are left out; at least LAW_MIN_SHARE of a site's live entries must remain."""
    import ssm_fuzz as S

    cover, _, reasons = law_coverage(source, latents, observed, args)
    assert not reasons, reasons
    try:
        from scipy.special import betainc
    except ImportError:  # pragma: no cover - the CPU tests of this repository import scipy
        betainc = None
    n = len(next(iter(latents.values())))
    wide = [(("latent", k), np.asarray(v, dtype=np.float64).reshape(n, 1)) for k, v in latents.items()]
    wide += [(("data", k), np.asarray(v, dtype=np.float64).reshape(1, -1)) for k, v in enumerate(args) if np.ndim(v) == 1]
    wide += [(("observed", k), np.asarray(v, dtype=np.float64).reshape(1, -1)) for k, v in observed.items()
             if np.ndim(v) == 1 and np.asarray(v).dtype != bool]
    out = {}
    for addr, y in draws.items():
        kind, a64, ok = cover[addr]
        y = np.asarray(y, dtype=np.float32).astype(np.float64)
        assert y.shape == ok.shape, (addr, y.shape, ok.shape)
        x, a = torch.from_numpy(y[ok]), [torch.from_numpy(np.ascontiguousarray(v[ok])) for v in a64]
        nan = np.where(np.isnan(x.numpy()), np.nan, 0.0)  # (a NaN draw where a truth exists fails check_laws)
        if kind == "beta" and betainc is not None:
            law, v = "pit", betainc(a[0].numpy(), a[1].numpy(), np.clip(x.numpy(), 0.0, 1.0))
        else:
            law, v = S._law(kind, a, x)
            v = v.numpy()
        out[addr] = (law, v + nan)
        r = (math.sqrt(12.0) * (v - 0.5) if law == "pit" else v) + nan
        with np.errstate(invalid="ignore", divide="ignore"):
            own = [np.log(a64[0]) - np.log1p(-a64[0])] if kind == "flip" else list(a64)
            covs = [((f"arg{k}",), np.broadcast_to(w, ok.shape)[ok]) for k, w in enumerate(own)]
        covs += [(name, np.broadcast_to(w, ok.shape)[ok]) for name, w in wide if name != ("observed", addr)]
        for name, w in covs:
            w = w - w.mean()
            ms = float(np.mean(w * w))
            if np.isfinite(ms) and ms > 1e-24 * max(1.0, float(np.max(np.abs(w))) ** 2):
                out[(addr,) + name] = ("z", r * w / math.sqrt(ms))
    return out


def check_predictive(source, latents, observed, args, draws, context=""):
    """predictive_laws through ssm_fuzz.check_laws -> its worst ratios."""
    import ssm_fuzz as S

    return S.check_laws(predictive_laws(source, latents, observed, args, draws), context)


def draws_by_address(addrs, y):
    """Draws [S, n, D] in table order (the kernel's layout; the replay's y [S, D, n] transposed) -> {address: [n, D]}."""
    assert len(addrs) == len(y)
    return {a: np.asarray(y[s]) for s, a in enumerate(addrs)}


# ---- the predictive cases of tests/test_predictive_fuzz_cpu.py and tests/test_gpu_predictive_fuzz.py --------------------------
# ONE definition of the seeds, sizes, inputs and populations: the CPU suite proves them admissible on the replay (the laws hold,
# the coverage is there), the GPU suite compares the kernel on the very same numbers.  Keys: genjax.random.key(PRED_KEY + ., impl).
PRED_DS = (1, 2, 3, 127, 129, 513)   # a lone row, a pair, an odd tail behind a pair, both sides of a wave's 128 rows, one past a tile
PRED_NS = (1, 5, 257)
PRED_BIG = (1000, 129)               # W = 4 chunks
PRED_OUTSIDE = (257, 65)
PRED_API = (300, 65, 33)             # n, the fitted rows, the held-out rows
PRED_SEEDS = (41, 42, 43, 44)
PRED_PER_SEED = 25                   # generated bodies per seed on the CPU; the GPU suite takes the first kept ones of each stream
PRED_RANDOM = (257, (65, 2))         # n and the two row counts of a random body: 257 * 65 = 16705 >= LAW_MIN_DRAWS
PRED_KEY = 5100


def interleaved_inputs():
    """(args, observed) of INTERLEAVED over max(PRED_DS) rows; a case of D rows reads the first D."""
    return random_inputs(np.random.default_rng(77), INTERLEAVED_SITES, max(PRED_DS))


def heldout_inputs():
    """(args, observed) of INTERLEAVED over PRED_API[2] OTHER rows."""
    return random_inputs(np.random.default_rng(78), INTERLEAVED_SITES, PRED_API[2])


def head_rows(args, obs, D):
    """The first D rows of a case's columns."""
    cut = lambda v: v[:D] if isinstance(v, np.ndarray) else v  # noqa: E731
    return tuple(cut(a) for a in args), {k: cut(v) for k, v in obs.items()}


def interleaved_latents(what, n):
    """The population of one interleaved case: `what` a row count of the grid, "big", "outside", "api"."""
    seed = 3100 + what if isinstance(what, int) else {"big": 3001, "outside": 3002, "api": 3003}[what]
    return latent_columns(np.random.default_rng(seed), INTERLEAVED_SITES, n, outside=what == "outside")


def predictive_stream(seed, count=PRED_PER_SEED):
    """The first `count` bodies of a seed's stream: (index, source, sites, args, observed, latents, reasons) — inputs of
    max(PRED_RANDOM[1]) rows, a population of PRED_RANDOM[0].  `reasons`, from the reference alone: empty for a body the
    predictive suites compare, else why not ("no plated site", or law_coverage's at the larger row count)."""
    n, (D, _) = PRED_RANDOM
    rng = np.random.default_rng(seed)
    for i in range(count):
        src, sites = random_tempered_model(rng)
        args, obs = random_inputs(rng, sites, D)
        latents = latent_columns(rng, sites, n)
        if not any(role == "plated" for _, role, _ in sites):
            reasons = ["no plated site"]
        else:
            reasons = law_coverage(src, latents, obs, args)[2]
        yield i, src, sites, args, obs, latents, reasons


# ---- the project's side of a case (the only part that imports the package) ------------------------------------------------
def target_of(source, args, observed, device=None):
    """The body as a `@gen` function over torch tensors of the same f32 values -> genjax.Target."""
    from genjax import ChoiceMap, Target, beta, flip, gamma, gen, normal

    ns = {"normal": normal, "gamma": gamma, "beta": beta, "flip": flip, "torch": torch}
    exec(source, ns)  # noqa: S102 - generated by random_tempered_model above
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(device or "cpu") if isinstance(v, np.ndarray) else v  # noqa: E731
    return Target(gen(ns["model"]), tuple(t(a) for a in args), ChoiceMap.d({k: t(v) for k, v in observed.items()}))


def data_of(tracer, D=None):
    """The tracer's data columns as f32 numpy (the first D rows: every column is elementwise in the arguments' rows)."""
    return [t.detach().to(torch.float32).cpu().numpy().copy()[:D] for t in tracer.data]


def columns_of(tracer, latents):
    """The latent columns in the plan's latent order."""
    return [latents[m["addr"]] for m in tracer.meta if m["obs"] is None]
