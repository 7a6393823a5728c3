"""Random and fixed GROUPED tempered bodies against a float64 evaluation of their own source text (include/gjx_group.h).

tests/temper_fuzz.py carried over to plans with grouped latents: `dist(...).repeat(n=G) @ "a"` and `a[g]`, readers of every
plated kind (count sites included), grouped sites of every kind with literal, parameter, affine and PROGRAM arguments.  The
float64 truth is temper_fuzz.evaluate64 — a grouped address's value is an f32 [G, n] column in the same `latents` mapping, so
temper_fuzz.Reference and check64 are used unchanged, with their tolerance.  The replay the kernels are pinned to bit for bit
is tests/group_ref.py's; it is built from the tracer's table, the truth from the source text.  Used by
tests/test_group_fuzz_cpu.py (oracle backend) and tests/test_gpu_group_fuzz.py (HIP backend)."""

import numpy as np
import torch

import group_ref as GR
import temper_fuzz as F
from fuzz_models import _expr, _pos

COUNTS = ("poisson", "negative_binomial")
GAMMA_OUTSIDE = (-0.5, 0.0, np.nan, -1e-30)
BETA_OUTSIDE = (-0.25, 0.0, np.nan, 1.0, 1.5)
MAX_ROW_SITES = 5   # plated sites and readers per random body: their columns (a count site's two) stay below the plan's sixteen

# ---- the fixed body --------------------------------------------------------------------------------------------------------------
GROUPED_INTERLEAVED = '''def model(xs, zs, ps, s, t, g):
    m = normal(0.0, 1.5) @ "m"                                        # a scalar Normal latent
    u = beta(2.0, 3.0).repeat(n=G) @ "u"                              # a grouped BETA, literal arguments, declared BEFORE the next scalar latent
    r = gamma(2.0, 1.5) @ "r"                                         # a scalar Gamma latent: position 2 in the table, latent 1
    ls = normal(0.0, 0.5) @ "ls"                                      # a scalar Normal latent: position 3, latent 2
    a = normal(0.5 * m + 0.2, torch.exp(0.3 * ls)).repeat(n=G) @ "a"  # grouped Normal: an affine location, a PROGRAM as scale
    sg = gamma(1.5 * r + 0.5, 2.0).repeat(n=G) @ "sg"                 # grouped Gamma: its shape reads a scalar latent affinely
    c = normal(t, 0.6).repeat(n=G) @ "c"                              # grouped Normal with a parameter as location: S = 4
    w = normal(m * xs + 0.25, s) @ "w"                                # a flat plated Normal (no grouped value)
    normal(m + 0.5, 0.7) @ "o"                                        # a scalar observed site
    normal(2.0 * a[g] - 0.5, sg[g] + 0.1) @ "y1"                      # both arguments bare affine GROUP operands; the scale reads the Gamma
    gamma(r * 1.5 + 0.2, torch.exp(0.3 * a[g])) @ "y2"                # a Gamma reader: a[g] under a nonlinear function, in its rate
    flip(torch.sigmoid(a[g] + ls * xs)) @ "y3"                        # a flip reader
    beta(u[g] * ps + 0.5, 1.0 + w * w) @ "y4"                         # a Beta reader: the grouped Beta in a shape, an EARLIER PLATE'S VALUE as data
    poisson(log_rate=a[g] + c[g] * xs) @ "y5"                         # a Poisson reader of two grouped sites
    negative_binomial(r + 1.0, logits=0.5 * c[g] - zs) @ "y6"         # a negative-binomial reader with a group-dependent logit
'''
GROUPED_SITES = (("m", "latent", "normal"), ("u", "grouped", "beta"), ("r", "latent", "gamma"), ("ls", "latent", "normal"),
                 ("a", "grouped", "normal"), ("sg", "grouped", "gamma"), ("c", "grouped", "normal"), ("w", "plated", "normal"),
                 ("o", "scalar", "normal"), ("y1", "reader", "normal"), ("y2", "reader", "gamma"), ("y3", "reader", "flip"),
                 ("y4", "reader", "beta"), ("y5", "reader", "poisson"), ("y6", "reader", "negative_binomial"))


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _ok(e, data_names):
    """temper_fuzz._lowers_by_design with `name[g]` read as the traced value it is (a condition over it is traced)."""
    return F._lowers_by_design(e.replace("[g]", ""), data_names)


def _draw(rng, make, data_names, need=None):
    """An expression that lowers by design and (need) contains the leaf `need`; after 20 attempts None."""
    for _ in range(20):
        e = make()
        if _ok(e, data_names) and (need is None or need in e):
            return e
    return None


def random_grouped_model(rng):
    """-> (source of `def model(xs, zs, ps, s, t, g): ...`, sites as (name, role, kind)).  temper_fuzz.random_tempered_model's
    roles ('latent', 'scalar', 'plated') and two more:
      'grouped'  normal / gamma / beta `.repeat(n=G)`, 1 <= S <= 4 per body; its arguments are fuzz_models' expressions over the
                 scalar latents and parameters declared so far — never data, never a grouped value;
      'reader'   a plated site of kind normal / gamma / beta / flip / poisson / negative_binomial whose argument expressions take
                 `name[g]` of every grouped site declared so far as leaves (real for Normal, positive for Gamma, unit-interval for
                 Beta); at least one argument holds such a leaf, and every grouped site is read by at least one reader.
    Every body is supported by construction; the one refusal left is temper_fuzz._lowers_by_design's."""
    lines, sites = [], []
    reals, poss, units = [], [], []          # scalar latents by kind
    g_reals, g_poss, g_units = [], [], []    # `name[g]` leaves by kind
    unread, n_rows = [], 0                   # grouped leaves no reader holds yet; plated sites and readers so far
    d_reals, d_poss = list(F.DATA), ["ps"]
    n_sites = int(rng.integers(4, 9))
    lit = lambda lo, hi: round(float(rng.uniform(lo, hi)), 3)  # noqa: E731
    q = 0
    while q < n_sites or unread:
        name = f"v{q}"
        r = rng.random()
        S = len(g_reals) + len(g_poss) + len(g_units)
        room = n_rows + len(unread) < MAX_ROW_SITES  # (every unread grouped site still gets a reader of its own, at the worst)
        if q == 0:
            role = "latent"
        elif q >= n_sites:
            role = "reader"
        elif q == n_sites - 1 and S == 0:
            role = "grouped"
        elif r < 0.25:
            role = "latent"
        elif r < 0.5 and S < GR.abi.GROUP_MAX_SITES and room:
            role = "grouped"
        elif r < 0.6 or not room:
            role = "scalar" if r < 0.6 else ("reader" if unread else "latent")
        elif r < 0.7 or S == 0:
            role = "plated"
        else:
            role = "reader"
        kind = str(rng.choice({"latent": ["normal", "normal", "gamma", "beta"], "grouped": ["normal", "normal", "gamma", "beta"],
                               "scalar": ["normal", "normal", "gamma", "beta", "flip"], "plated": ["normal", "normal", "gamma", "beta", "flip"],
                               "reader": ["normal", "normal", "gamma", "beta", "flip", "poisson", "negative_binomial"]}[role]))
        pool, ppool, dn, need = reals + poss + units, list(poss), set(), None
        if role in ("plated", "reader"):
            pool, ppool, dn = pool + d_reals, ppool + d_poss, set(d_reals)
        if role == "reader":
            need = str(unread[0] if unread else rng.choice(g_reals + g_poss + g_units))
            # (the leaf the site must read is met three times as often as another)
            pool, ppool = pool + g_reals + g_poss + g_units + [need] * 3, ppool + g_poss + ([need] * 3 if need in g_poss else [])
        e0 = _draw(rng, lambda: _expr(rng, pool, ["t"]), dn) or repr(lit(-1.0, 1.0))
        p0, p1 = (_draw(rng, lambda: _pos(rng, pool, ppool, ["s"]), dn) or repr(lit(0.3, 1.5)) for _ in range(2))
        by_rate = kind == "poisson" and rng.random() < 0.3  # poisson(rate), else poisson(log_rate=...)
        used = {"normal": (e0, p0), "gamma": (p0, p1), "beta": (p0, p1), "flip": (e0,), "poisson": (p0,) if by_rate else (e0,),
                "negative_binomial": (p0, e0)}[kind]
        if need is not None and not any(need in e for e in used):
            # the leaf by a template of the kind: in a location / logit / log-rate, or under exp in a rate / shape
            if kind in ("normal", "flip", "negative_binomial") or (kind == "poisson" and not by_rate):
                e0 = f"({need} * {lit(0.3, 1.5)} + {e0})"
            elif kind == "poisson":
                p0 = f"({p0} + torch.exp({lit(-0.5, 0.5)} * {need}))"
            else:
                p1 = f"({p1} + torch.exp({lit(-0.5, 0.5)} * {need}))"
        traced = bool(F._names(e0)) or "[g]" in e0  # (torch.sigmoid of a Python float is no tensor operation)
        if kind == "normal":
            call = f"normal({e0}, {p0})"
        elif kind in ("gamma", "beta"):
            call = f"{kind}({p0}, {p1})"
        elif kind == "flip":
            if need is not None and need in g_units and rng.random() < 0.3:
                call = f"flip({need})"
            else:
                call = f"flip(torch.sigmoid({e0}))" if traced else f"flip({lit(0.1, 0.9)})"
        elif kind == "poisson":  # (a log-rate is kept moderate: exp of it is a rate)
            call = f"poisson({p0})" if by_rate else f"poisson(log_rate=0.3 * {e0})"
        else:
            call = f"negative_binomial({p0}, torch.sigmoid({e0}))" if traced and rng.random() < 0.4 else f"negative_binomial({p0}, logits={e0})"
        assert need is None or need in call, (need, call)
        lines.append(f"    {name} = {call}{'.repeat(n=G)' if role == 'grouped' else ''} @ '{name}'")
        sites.append((name, role, kind))
        if role == "latent":
            {"normal": reals, "gamma": poss, "beta": units}[kind].append(name)
        elif role == "grouped":
            {"normal": g_reals, "gamma": g_poss, "beta": g_units}[kind].append(f"{name}[g]")
            unread.append(f"{name}[g]")
        elif role in ("plated", "reader"):
            n_rows += 1
            if kind in ("normal", "gamma", "beta"):
                d_reals.append(name)
            if kind == "gamma":
                d_poss.append(name)
        if role == "reader":
            unread = [v for v in unread if v not in call]
        q += 1
    return "def model(xs, zs, ps, s, t, g):\n" + "\n".join(lines) + "\n", sites


# ---- inputs and populations --------------------------------------------------------------------------------------------------------
def random_inputs(rng, sites, sizes, like=None):
    """-> (args (xs, zs, ps, s, t, g), observed {name: value}): temper_fuzz.random_inputs over D = sum(sizes) rows with the int64
    group column of the group sizes `sizes` as the last argument; a count site observes Poisson(2) counts as an f32 column.
    `like` (args, observed): the scalar arguments and scalar observations are taken from that case — the same body over
    another layout with everything a plan's SOURCE may hold (a constant where a parameter cannot be traced) unchanged."""
    g = GR.group_column(sizes)
    flat = [(name, "plated" if role == "reader" else role, kind) for name, role, kind in sites if role != "grouped" and kind not in COUNTS]
    args, obs = F.random_inputs(rng, flat, len(g))
    for name, role, kind in sites:
        if kind in COUNTS:
            obs[name] = rng.poisson(2.0, len(g)).astype(np.float32)
    if like is not None:
        args = args[:3] + like[0][3:5]
        obs.update({k: v for k, v in like[1].items() if np.ndim(v) == 0})
    return args + (g,), obs


def latent_columns(rng, sites, n, G, outside=False, centred=False):
    """{name: f32 [n]} per scalar latent (temper_fuzz.latent_columns) and {name: f32 [G, n]} per grouped site.  `outside`:
    every fourth particle's value of every Gamma / Beta GROUPED site outside its support (negative, zero, NaN, for Beta also 1
    and above; the scalars stay inside) — the same particles in every group, so that three quarters of them stay live;
    `centred`: a tenth of a unit wide around one centre per scalar and per (grouped site, group)."""
    out = F.latent_columns(rng, [s for s in sites if s[1] == "latent"], n, centred=centred)
    for name, role, kind in sites:
        if role != "grouped":
            continue
        if centred:
            c = {"normal": rng.uniform(-0.5, 0.5, (G, 1)), "gamma": rng.uniform(0.6, 1.5, (G, 1)), "beta": rng.uniform(0.3, 0.7, (G, 1))}[kind]
            z = 0.1 * rng.standard_normal((G, n))
            col = c + z if kind == "normal" else (c * np.exp(z) if kind == "gamma" else np.clip(c + 0.3 * z, 0.02, 0.98))
        else:
            col = {"normal": lambda: rng.standard_normal((G, n)), "gamma": lambda: rng.gamma(2.0, 0.5, (G, n)) + 0.01,
                   "beta": lambda: np.clip(rng.beta(2.0, 2.0, (G, n)), 0.01, 0.99)}[kind]()
        col = col.astype(np.float32)
        if outside and kind in ("gamma", "beta"):
            bad = np.asarray(GAMMA_OUTSIDE if kind == "gamma" else BETA_OUTSIDE, dtype=np.float32)
            k = np.arange(col[:, ::4].shape[1])
            for g in range(G):
                col[g, ::4] = bad[(k + g) % len(bad)]
        out[name] = col
    return out


def inside(sites, latents):
    """bool [n]: the particles whose Gamma / Beta latents, scalar and grouped (in every group), lie in their open support."""
    ok = np.ones(np.shape(next(iter(latents.values())))[-1], dtype=bool)
    with np.errstate(invalid="ignore"):
        for name, role, kind in sites:
            if role in ("latent", "grouped") and kind in ("gamma", "beta"):
                v = np.asarray(latents[name]).reshape(-1, len(ok))
                ok &= np.all((v > 0) & ((v < 1) | (kind == "gamma")), axis=0)
    return ok


# ---- the project's side of a case (the only part that imports the package) -----------------------------------------------------
def target_of(source, args, observed, G, device=None):
    """The body as a `@gen` function over torch tensors of the same f32 values, the group column as an int64 tensor, the
    group count G as the body's global -> genjax.Target."""
    from genjax import ChoiceMap, Target, beta, flip, gamma, gen, negative_binomial, normal, poisson

    ns = {"normal": normal, "gamma": gamma, "beta": beta, "flip": flip, "poisson": poisson, "negative_binomial": negative_binomial,
          "torch": torch, "G": int(G)}
    exec(source, ns)  # noqa: S102 - GROUPED_INTERLEAVED or generated by random_grouped_model above
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(device or "cpu") if isinstance(v, np.ndarray) else v  # noqa: E731
    return Target(gen(ns["model"]), tuple(t(a) for a in args), ChoiceMap.d({k: t(v) for k, v in observed.items()}))


def columns_of(tracer, latents):
    """-> (x, z): the scalar columns in the plan's latent order, the grouped [G, n] columns in the grouped sites' order."""
    x = [latents[m["addr"]] for m in tracer.meta if m["obs"] is None and not m.get("grouped")]
    z = [latents[m["addr"]] for m in tracer.meta if m.get("grouped")]
    return x, z


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


# ---- the law of `init`'s draws -----------------------------------------------------------------------------------------------------
def init_laws(source, scalars, observed, args, z):
    """`z` {grouped address: f32 [G, n]} — the draws of `init` at the particles' scalars `scalars` — against the law the body's
    SOURCE TEXT gives each grouped site at the particle's scalars: -> samples for ssm_fuzz.check_laws.  Per site the
    probability-integral transform of every draw under its float64 arguments (Normal, Gamma: ssm_fuzz._law; Beta: scipy's
    betainc where importable, else _law's standardised residual), and — temper_fuzz.predictive_laws' reason: a marginal law is
    blind to an error that averages out — the conditional residuals against the site's own arguments and every scalar latent."""
    import math

    import ssm_fuzz as S

    try:
        from scipy.special import betainc
    except ImportError:  # pragma: no cover
        betainc = None
    ev = F.evaluate64(source, {**scalars, **z}, observed, args)
    out = {}
    for addr, (kind, a64) in ev.group_laws.items():
        y = np.asarray(z[addr], dtype=np.float64).T  # [n, G]
        x, a = torch.from_numpy(np.ascontiguousarray(y)), [torch.from_numpy(np.ascontiguousarray(v)) for v in a64]
        if kind == "beta" and betainc is not None:
            law, v = "pit", betainc(a64[0], a64[1], np.clip(y, 0.0, 1.0))
        else:
            law, v = S._law(kind, a, x)
            v = v.numpy()
        v = v + np.where(np.isnan(y), np.nan, 0.0)
        out[addr] = (law, v.reshape(-1))
        r = math.sqrt(12.0) * (v - 0.5) if law == "pit" else v
        covs = [((f"arg{k}",), w) for k, w in enumerate(a64)]
        covs += [(("latent", k), np.broadcast_to(np.asarray(c, dtype=np.float64)[:, None], y.shape)) for k, c in scalars.items()]
        for name, w in covs:
            w = w - w.mean()
            ms = float(np.mean(w * w))
            if np.isfinite(ms) and ms > 1e-24 * max(1.0, float(np.max(np.abs(w))) ** 2):
                out[(addr,) + name] = ("z", (r * w / math.sqrt(ms)).reshape(-1))
    return out
