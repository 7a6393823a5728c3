"""The references the grouped check kernels (include/gjx_group_checks.h; TemperedSMC.pointwise / .loo / .predictive on a plan
with grouped latents) are held to.

1. The TERMS t[d, i]: group_ref.Assess' single-site oracle plans of the PLATED sites, flat and group-reading alike, one oracle
   run per data row with the scalars and the row's group values z[s][g(d)] as input columns; numpy adds the sites' f32 terms
   in table order.  The reductions are pointwise_ref's and psis_ref's, unchanged.
2. The predictive REPLAY: predictive_ref.Replay's shadow table with one more per-row input column per grouped site, which
   holds z[ref][g(d), i].
3. The CLOSED FORM of group_ref.Intercepts for the per-row predictive densities, and the spread of a float64 numpy population
   around it.
4. The generated sources of FLAT plans, by sha256 (tests/golden/flat_temper_sources.json was recorded before the grouped
   check kernels existed)."""

import hashlib
import json
import math
import os

import numpy as np
import torch

import group_ref as GR
import plate_ref as P
import pointwise_ref as W
import predictive_ref as PR
from genjax._amd import abi, temper
from genjax._amd.runtime import use_ops

HERE = os.path.dirname(os.path.abspath(__file__))
FLAT_GOLDEN = os.path.join(HERE, "golden", "flat_temper_sources.json")


# ---- 4. flat sources ---------------------------------------------------------------------------------------------------------------
def counts_target(D=20):
    """A plated Poisson regression next to a plated Normal site: the counts creator's plan."""
    from genjax import ChoiceMap, Target, gen, normal, poisson

    @gen
    def counts(xs):
        w = normal(0.0, 1.0) @ "w"
        b = normal(0.0, 1.0) @ "b"
        poisson(log_rate=w * xs + b) @ "k"
        normal(w + b * xs, 0.8) @ "y"

    rng = np.random.default_rng(77)
    xs = torch.from_numpy(rng.uniform(-1.0, 1.0, D).astype(np.float32))
    k = torch.from_numpy(rng.poisson(2.0, D).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal(D).astype(np.float32))
    return Target(counts, (xs,), ChoiceMap.d({"k": k, "y": y}))


def flat_plans(ops):
    """name -> TemperPlan of plate_ref's four models and the counts model, lowered from 20 rows."""
    out = {}
    with use_ops(ops):
        for name in P.MODELS + ("counts",):
            tr = temper.lower(counts_target() if name == "counts" else P.target(name, 20)[0], 64)
            out[name] = ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
    return out


def flat_source_hashes(ops):
    """"<model>/<kernel>[/<impl>]" -> sha256 of the generated source, for the five kernel kinds of a flat tempered plan."""
    h = lambda s: hashlib.sha256(s.encode()).hexdigest()
    out = {}
    for name, plan in flat_plans(ops).items():
        out[f"{name}/pointwise"] = h(plan.pointwise_source())
        out[f"{name}/psis"] = h(plan.psis_source())
        for impl in (0, 1):
            out[f"{name}/move/{impl}"] = h(plan.source(impl))
            out[f"{name}/cov/{impl}"] = h(plan.cov_source(impl))
            out[f"{name}/predictive/{impl}"] = h(plan.predictive_source(impl))
    return out


def flat_golden():
    with open(FLAT_GOLDEN) as f:
        return json.load(f)


# ---- layouts and populations ---------------------------------------------------------------------------------------------------------
# group_ref.LAYOUTS (D = 9 .. 52) and one WIDE layout, D = 401: a group spans the 256-row tile boundary of the pointwise
# kernel (rows 131 .. 257) and several wave boundaries; a one-row group, an empty first group and an empty middle group.
WIDE = [0, 130, 1, 127, 3, 0, 140]
LAYOUTS = dict(GR.LAYOUTS)
LAYOUTS[7] = WIDE
ROWS = {G: int(sum(sizes)) for G, sizes in LAYOUTS.items()}  # 1: 9, 2: 9, 5: 13, 17: 52, 7: 401


def group_of_rows(off, D):
    """g(d) of the header for d = 0 .. D-1: the number of g' in 1 .. G-1 with off[g'] <= d."""
    off = np.asarray(off, dtype=np.int64)
    return np.searchsorted(off[1:len(off) - 1], np.arange(D), side="right").astype(np.int64)


def generating(name, sizes, seed=0):
    """The values group_ref.target generates its data from — its generator, replayed: (scalars, grouped [G] each)."""
    G, D = len(sizes), int(sum(sizes))
    rng = np.random.default_rng(100 * seed + 7 * G + D)
    rng.uniform(-1.0, 1.0, D)
    a = 0.4 + 0.7 * rng.standard_normal(G)
    if name == "gamma":
        return [0.7], [rng.gamma(2.0, 0.5, G)]
    if name == "slope":
        return [0.4, 0.6], [a, np.full(G, 0.6)]
    return [0.4, 0.6], [a]


def centred_columns(name, sizes, n, rng, seed=0, width=0.1):
    """Populations a tenth of a unit wide around the generating values (the Gamma component log-normal around its own):
    (x: L float32 [n], z: S float32 [G, n]).  A row's terms then spread a few nats, far below pointwise_ref.LSE_MAX_SPREAD."""
    xs, zs = generating(name, sizes, seed)
    x = [(c + width * rng.standard_normal(n)).astype(np.float32) for c in xs]
    z = [(c[:, None] + width * rng.standard_normal((len(sizes), n))).astype(np.float32) for c in zs]
    if name == "gamma":
        z[0] = (zs[0][:, None] * np.exp(width * rng.standard_normal((len(sizes), n)))).astype(np.float32)
    return x, z


# ---- 1. the terms ----------------------------------------------------------------------------------------------------------------------
def terms(assess, x, z):
    """t[d, i], float32 [D, n]: per row the f32 sum, in table order, of the plated sites' terms (group_ref.Assess' `plated`
    and `reader` plans through its _row), the group-reading ones at the row's group values z[s][g(d)]."""
    n, D = len(x[0]), len(assess.data[0])
    g = group_of_rows(assess.off, D)
    out = np.empty((D, n), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            ins = assess._ins(x, [c[g[d]] for c in z])
            t = None
            for kind, plan, _ in assess.terms:
                if kind not in ("plated", "reader"):
                    continue
                v = assess._row(plan, d, ins, n)
                t = v if t is None else (t + v).astype(np.float32)
            assert t is not None
            out[d] = t
    return out


def terms_many(assess, pops):
    """terms() of several populations [(x, z), ...] in ONE pass over the rows (a term depends on its own particle alone, so
    the populations travel side by side): a list of float32 [D, n_k]."""
    x = [np.concatenate([p[0][l] for p in pops]) for l in range(len(pops[0][0]))]
    z = [np.concatenate([p[1][s] for p in pops], axis=1) for s in range(len(pops[0][1]))]
    t = terms(assess, x, z)
    cuts = np.cumsum([len(p[0][0]) for p in pops])[:-1]
    return [np.ascontiguousarray(v) for v in np.split(t, cuts, axis=1)]


# ---- 2. the predictive replay ------------------------------------------------------------------------------------------------------------
def _input_arg(a, lat, n_data, L, keep):
    """predictive_ref._input_arg with one more rule: a GROUP operand reads input column n_data + L + ref."""
    if a.kind == abi.ARG_GROUP:
        return abi.Arg(abi.ARG_INPUT, n_data + L + a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_EXPR:
        ops = (abi.ExprOp * a.ref).from_address(a.table)
        prog = [((abi.EXPR_INPUT, n_data + lat[o.ref], o.value) if o.op == abi.EXPR_SITE else
                 (abi.EXPR_INPUT, o.ref, o.value) if o.op == abi.EXPR_DATA else
                 (abi.EXPR_INPUT, n_data + L + o.ref, o.value) if o.op == abi.EXPR_GROUP else (o.op, o.ref, o.value)) for o in ops]
        return abi.expr_arg(prog, keep)
    return PR._input_arg(a, lat, n_data, keep)


class Replay(PR.Replay):
    """predictive_ref.Replay over a lowered GROUPED model: the shadow table's plated sites read, per data row, the data
    columns (inputs 0 .. C-1), the particle's scalars (C .. C+L-1) and the row's group values z[ref][g(d), i] (C+L+ref)."""

    def __init__(self, oracle_ops, tracer, data, offsets, impl):
        self.ops, self.impl, self.keep = oracle_ops, impl, []
        self.data = [np.ascontiguousarray(c, dtype=np.float32) for c in data]
        self.D, C = len(self.data[0]), len(self.data)
        self.g = group_of_rows(offsets, self.D)
        lat = GR._latent_index(tracer)
        self.L = L = len(lat)
        sites, self.obs_col, self.is_int, self.addrs = [], [], [], []
        for q, s in enumerate(tracer.sites):
            if s.observed != abi.SITE_PLATED:
                continue
            assert s.obs.kind == abi.ARG_DATA and s.obs.scale == 1.0 and s.obs.offset == 0.0
            c = abi.Site.from_buffer_copy(s)
            c.arg[0], c.arg[1] = _input_arg(s.arg[0], lat, C, L, self.keep), _input_arg(s.arg[1], lat, C, L, self.keep)
            c.observed, c.out_col = 0, len(sites)
            c.obs = abi.Arg(abi.ARG_CONST, 0, 0.0, 0.0, None)
            sites.append(c)
            self.obs_col.append(s.obs.ref)
            self.is_int.append(s.dist == abi.DIST_BERNOULLI)
            self.addrs.append(tracer.meta[q]["addr"])
        self.S, self.sites = len(sites), sites
        self.plan = oracle_ops.plan_create(sites)
        if tracer.params:
            self.plan.set_params(tracer.params)
        self._ins = [torch.from_numpy(c) for c in self.data]
        self._dtypes = [torch.int32 if i else torch.float32 for i in self.is_int]

    def draws(self, key, cols, z):
        """y[s][d, i]: float32 [S, D, n] over the scalar columns `cols` ([n] each) and the grouped columns `z` ([G, n] each)."""
        cols = [np.ascontiguousarray(c, dtype=np.float32) for c in cols]
        z = [np.ascontiguousarray(c, dtype=np.float32) for c in z]
        assert len(cols) == self.L
        n = len(cols[0])
        out = np.empty((self.S, self.D, n), dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(n):
                ins = self._ins + [torch.full((self.D,), float(np.float32(c[i])), dtype=torch.float32) for c in cols]
                ins = ins + [torch.from_numpy(np.ascontiguousarray(c[self.g, i])) for c in z]
                vals = self.ops.importance_run(self.plan, self.key_batch(key, i), self.D, ins, self._dtypes, want_score=False,
                                               want_max_partials=False)[0]
                out[:, :, i] = np.stack([v.numpy().astype(np.float32) for v in vals])
        return out


# ---- 3. the closed form and the recorded spreads ----------------------------------------------------------------------------------------
# Four times these is what tests/test_gpu_group_checks.py allows end to end on group_ref.e2e_model() (D = 200, G = 8): the
# root-mean-square error, bias included, over the 24 seeds E2E_SEEDS of the FINAL population of group_ref.tempered_f64 at
# n = 8192 (K = 2, ESS target 0.5) against the closed form — float64 numpy on the CPU with numpy's generator, not the code
# under test (e2e_errors below; profiles/group_checks_summary.md has the per-seed ranges):
#   lppd      sum_d lppd_d against sum_d log N(y_d; E[a_g + b x_d], 0.5^2 + Var[a_g + b x_d])
#   held      the same sum over the held-out rows of held_out_rows() under the same populations
#   loo       sum_d elpd_loo_d of the numpy PSIS (psis_ref.psis on the f32-rounded terms, the package's tail length) against
#             the closed-form leave-one-out sum (the Gaussian conditional of y_d given the other rows)
#   mean, var, pit   predictive_ref.errors_of's three statistics of replicated data y_rep = a_g + b x_d + 0.5 eps
E2E_SEEDS = tuple(GR.E2E_SEEDS)
E2E_FACTOR = 4.0
E2E_N = 8192
# Measured (42 s for the 24 populations); closed-form sums: lppd -144.5610, held-out (120 rows) -82.7247, leave-one-out -153.5750.
#   lppd   0.00908  (errors between -0.0179 and +0.0107, mean -0.0029)
#   held   0.0383   (errors between -0.0757 and +0.0981, mean +0.0066)
#   loo    0.0584   (errors between -0.1029 and +0.0968, mean -0.0304)
#   mean   0.0324   (per seed between 0.0266 and 0.0456)
#   var    0.0457   (per seed between 0.0317 and 0.0604)
#   pit    0.0435   (per seed between 0.0404 and 0.0486: the 200 observed rows are ONE data set, so most of the distance is theirs)
# The largest khat over those populations and rows is 0.334 (per seed between 0.219 and 0.334), below the threshold
# min(1 - 1 / log10(8192), 0.7) = 0.7: the end-to-end condition n_high == 0 holds on the reference.
SPREAD_LPPD_SUM = 0.00908
SPREAD_HELD_SUM = 0.0383
SPREAD_ELPD_SUM = 0.0584
SPREAD_MEAN = 0.0324
SPREAD_VAR = 0.0457
SPREAD_PIT = 0.0435
E2E_MAX_KHAT = 0.334
# The rows of e2e_errors for the first two seeds (5000, 5001), as measured: lppd, held, loo, mean, var, pit, largest khat.
# tests/test_group_checks_cpu.py repeats these two populations and compares digit for digit (float64 numpy: 1e-5).
E2E_FIRST_SEEDS = ((0.004448, 0.015487, -0.047183, 0.027256, 0.046814, 0.041260, 0.269629),
                   (0.006906, -0.041488, -0.095324, 0.033232, 0.042377, 0.042520, 0.301284))
# Per statistic the smallest and largest of the 24 per-seed values (the RMS lies between the smallest and largest magnitude).
E2E_RANGE = ((-0.0179, 0.0107), (-0.0757, 0.0981), (-0.1029, 0.0968), (0.0266, 0.0456), (0.0317, 0.0604), (0.0404, 0.0486), (0.219, 0.334))


def held_out_rows(m: GR.Intercepts, D=120, seed=1):
    """Other rows of the e2e model's process, same G: (xs f32, g int64 sorted, ys f32).  The generating intercepts are those
    of group_ref.e2e_model(seed=0), replayed from its generator."""
    rng0 = np.random.default_rng(0)
    rng0.integers(0, m.G, m.D)
    rng0.uniform(-1.0, 1.0, m.D)
    a = 0.4 + 0.7 * rng0.standard_normal(m.G)
    rng = np.random.default_rng([seed, 77])
    g = np.sort(rng.integers(0, m.G, D))
    xs = rng.uniform(-1.0, 1.0, D).astype(np.float32)
    ys = (a[g] + 0.6 * xs + 0.5 * rng.standard_normal(D)).astype(np.float32)
    return xs, g.astype(np.int64), ys


def closed_form(m: GR.Intercepts, xs=None, g=None):
    """(mean_d, V_d) of y at the rows (xs, g) — the model's own when None — under the posterior of theta = (mu, b, a):
    E[a_g + b x_d] and noise^2 + Var[a_g + b x_d]; float64 [D] each."""
    xs = m.xs if xs is None else np.asarray(xs, dtype=np.float64)
    g = m.g if g is None else np.asarray(g)
    H = np.zeros((len(xs), 2 + m.G))
    H[:, 1] = xs
    H[np.arange(len(xs)), 2 + g] = 1.0
    return H @ m.post_mean, m.noise ** 2 + np.einsum("di,ij,dj->d", H, m.post_cov, H)


def closed_form_lppd(m, xs=None, g=None, ys=None):
    mean, V = closed_form(m, xs, g)
    r = (m.ys if ys is None else np.asarray(ys, dtype=np.float64)) - mean
    return -0.5 * (np.log(2 * np.pi * V) + r * r / V)


def closed_form_loo(m: GR.Intercepts):
    """float64 [D]: log p(y_d | y_-d).  y ~ N(0, C) with C = noise^2 I + H cov H'; with Q = C^-1 the conditional of y_d given
    the rest is N(y_d - (Q y)_d / Q_dd, 1 / Q_dd)."""
    M = np.zeros((2 + m.G, 2 + m.G))
    M[0, 0], M[1, 1] = m.s_mu, m.s_b
    M[2:, 0], M[2:, 2:] = m.s_mu, m.tau * np.eye(m.G)
    H = np.zeros((m.D, 2 + m.G))
    H[:, 1] = m.xs
    H[np.arange(m.D), 2 + m.g] = 1.0
    Q = np.linalg.inv(m.noise ** 2 * np.eye(m.D) + H @ (M @ M.T) @ H.T)
    V = 1.0 / np.diag(Q)
    r = (Q @ m.ys) * V  # y_d - E[y_d | y_-d]
    return -0.5 * (np.log(2 * np.pi * V) + r * r / V)


def terms_f64(m: GR.Intercepts, b, a, xs=None, g=None, ys=None):
    """The model's row log-densities in float64 numpy at a population (b [n], a [G, n]): [D, n]."""
    xs = m.xs if xs is None else np.asarray(xs, dtype=np.float64)
    g = m.g if g is None else np.asarray(g)
    ys = m.ys if ys is None else np.asarray(ys, dtype=np.float64)
    r = ys[:, None] - (np.asarray(a, dtype=np.float64)[g] + np.asarray(b, dtype=np.float64)[None, :] * xs[:, None])
    return -0.5 * (r / m.noise) ** 2 - (0.5 * math.log(2 * math.pi) + math.log(m.noise))


def e2e_errors(m: GR.Intercepts, n, seeds, loo=True):
    """Per seed: (lppd-sum error, held-out lppd-sum error, elpd_loo-sum error (NaN without `loo`), mean, var, pit errors,
    the largest khat) of the final population of group_ref.tempered_f64 — float64 [len(seeds), 7]."""
    import psis_ref as S

    class _Rows:  # (what predictive_ref.errors_of reads of a model)
        pass

    hx, hg, hy = held_out_rows(m)
    exact, exact_held, exact_loo = closed_form_lppd(m).sum(), closed_form_lppd(m, hx, hg, hy).sum(), closed_form_loo(m).sum()
    mu, V = closed_form(m)
    out = []
    for s in seeds:
        r = GR.tempered_f64(m, n, 2, 0.5, np.random.default_rng(s))
        b, a = r["b"].astype(np.float32), r["a"].astype(np.float32)
        t = terms_f64(m, b, a)
        e_lppd = (W.reduce64(t)[0] - math.log(n)).sum() - exact
        e_held = (W.reduce64(terms_f64(m, b, a, hx, hg, hy))[0] - math.log(n)).sum() - exact_held
        e_loo, kmax = math.nan, math.nan
        if loo:
            ps = S.psis(t.astype(np.float32), S.tail_len(n))
            e_loo, kmax = ps["elpd"].sum() - exact_loo, ps["khat"].max()
        rng = np.random.default_rng([s, 1])
        y = a.astype(np.float64)[m.g] + b.astype(np.float64)[None, :] * m.xs[:, None] + m.noise * rng.standard_normal((m.D, n))
        below, equal = (y < m.ys[:, None]).sum(axis=1), (y == m.ys[:, None]).sum(axis=1)
        mean, var, pit = y.mean(axis=1), y.var(axis=1, ddof=1), (below + 0.5 * equal) / n
        out.append((e_lppd, e_held, e_loo, float(np.max(np.abs(mean - mu) / np.sqrt(V))), float(np.max(np.abs(var / V - 1.0))),
                    PR.kolmogorov_uniform(pit), kmax))
    return np.asarray(out)


def spreads(errors):
    """The root-mean-square over the seeds of the first six columns of e2e_errors."""
    return np.sqrt(np.mean(np.asarray(errors)[:, :6] ** 2, axis=0))
