"""The references the predictive kernels (include/gjx_predictive.h, genjax/_amd/temper.py TemperedSMC.predictive) are held to.

1. The REPLAY of the header's definition from UNCHANGED oracle entry points (the oracle knows no gjx_predictive.h): the SHADOW
   TABLE of a lowered plated model — its plated sites alone, as latent sites, DATA operands read from per-particle input
   columns 0 .. C-1, references to latent l from input column C + l — and one oracle `importance_run` per particle i over the D
   data rows under split_lazy(fold_in(key, i), D), the latent columns constant at x_l[i].  Data and latents travel as INPUT
   COLUMNS: nothing goes through host-hoisted parameters (plate_ref reads data from launch parameters; here the rows are the
   oracle's particles, so the oracle evaluates every argument per row in f32 itself).
2. The SUMMARIES of those draws in float64 numpy, with the bounds pointwise_ref.moment_bounds gives a float64 sum in any order.
3. The closed form of the conjugate regression (plate_ref.conjugate): with (w, b) ~ N(mu, Sigma) the posterior, replicated
   data at row d are N(x_d' mu, noise^2 + x_d' Sigma x_d), and the PIT values of the observed rows are uniform."""

import math

import numpy as np
import torch

import pointwise_ref as W
import temper_ref as R
from genjax._amd import abi, prng

# Four times these is what tests/test_gpu_predictive.py::test_closed_form and tests/test_predictive_cpu.py allow: the
# root-mean-square over 24 seeds (CLOSED_FORM_SEEDS) of the three errors of closed_form_errors below on
# plate_ref.conjugate(500) at n = 8192 — populations from the exact posterior (pointwise_ref.posterior_columns) and replicated
# data y_rep[d, i] = w_i x_d + b_i + noise * eps with numpy's generator, float64 numpy throughout, not the code under test
# (profiles/predictive_summary.md; 3 s for the 24 populations; spreads(plate_ref.conjugate(500), 8192, CLOSED_FORM_SEEDS)):
#   mean   max over the 500 rows of |mean_d - x_d' mu| / sd_d, sd_d the closed-form predictive deviation:   0.0348
#          (per seed between 0.0301 and 0.0426)
#   var    max over the rows of |var_d / V_d - 1|, V_d the closed-form predictive variance:                   0.0513
#          (per seed between 0.0447 and 0.0668)
#   pit    the Kolmogorov distance of the 500 values (below_d + 0.5 equal_d) / n from the uniform distribution: 0.0281
#          (per seed between 0.0260 and 0.0296: the 500 observed rows are ONE data set, so most of the distance is theirs)
SPREAD_MEAN = 0.0348
SPREAD_VAR = 0.0513
SPREAD_PIT = 0.0281
CLOSED_FORM_FACTOR = 4.0
CLOSED_FORM_SEEDS = tuple(range(8000, 8024))
FIELDS = ("s1", "s2", "below", "equal", "nan")


# ---- 1. the replay ---------------------------------------------------------------------------------------------------------
def _input_arg(a, lat, n_data, keep):
    """An operand of a plated site in the shadow table (in the manner of plate_ref._param_arg): DATA column c -> input
    column c, a reference to latent l -> input column n_data + l; literals and parameters as they are."""
    if a.kind == abi.ARG_DATA:
        return abi.Arg(abi.ARG_INPUT, a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_SITE:
        return abi.Arg(abi.ARG_INPUT, n_data + lat[a.ref], a.scale, a.offset, None)
    if a.kind == abi.ARG_EXPR:
        ops = (abi.ExprOp * a.ref).from_address(a.table)
        prog = [((abi.EXPR_INPUT, n_data + lat[o.ref], o.value) if o.op == abi.EXPR_SITE else
                 (abi.EXPR_INPUT, o.ref, o.value) if o.op == abi.EXPR_DATA else (o.op, o.ref, o.value)) for o in ops]
        return abi.expr_arg(prog, keep)
    assert a.kind in (abi.ARG_CONST, abi.ARG_PARAM), a.kind
    return abi.Arg(a.kind, a.ref, a.scale, a.offset, a.table)


class Replay:
    """The draws and observed values of a lowered plated model over `data` (float32 numpy columns of one length D, in column
    order) from one oracle importance plan: the shadow table."""

    def __init__(self, oracle_ops, tracer, data, impl):
        self.ops, self.impl, self.keep = oracle_ops, impl, []
        self.data = [np.ascontiguousarray(c, dtype=np.float32) for c in data]
        self.D, C = len(self.data[0]), len(self.data)
        lat = R._latent_index(tracer)
        self.L = len(lat)
        sites, self.obs_col, self.is_int, self.addrs = [], [], [], []
        for q, s in enumerate(tracer.sites):
            if s.observed != abi.SITE_PLATED:
                continue
            assert s.obs.kind == abi.ARG_DATA and s.obs.scale == 1.0 and s.obs.offset == 0.0  # (what the lowering emits)
            c = abi.Site.from_buffer_copy(s)
            c.arg[0], c.arg[1] = _input_arg(s.arg[0], lat, C, self.keep), _input_arg(s.arg[1], lat, C, self.keep)
            c.observed, c.out_col = 0, len(sites)
            c.obs = abi.Arg(abi.ARG_CONST, 0, 0.0, 0.0, None)
            sites.append(c)
            self.obs_col.append(s.obs.ref)
            self.is_int.append(s.dist == abi.DIST_BERNOULLI)
            self.addrs.append(tracer.meta[q]["addr"])
        self.S = len(sites)
        self.sites = sites
        self.plan = oracle_ops.plan_create(sites)
        if tracer.params:
            self.plan.set_params(tracer.params)
        self._ins = [torch.from_numpy(c) for c in self.data]
        self._dtypes = [torch.int32 if i else torch.float32 for i in self.is_int]

    def key_batch(self, key, i):
        return prng.split_lazy(prng.fold_in(key, i), self.D)

    def particle(self, key, i, x):
        """The draws of particle i with latent values x[l]: float32 [S, D] (Bernoulli as 0 / 1)."""
        ins = self._ins + [torch.full((self.D,), float(np.float32(v)), dtype=torch.float32) for v in x]
        vals = self.ops.importance_run(self.plan, self.key_batch(key, i), self.D, ins, self._dtypes, want_score=False,
                                       want_max_partials=False)[0]
        return np.stack([v.numpy().astype(np.float32) for v in vals])

    def draws(self, key, cols):
        """y[s][d, i]: float32 [S, D, n] over the latent columns `cols` (float32 numpy [n] each)."""
        cols = [np.ascontiguousarray(c, dtype=np.float32) for c in cols]
        assert len(cols) == self.L
        n = len(cols[0])
        out = np.empty((self.S, self.D, n), dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(n):
                out[:, :, i] = self.particle(key, i, [c[i] for c in cols])
        return out

    def observed(self):
        """obs[s][d] as gjx_plate.h evaluates it: float32 [S, D] (Bernoulli: rint(value) != 0, as 0 / 1)."""
        out = []
        for c, is_int in zip(self.obs_col, self.is_int):
            v = self.data[c]
            with np.errstate(invalid="ignore"):
                out.append((np.rint(v) != 0).astype(np.float32) if is_int else v.copy())
        return np.stack(out)


# ---- 2. the summaries --------------------------------------------------------------------------------------------------------
def summarize(y, obs):
    """y float32 [S, D, n], obs float32 [S, D] -> float64 [S, 5, D]: s1, s2, below, equal, nan (comparisons false on NaN)."""
    y64 = np.asarray(y, dtype=np.float64)
    o = np.asarray(obs, dtype=np.float32)[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([y64.sum(axis=2), (y64 * y64).sum(axis=2), (y < o).sum(axis=2).astype(np.float64),
                         (y == o).sum(axis=2).astype(np.float64), np.isnan(y).sum(axis=2).astype(np.float64)], axis=1)


def moment_bounds(y):
    """-> (bound of |s1 - ref|, bound of |s2 - ref|), float64 [S, D] each: pointwise_ref.moment_bounds per site."""
    b = [W.moment_bounds(y[s]) for s in range(y.shape[0])]
    return np.stack([x[0] for x in b]), np.stack([x[1] for x in b])


def check(got, y, obs, case):
    """got float64 [S, 5, D] (the kernel's table) against the replay's draws: counts equal, moments within the bounds."""
    ref = summarize(y, obs)
    b1, b2 = moment_bounds(y)
    assert got.shape == ref.shape, case
    for k in (2, 3, 4):
        assert np.array_equal(got[:, k], ref[:, k]), (case, FIELDS[k])
    for k, b in ((0, b1), (1, b2)):
        fin = np.isfinite(ref[:, k])
        assert np.array_equal(np.isnan(got[:, k]), np.isnan(ref[:, k])), (case, FIELDS[k])
        assert np.array_equal(got[:, k][~fin & ~np.isnan(ref[:, k])], ref[:, k][~fin & ~np.isnan(ref[:, k])]), (case, FIELDS[k])
        assert np.all(np.abs(got[:, k] - ref[:, k])[fin] <= b[fin]), (case, FIELDS[k])
    return ref


def same_bits(a, b):
    """float32 arrays equal bit for bit, except that a NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- 3. the closed form ----------------------------------------------------------------------------------------------------
def closed_form(model):
    """(mean_d, V_d) of the replicated data of the conjugate regression: x_d' mu, noise^2 + x_d' Sigma x_d; float64 [D] each."""
    X = np.stack([model.xs, np.ones(model.m)], axis=1)
    return X @ model.post_mean, model.noise ** 2 + np.einsum("di,ij,dj->d", X, model.post_cov, X)


def kolmogorov_uniform(u):
    """sup |F_n(t) - t| of the sample u against the uniform distribution on [0, 1]."""
    u = np.sort(np.asarray(u, dtype=np.float64))
    k = np.arange(1, len(u) + 1)
    return float(max(np.max(k / len(u) - u), np.max(u - (k - 1) / len(u))))


def errors_of(model, n, mean, var, pit):
    """The three errors of a predictive summary (float64 [D] each) against the closed form."""
    mu, V = closed_form(model)
    return (float(np.max(np.abs(mean - mu) / np.sqrt(V))), float(np.max(np.abs(var / V - 1.0))), kolmogorov_uniform(pit))


def replicate_f64(model, cols, rng):
    """y_rep float64 [D, n] of the regression at the (f32) columns: w_i x_d + b_i + noise * eps, numpy's generator."""
    w, b = (np.asarray(c, dtype=np.float64) for c in cols)
    return model.xs[:, None] * w[None, :] + b[None, :] + model.noise * rng.standard_normal((model.m, len(w)))


def closed_form_errors(model, n, seeds):
    """-> float64 [len(seeds), 3]: errors_of a posterior population's replicated data, per seed."""
    out = []
    for s in seeds:
        y = replicate_f64(model, W.posterior_columns(model, n, s), np.random.default_rng([s, 1]))
        below, equal = (y < model.ys[:, None]).sum(axis=1), (y == model.ys[:, None]).sum(axis=1)
        out.append(errors_of(model, n, y.mean(axis=1), y.var(axis=1, ddof=1), (below + 0.5 * equal) / n))
    return np.asarray(out)


def spreads(model, n, seeds):
    """The root-mean-square over the seeds of each of the three errors."""
    return np.sqrt(np.mean(closed_form_errors(model, n, seeds) ** 2, axis=0))
