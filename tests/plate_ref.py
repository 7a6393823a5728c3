"""The references plated tempered plans (include/gjx_plate.h, genjax/_amd/temper.py) are held to.

1. The REPLAY of the header's addition to `assess` from UNCHANGED oracle entry points (the oracle knows no gjx_plate.h):
   lp as tests/temper_ref.py composes it; per observed site in table order one single-site oracle importance plan whose
   log-weight column is that site's log-density.  A PLATED site's plan reads the row's data values as LAUNCH PARAMETERS
   (DATA column c -> parameter slot P + c, P the model's own parameter count): one oracle run per row gives the f32 terms
   t_d, numpy sums them in float64 in row order, rounds once to f32 and adds to ll in f32.
2. The models both test files use, and a float64 numpy RESTATEMENT of the whole sampler (temper_ref.tempered_f64 with a
   vector likelihood: temper_ref.Regression at m = 500) with the closed-form log Z and posterior."""

import numpy as np
import torch

import temper_ref as R
from genjax._amd import abi, prng

# The end-to-end tolerance (tests/test_gpu_plate.py, tests/test_plate_cpu.py): FOUR TIMES the spread (root-mean-square error, bias included) of the
# float64 restatement restatement_errors (below) over 24 seeds (default_rng(3000 .. 3023)) on the conjugate regression
# with D = 500 at n = 8192, K = 2, ESS target 0.5 — measured on the CPU with numpy's generator, not on the code under test
# (profiles/plate_summary.md): log Z 0.0706; posterior means of (w, b) 0.0148, 0.0154 posterior deviations; posterior
# deviations of (w, b) 0.0112, 0.0095 relative (27 s for the 24 runs).
SPREAD_LOG_Z = 0.0706
SPREAD_MEAN = (0.0148, 0.0154)
SPREAD_SD = (0.0112, 0.0095)
E2E_FACTOR = 4.0
# The same spread for the TWO-PLATE regression (two_plate below; tests/test_gpu_temper_fuzz.py, tests/test_temper_fuzz_cpu.py):
# restatement_errors over the same 24 seeds at n = 4096, K = 2, ESS target 0.5, D = 200 rows per plate (profiles/plate_summary.md):
# log Z 0.1009 (errors between -0.257 and +0.199, mean +0.008; log Z = -17.939); posterior means of (w, b) 0.0214, 0.0181 posterior
# deviations; posterior deviations 0.0166, 0.0156 relative (12 s for the 24 runs).
TWO_PLATE_SPREAD_LOG_Z = 0.1009
TWO_PLATE_SPREAD_MEAN = (0.0214, 0.0181)
TWO_PLATE_SPREAD_SD = (0.0166, 0.0156)


def _param_arg(a, lat, base, keep):
    """An argument of a site with latent references read from input columns (temper_ref._col_arg) and DATA operands read
    from launch parameters `base + column`."""
    if a.kind == abi.ARG_DATA:
        return abi.Arg(abi.ARG_PARAM, base + a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_EXPR:
        ops = (abi.ExprOp * a.ref).from_address(a.table)
        prog = [((abi.EXPR_INPUT, lat[o.ref], o.value) if o.op == abi.EXPR_SITE else
                 (abi.EXPR_PARAM, base + o.ref, o.value) if o.op == abi.EXPR_DATA else (o.op, o.ref, o.value)) for o in ops]
        return abi.expr_arg(prog, keep)
    return R._col_arg(a, lat, keep)


class Assess:
    """assess(x) of a lowered plated model: (lp, ll) float32 numpy from oracle plans and the float64 row sum."""

    def __init__(self, oracle_ops, tracer, data, impl=1):
        """`data`: the plan's data columns as float32 numpy arrays of one length D, in column order."""
        self.ops, self.impl, self.keep, self._tracer = oracle_ops, impl, [], tracer
        self.data = [np.ascontiguousarray(c, dtype=np.float32) for c in data]
        self.base = len(tracer.params)
        lat = R._latent_index(tracer)
        self.L = len(lat)
        self.latent_plans, self.dists, self.observed = [], [], []  # observed: (plan, plated?) in table order
        for q, s in enumerate(tracer.sites):
            c = abi.Site.from_buffer_copy(s)
            c.arg[0], c.arg[1] = _param_arg(s.arg[0], lat, self.base, self.keep), _param_arg(s.arg[1], lat, self.base, self.keep)
            plated = s.observed == abi.SITE_PLATED
            c.observed, c.out_col = 1, -1
            if q in lat:
                c.obs = abi.Arg(abi.ARG_INPUT, lat[q], 1.0, 0.0, None)
                plan = oracle_ops.plan_create([c])
                self.latent_plans.append(plan)
                self.dists.append(s.dist)
            else:
                if plated:
                    assert s.obs.kind == abi.ARG_DATA  # (what the lowering emits: the observed column itself)
                    c.obs = abi.Arg(abi.ARG_PARAM, self.base + s.obs.ref, s.obs.scale, s.obs.offset, None)
                plan = oracle_ops.plan_create([c])
                self.observed.append((plan, plated))
            if tracer.params and not (plated and q not in lat):
                plan.set_params(tracer.params)

    def _logw(self, plan, ins, n):
        kb = prng.split_lazy(prng.key(0, self.impl), n)  # (no latent site: no draw is made)
        return self.ops.importance_run(plan, kb, n, ins, [], want_score=False, want_max_partials=False)[2].numpy().copy()

    def row_terms(self, plan, ins, n):
        """t_d for every row: float32 [D, n]."""
        D = len(self.data[0])
        out = np.empty((D, n), dtype=np.float32)
        for d in range(D):
            plan.set_params(list(self._tracer.params) + [float(c[d]) for c in self.data])
            out[d] = self._logw(plan, ins, n)
        return out

    def __call__(self, x):
        n = len(x[0])
        x = [np.ascontiguousarray(c, dtype=np.float32) for c in x]
        ins = [torch.from_numpy(c) for c in x]
        lp = np.zeros(n, dtype=np.float32)
        ll = np.zeros(n, dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for l, plan in enumerate(self.latent_plans):
                term = self._logw(plan, ins, n)
                if self.dists[l] == abi.DIST_GAMMA:
                    term = np.where(x[l] > 0, term, np.float32(-np.inf))
                elif self.dists[l] == abi.DIST_BETA:
                    term = np.where((x[l] > 0) & (x[l] < 1), term, np.float32(-np.inf))
                lp = (lp + term).astype(np.float32)
            for plan, plated in self.observed:
                if not plated:
                    ll = (ll + self._logw(plan, ins, n)).astype(np.float32)
                    continue
                acc = np.zeros(n, dtype=np.float64)
                for t in self.row_terms(plan, ins, n):  # rows in order: acc = acc + (double) t_d
                    acc = acc + t.astype(np.float64)
                ll = (ll + acc.astype(np.float32)).astype(np.float32)
        return lp, ll


# ---- the models --------------------------------------------------------------------------------------------------------
MODELS = ("normal", "hetero", "logistic", "gamma_rate")


def bodies():
    from genjax import flip, gamma, gen, normal

    @gen
    def normal_reg(xs, s):
        w = normal(0.0, 2.0) @ "w"
        b = normal(0.0, 2.0) @ "b"
        normal(w * xs + b, s) @ "y"

    @gen
    def hetero(xs, ss):  # a data-dependent scale, times a Gamma latent (whose support rule the tests exercise)
        w = normal(0.0, 2.0) @ "w"
        s0 = gamma(2.0, 2.0) @ "s0"
        normal(w * xs, s0 * ss) @ "y"

    @gen
    def logistic(x1, x2):
        w1 = normal(0.0, 2.0) @ "w1"
        w2 = normal(0.0, 2.0) @ "w2"
        b = normal(0.0, 2.0) @ "b"
        flip(torch.sigmoid(w1 * x1 + w2 * x2 + b)) @ "y"

    @gen
    def gamma_rate(xs):
        w = normal(0.0, 1.0) @ "w"
        gamma(2.0, torch.exp(w * xs)) @ "y"

    return dict(normal=normal_reg, hetero=hetero, logistic=logistic, gamma_rate=gamma_rate)


def target(name, D, seed=0, inf_row=False):
    """-> (Target, the data tensors in argument order then the observed column).  `inf_row`: one +inf observed value
    (models with a float value)."""
    from genjax import ChoiceMap, Target

    rng = np.random.default_rng(1000 * seed + D)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    xs = rng.uniform(-1.0, 1.0, D)
    body = bodies()[name]
    if name == "normal":
        ys = 0.7 * xs - 0.3 + 0.1 * rng.standard_normal(D)
        args, y = (f(xs), 0.1), f(ys)
    elif name == "hetero":
        ss = rng.uniform(0.5, 1.5, D)
        args, y = (f(xs), f(ss)), f(0.7 * xs + ss * rng.standard_normal(D))
    elif name == "logistic":
        x2 = rng.uniform(-1.0, 1.0, D)
        p = 1.0 / (1.0 + np.exp(-(1.5 * xs - 1.0 * x2 + 0.2)))
        args, y = (f(xs), f(x2)), torch.from_numpy(rng.random(D) < p)
    else:
        args, y = (f(xs),), f(rng.gamma(2.0, 1.0, D) / np.exp(0.5 * xs))
    if inf_row and y.dtype == torch.float32:
        y[D // 2] = float("inf")
    return Target(body, args, ChoiceMap.d({"y": y})), [a for a in args if isinstance(a, torch.Tensor)] + [y]


def columns(name, n, rng, outside=False):
    """Start columns of a model's latents, float32 numpy; `outside`: every fourth value of a Gamma latent outside its
    support (negative, zero, NaN)."""
    L = {"normal": 2, "hetero": 2, "logistic": 3, "gamma_rate": 1}[name]
    cols = [(1.5 * rng.standard_normal(n)).astype(np.float32) for _ in range(L)]
    if name == "hetero":
        cols[1] = rng.gamma(2.0, 0.5, n).astype(np.float32)
        if outside:
            bad = np.array([-0.5, 0.0, np.nan, -1e-30], dtype=np.float32)
            cols[1][::4] = bad[np.arange(len(cols[1][::4])) % 4]
    return cols


# ---- 2. the float64 restatement on the conjugate regression with D rows ---------------------------------------------------
def conjugate(D=500):
    """temper_ref.Regression at m = D: y_d ~ N(w x_d + b, 0.1), w, b ~ N(0, 2); log_lik is the vector likelihood."""
    return R.Regression(m=D, noise=0.1, prior_sd=2.0, seed=0)


def restatement_errors(model, n, n_moves, seeds):
    """-> (log Z errors, posterior-mean errors of (w, b) in posterior standard deviations) of temper_ref.tempered_f64 over
    `seeds`: float64 numpy, numpy's own generator."""
    sd = np.sqrt(np.diag(model.post_cov))
    ez, em = [], []
    for s in seeds:
        r = R.tempered_f64(model, n, n_moves, 0.5, np.random.default_rng(s))
        ez.append(r["log_z"] - model.log_z)
        em.append([(r["w"].mean() - model.post_mean[0]) / sd[0], (r["b"].mean() - model.post_mean[1]) / sd[1],
                   r["w"].std() / sd[0] - 1.0, r["b"].std() / sd[1] - 1.0])
    return np.asarray(ez), np.asarray(em)


# ---- the two-plate regression: the second latent is declared BETWEEN the plates (temper.prior_table renumbers) -----------------
TWO_PLATE = '''def model(xs, zs):
    w = normal(0.0, 2.0) @ "w"
    normal(w * xs, 0.2) @ "y1"
    b = normal(0.0, 2.0) @ "b"
    normal(w * zs + b, 0.3) @ "y2"
'''


def two_plate_data(D=200, seed=0):
    """(xs, zs, y1, y2): f32 columns (the closed form is taken at exactly these numbers)."""
    rng = np.random.default_rng(seed)
    xs, zs = np.linspace(-1.0, 1.0, D), rng.uniform(-1.0, 1.0, D)
    y1 = 0.7 * xs + 0.2 * rng.standard_normal(D)
    y2 = 0.7 * zs - 0.3 + 0.3 * rng.standard_normal(D)
    return tuple(np.asarray(c, dtype=np.float32) for c in (xs, zs, y1, y2))


def two_plate(D=200, seed=0):
    """The closed form of TWO_PLATE from the stacked design: rows (xs_d, 0) at noise 0.2, then (zs_d, 1) at noise 0.3."""
    xs, zs, y1, y2 = (c.astype(np.float64) for c in two_plate_data(D, seed))
    X = np.concatenate([np.stack([xs, np.zeros(D)], axis=1), np.stack([zs, np.ones(D)], axis=1)])
    noise = np.concatenate([np.full(D, float(np.float32(0.2))), np.full(D, float(np.float32(0.3)))])
    return R.DesignRegression(X, np.concatenate([y1, y2]), noise, prior_sd=2.0)
