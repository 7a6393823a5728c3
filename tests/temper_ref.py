"""The references the tempered sampler (include/gjx_temper.h, genjax/_amd/temper.py) is held to.

1. The REPLAY of the header's specification from UNCHANGED oracle entry points (the oracle knows no gjx_temper.h):
   * assess: oracle importance plans over the model's own sites, every latent value read from input column l (the site's
     own arguments, programs and launch parameters untouched).  One single-site plan per latent gives that site's
     log-density column; lp is their f32 sum from +0 in table order under the header's support rule (numpy f32).  One
     plan over the observed sites gives ll: its log-weight column is that very sum;
   * keys: prng.fold_in on the host — k_r = fold_in(key, r), p_r = fold_in(k_r, 0), a_r = fold_in(k_r, 1);
   * proposals: the oracle's gjx_sample_logpdf_normal over the lazy children of p_r with fold l + 1 (THREEFRY) / l (PHILOX);
   * uniforms: the oracle's gjx_rng_bits over the lazy children of a_r, uniform01 restated in numpy, the spec's logarithm as
     the oracle's gjx_logpdf_bernoulli(value 1, probs u);
   * energies, the accept test and the select are numpy f32.
2. A float64 numpy RESTATEMENT of the whole sampler (numpy's own generator: it shares no stream with the library) for the
   linear-Gaussian regression, with the closed-form log Z and posterior."""

import math

import numpy as np
import torch

from genjax._amd import abi, prng, temper
from genjax._amd.ops import KeyBatch


# ---- 1. the replay ------------------------------------------------------------------------------------------------------
def _latent_index(tracer):
    out, l = {}, 0
    for q, m in enumerate(tracer.meta):
        if m["obs"] is None:
            out[q] = l
            l += 1
    return out


def _col_arg(a, lat, keep):
    """An argument with every reference to a latent site turned into a read of that latent's input column."""
    if a.kind == abi.ARG_SITE:
        return abi.Arg(abi.ARG_INPUT, lat[a.ref], a.scale, a.offset, None)
    if a.kind == abi.ARG_EXPR:
        ops = (abi.ExprOp * a.ref).from_address(a.table)
        prog = [((abi.EXPR_INPUT, lat[o.ref], o.value) if o.op == abi.EXPR_SITE else (o.op, o.ref, o.value)) for o in ops]
        return abi.expr_arg(prog, keep)
    return abi.Arg(a.kind, a.ref, a.scale, a.offset, a.table)


class Assess:
    """assess(x) of a lowered model from oracle importance plans: one single-site plan per latent (its log-weight column is
    that site's log-density), one plan over the observed sites (its log-weight column is ll)."""

    def __init__(self, oracle_ops, tracer, impl=1):
        self.ops, self.impl, self.keep = oracle_ops, impl, []
        lat = _latent_index(tracer)
        self.L = len(lat)
        self.latent_plans, self.dists, observed = [], [], []
        for q, s in enumerate(tracer.sites):
            c = abi.Site.from_buffer_copy(s)
            c.arg[0], c.arg[1] = _col_arg(s.arg[0], lat, self.keep), _col_arg(s.arg[1], lat, self.keep)
            c.observed, c.out_col = 1, -1
            if q in lat:
                c.obs = abi.Arg(abi.ARG_INPUT, lat[q], 1.0, 0.0, None)
                self.latent_plans.append(oracle_ops.plan_create([c]))
                self.dists.append(s.dist)
            else:
                observed.append(c)
        self.observed_plan = oracle_ops.plan_create(observed)
        for p in self.latent_plans + [self.observed_plan]:
            if tracer.params:
                p.set_params(tracer.params)
        self._tracer = tracer  # (tables and programs the sites point into)

    def _logw(self, plan, ins, n):
        kb = prng.split_lazy(prng.key(0, self.impl), n)  # (no latent site: no draw is made)
        return self.ops.importance_run(plan, kb, n, ins, [], want_score=False, want_max_partials=False)[2].numpy().copy()

    def __call__(self, x):
        """x: L float32 numpy columns -> (lp, ll) float32 numpy."""
        n = len(x[0])
        x = [np.ascontiguousarray(c, dtype=np.float32) for c in x]
        ins = [torch.from_numpy(c) for c in x]
        lp = np.zeros(n, dtype=np.float32)
        with np.errstate(invalid="ignore"):
            for l, plan in enumerate(self.latent_plans):
                term = self._logw(plan, ins, n)
                if self.dists[l] == abi.DIST_GAMMA:  # the header's support rule: -inf outside the OPEN support (NaN included)
                    term = np.where(x[l] > 0, term, np.float32(-np.inf))
                elif self.dists[l] == abi.DIST_BETA:
                    term = np.where((x[l] > 0) & (x[l] < 1), term, np.float32(-np.inf))
                lp = (lp + term).astype(np.float32)  # from +0, in table order, one rounding per add
        return lp, self._logw(self.observed_plan, ins, n)


def uniform01(bits):
    w = np.asarray(bits).view(np.uint32)
    return ((w >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)


def move_ref(oracle_ops, assess, key, x, lp, ll, beta, n_moves, scales, ancestors=None, recompute=False, stats=None):
    """gjx_temper_move from oracle pieces.  x: L float32 numpy columns; -> (x, lp, ll, n_accept int32), numpy.  `stats` (a dict):
    proposals whose log-prior is -inf (outside a latent's support) are counted into stats["outside"]."""
    n, L = len(x[0]), len(x)
    if ancestors is not None:
        a = np.minimum(np.asarray(ancestors).astype(np.int64) & 0xFFFFFFFF, n - 1)  # min((uint32) word, n - 1)
        x = [np.asarray(c, dtype=np.float32)[a] for c in x]
        lp, ll = (None, None) if recompute else (np.asarray(lp, dtype=np.float32)[a], np.asarray(ll, dtype=np.float32)[a])
    else:
        x = [np.asarray(c, dtype=np.float32).copy() for c in x]
    if recompute:
        lp, ll = assess(x)
    lp, ll = np.asarray(lp, dtype=np.float32).copy(), np.asarray(ll, dtype=np.float32).copy()
    beta = np.float32(beta)
    acc_n = np.zeros(n, dtype=np.int32)
    for r in range(int(n_moves)):
        kr = prng.fold_in(key, r)
        pr, ar = prng.fold_in(kr, 0), prng.fold_in(kr, 1)
        y = []
        for l in range(L):
            kb = KeyBatch(key.impl, 1, parent=(pr.k0, pr.k1), first=0, fold=(l + 1 if key.impl == 0 else l), parent_lane=pr.lane)
            y.append(oracle_ops.sample_logpdf("normal", kb, n, torch.from_numpy(x[l].copy()), float(np.float32(scales[l])),
                                              want_score=False)[0].numpy().copy())
        lpn, lln = assess(y)
        if stats is not None:
            stats["outside"] = stats.get("outside", 0) + int(np.isneginf(lpn).sum())
        bits = oracle_ops.rng_bits(KeyBatch(key.impl, 1, parent=(ar.k0, ar.k1), first=0, parent_lane=ar.lane), n, 0)
        u = torch.from_numpy(uniform01(bits.numpy()).copy())
        logu = oracle_ops.logpdf("bernoulli", n, 1, u).numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            h = (lp + (beta * ll).astype(np.float32)).astype(np.float32)
            hn = (lpn + (beta * lln).astype(np.float32)).astype(np.float32)
            d = (hn - h).astype(np.float32)
            acc = (d >= np.float32(0.0)) | (logu < d)  # both False on NaN
        x = [np.where(acc, y[l], x[l]) for l in range(L)]
        lp, ll = np.where(acc, lpn, lp), np.where(acc, lln, ll)
        acc_n += acc.astype(np.int32)
    return x, lp, ll, acc_n


def ladder_ref(ll, deltas):
    """float64 numpy: (S1, S2, M) of gjx_temper_ess_ladder."""
    ll = np.asarray(ll, dtype=np.float64)
    deltas = np.asarray(deltas, dtype=np.float32).astype(np.float64)
    ok = ll > -np.inf
    if not ok.any():
        return np.zeros(len(deltas)), np.zeros(len(deltas)), -np.inf
    M = ll[ok].max()
    c = ll[ok] - M
    s1 = np.array([np.exp(d * c).sum() for d in deltas])
    s2 = np.array([np.exp(2.0 * d * c).sum() for d in deltas])
    return s1, s2, M


# ---- 2. the float64 restatement on the linear-Gaussian regression ------------------------------------------------------------
class Regression:
    """y_i ~ N(w x_i + b, noise), w, b ~ N(0, prior_sd): closed-form evidence and posterior."""

    def __init__(self, m=20, noise=0.1, prior_sd=2.0, seed=0, w_true=0.7, b_true=-0.3):
        rng = np.random.default_rng(seed)
        self.xs = np.linspace(-1.0, 1.0, m)
        self.ys = w_true * self.xs + b_true + noise * rng.standard_normal(m)
        self.noise, self.prior_sd, self.m = noise, prior_sd, m
        X = np.stack([self.xs, np.ones(m)], axis=1)
        prec = X.T @ X / noise ** 2 + np.eye(2) / prior_sd ** 2
        self.post_cov = np.linalg.inv(prec)
        self.post_mean = self.post_cov @ (X.T @ self.ys) / noise ** 2
        C = noise ** 2 * np.eye(m) + prior_sd ** 2 * X @ X.T  # the marginal covariance of y
        _, logdet = np.linalg.slogdet(C)
        self.log_z = float(-0.5 * (m * math.log(2 * math.pi) + logdet + self.ys @ np.linalg.solve(C, self.ys)))

    def log_prior(self, w, b):
        s = self.prior_sd
        return -0.5 * (w * w + b * b) / s ** 2 - 2.0 * (0.5 * math.log(2 * math.pi) + math.log(s))

    def log_lik(self, w, b):
        r = self.ys[None, :] - (w[:, None] * self.xs[None, :] + b[:, None])
        return -0.5 * (r * r).sum(axis=1) / self.noise ** 2 - self.m * (0.5 * math.log(2 * math.pi) + math.log(self.noise))


class DesignRegression:
    """Regression's sibling over a design matrix and a noise vector: y_i ~ N(w X[i, 0] + b X[i, 1], noise_i), w, b ~ N(0,
    prior_sd) — several plated sites over one pair of latents, stacked.  The same closed forms and the same interface
    (tempered_f64 and plate_ref.restatement_errors take either)."""

    def __init__(self, X, ys, noise, prior_sd=2.0):
        self.X, self.ys = np.asarray(X, dtype=np.float64), np.asarray(ys, dtype=np.float64)
        self.noise, self.prior_sd, self.m = np.asarray(noise, dtype=np.float64), prior_sd, len(self.ys)
        Xw = self.X / self.noise[:, None] ** 2
        prec = self.X.T @ Xw + np.eye(2) / prior_sd ** 2
        self.post_cov = np.linalg.inv(prec)
        self.post_mean = self.post_cov @ (Xw.T @ self.ys)
        C = np.diag(self.noise ** 2) + prior_sd ** 2 * self.X @ self.X.T  # the marginal covariance of y
        _, logdet = np.linalg.slogdet(C)
        self.log_z = float(-0.5 * (self.m * math.log(2 * math.pi) + logdet + self.ys @ np.linalg.solve(C, self.ys)))

    log_prior = Regression.log_prior

    def log_lik(self, w, b):
        r = (self.ys[None, :] - (w[:, None] * self.X[None, :, 0] + b[:, None] * self.X[None, :, 1])) / self.noise[None, :]
        return -0.5 * (r * r).sum(axis=1) - (0.5 * math.log(2 * math.pi) * self.m + np.log(self.noise).sum())


def systematic(rng, w):
    n = len(w)
    c = np.cumsum(w)
    c[-1] = 1.0
    return np.searchsorted(c, (rng.random() + np.arange(n)) / n, side="right").clip(max=n - 1)


def tempered_f64(model: Regression, n, n_moves, ess_target, rng, betas=None, scale=None):
    """The sampler of genjax/_amd/temper.py in float64 numpy: the same schedule rule (temper.next_beta), systematic
    resampling, 2.38 / sqrt(L) weighted-deviation scales (or the fixed `scale`), K random-walk sweeps per stage, the last
    stage moved too.
    -> dict(log_z, betas, w, b)."""
    w, b = model.prior_sd * rng.standard_normal(n), model.prior_sd * rng.standard_normal(n)
    lp, ll = model.log_prior(w, b), model.log_lik(w, b)
    beta, out_betas, log_z = 0.0, [0.0], 0.0
    fixed = None if betas is None else [float(x) for x in betas if x > 0.0]

    def ess_fn(deltas):
        s1, s2, _ = ladder_ref(ll, deltas)
        return temper.ess_of(s1, s2)

    s = 0
    while beta < 1.0:
        nb = fixed[s] if fixed is not None else temper.next_beta(beta, ess_target * n, ess_fn)[0]
        s += 1
        lw = (nb - beta) * ll
        mx = lw.max()
        wt = np.exp(lw - mx)
        log_z += mx + math.log(wt.sum()) - math.log(n)
        wt /= wt.sum()
        cols = np.stack([w, b])
        mean = (cols * wt).sum(axis=1, keepdims=True)
        sc = 2.38 / math.sqrt(2.0) * np.sqrt((((cols - mean) ** 2) * wt).sum(axis=1))
        if scale is not None:
            sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), (2,))
        a = systematic(rng, wt)
        w, b, lp, ll = w[a], b[a], lp[a], ll[a]
        for _ in range(n_moves):
            wn, bn = w + sc[0] * rng.standard_normal(n), b + sc[1] * rng.standard_normal(n)
            lpn, lln = model.log_prior(wn, bn), model.log_lik(wn, bn)
            d = (lpn + nb * lln) - (lp + nb * ll)
            acc = (d >= 0.0) | (np.log(rng.random(n)) < d)
            w, b, lp, ll = np.where(acc, wn, w), np.where(acc, bn, b), np.where(acc, lpn, lp), np.where(acc, lln, ll)
        beta = nb
        out_betas.append(nb)
    return dict(log_z=log_z, betas=out_betas, w=w, b=b)


# ---- the models both test files use -----------------------------------------------------------------------------------------
def models():
    """-> {name: Target}: the README's regression (two Normal latents, expression arguments; m = 20, noise 0.1, the data of
    Regression()), a Gamma-precision / Normal model, and the README's beta-bernoulli."""
    from genjax import ChoiceMap, Target, beta, flip, gamma, gen, normal

    @gen
    def regression(xs, s):
        w = normal(0.0, 2.0) @ "w"
        b = normal(0.0, 2.0) @ "b"
        for i, x in enumerate(xs):
            normal(w * x + b, s) @ ("y", i)

    @gen
    def gamma_normal(a, ys_n):
        tau = gamma(a, 1.0) @ "tau"
        mu = normal(0.0, 2.0) @ "mu"
        for i in range(ys_n):
            normal(mu, 1.0 / tau.sqrt()) @ ("y", i)

    @gen
    def beta_bernoulli(a, b):
        p = beta(a, b) @ "p"
        v = flip(p) @ "v"
        return v

    reg = Regression()
    return {
        "regression": Target(regression, ([float(x) for x in reg.xs], reg.noise),
                             ChoiceMap.d({("y", i): float(y) for i, y in enumerate(reg.ys)})),
        "gamma_normal": Target(gamma_normal, (2.0, 3), ChoiceMap.d({("y", i): v for i, v in enumerate((0.4, -0.2, 0.9))})),
        "beta_bernoulli": Target(beta_bernoulli, (2.0, 2.0), ChoiceMap.d({"v": True})),
    }
