"""What the count-family suites (test_counts_cpu.py, test_gpu_counts.py) share: the grid of include/gjx_counts.h's densities
with its scipy float64 fixture (tests/golden/logpmf_counts.json, written by `write_golden` below — the only function here that
needs scipy), plain float64 densities, the tolerances, a numpy-f32 restatement of the header's density formulas, the header's
draw rule replayed in float64 from the cipher words (the host ciphers restated in numpy), and the recorded sampling noise the
statistical checks are held to.  Nothing here calls the code under test."""

import json
import math
import os

import numpy as np
import torch

import dist_range_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "logpmf_counts.json")

POISSON_RATES = [1e-3, 0.05, 1.0, 3.0, 9.99, 10.0, 10.01, 50.0, 1e3, 1e4, 1e5, 1e6]
NB_TOTALS = [0.05, 0.5, 1.0, 3.0, 7.99, 8.0, 8.01, 50.0, 1e3, 1e4]  # (across m_lgamma's switch at 8)
NB_PROBS = [1e-3, 0.1, 0.3, 0.5, 0.9, 0.999]
MAX_OBSERVED = 1 << 24


def f32(x):
    return float(np.float32(x))


def _points(ppf):
    ks = [0.0, 1.0] + [float(k) for k in ppf(np.array(R.QUANTILES, dtype=np.float64))]
    out = []
    for k in ks:
        assert k == f32(k) and 0 <= k <= MAX_OBSERVED
        if k not in out:
            out.append(k)
    return out


def density_cases():
    """The fixture's content (scipy).  Every parameter is an f32 value written as a double, every k an integer below 2^24;
    `logpmf` is scipy's float64 value at exactly those numbers.  TFP's NegativeBinomial(total_count, probs) counts the
    successes before total_count failures: scipy's nbinom(n = total_count, p = 1 - probs)."""
    from scipy import stats

    poi, nb = [], []
    for r in POISSON_RATES:
        r32 = f32(r)
        d = stats.poisson(r32)
        ks = _points(d.ppf)
        poi.append({"rate": r32, "k": ks, "logpmf": [float(d.logpmf(k)) for k in ks]})
    for t in NB_TOTALS:
        for p in NB_PROBS:
            t32, p32 = f32(t), f32(p)
            d = stats.nbinom(t32, 1.0 - p32)
            ks = _points(d.ppf)
            nb.append({"total_count": t32, "probs": p32, "k": ks, "logpmf": [float(d.logpmf(k)) for k in ks]})
    return {"poisson": poi, "negative_binomial": nb}


def write_golden():
    with open(GOLDEN, "w") as f:
        json.dump(density_cases(), f, indent=0)
        f.write("\n")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- float64 densities (torch.lgamma: nothing below needs scipy) ---------------------------------------------------------------
def _lgamma(a):
    return torch.lgamma(torch.as_tensor(np.asarray(a, dtype=np.float64))).numpy()


def _xlogy(a, y):
    a, y = np.asarray(a, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(a == 0, 0.0, a * np.log(np.where(a == 0, 1.0, y)))


def poisson_logpmf(k, rate):
    k, rate = np.asarray(k, dtype=np.float64), np.asarray(rate, dtype=np.float64)
    return _xlogy(k, rate) - rate - _lgamma(k + 1.0)


def nb_logpmf(k, r, p):
    k, r, p = (np.asarray(v, dtype=np.float64) for v in (k, r, p))
    return _lgamma(k + r) - _lgamma(k + 1.0) - _lgamma(r) + _xlogy(k, p) + r * np.log1p(-p)


# ---- tolerances, from bounds the suite already pins (dist_range_ref.py: lgamma to 1e-5 max(1, |lgamma|), log to 2e-7 relative,
# the roundings of products and sums 6e-8 of their terms) — never from the code under test ----------------------------------------
def poisson_tolerance(k, rate):
    k, rate = np.asarray(k, dtype=np.float64), np.asarray(rate, dtype=np.float64)
    return 1e-5 * np.maximum(1.0, np.abs(_lgamma(k + 1.0))) + 1e-6 * (np.abs(_xlogy(k, rate)) + rate + k + 1.0)


def nb_tolerance(k, r, p):
    k, r, p = (np.asarray(v, dtype=np.float64) for v in (k, r, p))
    lg = sum(np.maximum(1.0, np.abs(_lgamma(v))) for v in (k + r, k + 1.0, r))
    return 1e-5 * lg + 1e-6 * (np.abs(_xlogy(k, p)) + np.abs(r * np.log1p(-p)) + k + r + 1.0)


# ---- the header's density formulas in numpy float32: every operator rounds once, m_lgamma's recurrence and series as
# DESIGN.md §3 states them, the logarithm numpy's f32 one (inside the 2e-7 the spec's is pinned to) ---------------------------------
F = np.float32


def m_lgamma32(x):
    x = np.asarray(x, dtype=F).copy()
    p = np.ones_like(x)
    for _ in range(8):
        low = x < F(8.0)
        p = np.where(low, p * x, p).astype(F)
        x = np.where(low, x + F(1.0), x).astype(F)
    xi = (F(1.0) / x).astype(F)
    xi2 = (xi * xi).astype(F)
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(F)  # noqa: E731  (one rounding)
    s = fma(xi2, F(7.9365079365e-4), F(-2.7777777778e-3))
    s = (s.astype(np.float64) * xi2.astype(np.float64) + np.float64(F(8.3333333333e-2))).astype(F)
    s = (s * xi).astype(F)
    r = ((x - F(0.5)) * np.log(x).astype(F)).astype(F)
    r = (r - x).astype(F)
    r = (r + F(0.91893853320467)).astype(F)
    r = (r + s).astype(F)
    return (r - np.log(p).astype(F)).astype(F)


def xlogy32(a, y):
    a, y = np.asarray(a, dtype=F), np.asarray(y, dtype=F)
    with np.errstate(all="ignore"):
        return np.where(a == 0, F(0.0), (a * np.log(y).astype(F)).astype(F)).astype(F)


def poisson_logpmf32(k, rate):
    k, rate = np.asarray(k, dtype=F), np.asarray(rate, dtype=F)
    lf = m_lgamma32(k + F(1.0))
    return ((xlogy32(k, rate) - rate).astype(F) - lf).astype(F)


def nb_logpmf32(k, r, p):
    k, r, p = (np.asarray(v, dtype=F) for v in (k, r, p))
    lf = m_lgamma32(k + F(1.0))
    t = (m_lgamma32((k + r).astype(F)) - lf).astype(F)
    t = (t - m_lgamma32(r)).astype(F)
    t = (t + xlogy32(k, p)).astype(F)
    return (t + xlogy32(r, (F(1.0) - p).astype(F))).astype(F)


# ---- the host ciphers, vectorised (genjax/_amd/prng.py restates them for scalars), and a site's draw stream --------------------
M = np.uint64(0xFFFFFFFF)
TAG_STREAM = 0x52


def threefry2x32(k0, k1, c0, c1):
    k0, k1, c0, c1 = (np.asarray(v, dtype=np.uint64) for v in (k0, k1, c0, c1))
    ks = (k0, k1, np.uint64(0x1BD11BDA) ^ k0 ^ k1)
    x0, x1 = (c0 + k0) & M, (c1 + k1) & M
    rot = ((13, 15, 26, 6), (17, 29, 16, 24))
    for blk in range(5):
        for r in rot[blk & 1]:
            x0 = (x0 + x1) & M
            x1 = (((x1 << np.uint64(r)) | (x1 >> np.uint64(32 - r))) & M) ^ x0
        x0 = (x0 + ks[(blk + 1) % 3]) & M
        x1 = (x1 + ks[(blk + 2) % 3] + np.uint64(blk + 1)) & M
    return x0, x1


def philox4x32(k0, k1, c0, c1, c2, c3):
    k0, k1, c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in (k0, k1, c0, c1, c2, c3))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c0, c1, c2, c3


class Streams:
    """The draw streams Stream<impl>(split(parent)[first + i], true, fold), i = 0 .. n - 1, of a lazy key batch under a
    lane-0 parent (gjx.h mode 1): words(sub) -> (w0, w1) as uint64 arrays holding 32-bit values."""

    def __init__(self, impl, parent, first, n, fold):
        self.impl, self.n, self.fold = impl, n, fold
        i = np.arange(first, first + n, dtype=np.uint64)
        p0, p1 = np.uint64(parent[0]), np.uint64(parent[1])
        if impl == 0:
            c0, c1 = threefry2x32(p0, p1, i >> np.uint64(32), i & M)             # split_at
            self.k0, self.k1 = threefry2x32(c0, c1, np.uint64(0), np.uint64(fold))  # fold_in
        else:
            lane = i + np.uint64(1)
            self.k0, self.k1, self.l0, self.l1 = p0, p1, lane & M, lane >> np.uint64(32)

    def words(self, sub):
        if self.impl == 0:
            return threefry2x32(self.k0, self.k1, np.uint64(0), np.uint64(sub))
        o = philox4x32(self.k0, self.k1, self.l0, self.l1, np.uint64(sub), np.uint64(((self.fold + 1) << 8) | TAG_STREAM))
        return o[0], o[1]

    def bits32(self, sub):
        """Stream::bits32 for sub >= 1 (what gjx_rng_bits returns there): THREEFRY w0 ^ w1, PHILOX w0."""
        w0, w1 = self.words(sub)
        return (w0 ^ w1) if self.impl == 0 else w0


def uniform01(w):
    """gjx_device.hpp uniform01: the top 23 bits as a multiple of 2^-23 — exact in f32 and in f64."""
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) * 2.0 ** -23


# ---- the header's Poisson rule in float64, from the same words -----------------------------------------------------------------
def poisson_replay(st: Streams, B: int, rate):
    """include/gjx_counts.h poisson(st, B, rate) with every operation in float64: equal to the f32 kernel except where an f32
    rounding moves a comparison or a floor (the bound on how often is the test's, from the header)."""
    rate = np.broadcast_to(np.asarray(rate, dtype=np.float64), (st.n,)).copy()
    out = np.zeros(st.n, dtype=np.int64)
    out[~(rate >= 0)] = -1
    out[rate > 2.0 ** 30] = 1 << 30
    live = (rate > 0) & (rate <= 2.0 ** 30)
    small = live & (rate < 10)
    if small.any():
        w0, _ = st.words(B)
        u = uniform01(w0)
        p = np.exp(-rate)
        s = p.copy()
        k = np.zeros(st.n, dtype=np.float64)
        act = small & (u >= s)
        for _ in range(128):
            if not act.any():
                break
            k[act] += 1
            p[act] = p[act] * rate[act] / k[act]
            s[act] += p[act]
            act &= u >= s
        out[small] = k[small].astype(np.int64)
    big = live & (rate >= 10)
    if big.any():
        with np.errstate(all="ignore"):
            slam = np.sqrt(rate)
            b = 0.931 + 2.53 * slam
            a = -0.059 + 0.02483 * b
            l_inv_alpha = np.log(1.1239 + 1.1328 / (b - 3.4))
            vr = 0.9277 - 3.6224 / (b - 2.0)
            out[big] = np.floor(rate[big]).astype(np.int64)
            pend = big.copy()
            for att in range(64):
                if not pend.any():
                    break
                w0, w1 = st.words(B + 1 + att)
                U, V = uniform01(w0) - 0.5, uniform01(w1)
                us = 0.5 - np.abs(U)
                kf = np.floor((2.0 * a / us + b) * U + rate + 0.43)
                ok = (kf >= 0) & (kf < 2.0 ** 31)
                quick = ok & (us >= 0.07) & (V <= vr)
                rej = ~ok | (~quick & (us < 0.013) & (V > us))
                lhs = np.log(V) + l_inv_alpha - np.log(a / (us * us) + b)
                rhs = -rate + kf * np.log(rate) - _lgamma(np.where(ok, kf, 0.0) + 1.0)
                acc = pend & (quick | (~rej & (lhs <= rhs)))
                out[acc] = kf[acc].astype(np.int64)
                pend &= ~acc
    return out


# ---- recorded sampling noise ---------------------------------------------------------------------------------------------------
NB_MOMENT_CASES = [(0.5, 0.3), (3.0, 0.5), (50.0, 0.9)]
N_DRAWS = 100_000


def nb_moment_rms(seeds=24, n=N_DRAWS):
    """The RMS deviation of the sample mean and variance of n negative-binomial draws of numpy's own generator from
    r p / (1 - p) and r p / (1 - p)^2, over `seeds` seeds: what NB_MOMENT_RMS records."""
    out = {}
    for r, p in NB_MOMENT_CASES:
        m, v = r * p / (1 - p), r * p / (1 - p) ** 2
        dm, dv = [], []
        for s in range(seeds):
            x = np.random.default_rng(1000 + s).negative_binomial(r, 1.0 - p, size=n).astype(np.float64)
            dm.append(x.mean() - m)
            dv.append(x.var() - v)
        out[(r, p)] = (float(np.sqrt(np.mean(np.square(dm)))), float(np.sqrt(np.mean(np.square(dv)))))
    return out


# nb_moment_rms() as run when this file was written: (r, p) -> (RMS of the mean, RMS of the variance)
NB_MOMENT_RMS = {
    (0.5, 0.3): (0.0018942916846131632, 0.004020064331932156),
    (3.0, 0.5): (0.007162346275255452, 0.03468021402131342),
    (50.0, 0.9): (0.25368775267707255, 17.503951578717476),
}


# ---- the conjugate model of the end-to-end checks: lam ~ Gamma(a, b); y_d ~ Poisson(lam), d = 1 .. D ----------------------------
class GammaPoisson:
    """Closed forms: the posterior Gamma(a + S, b + D), the evidence, the posterior predictive (negative binomial: mean
    (a + S) / (b + D), variance mean (1 + 1 / (b + D))) and the exact leave-one-out predictive log-density of every row."""

    def __init__(self, D=200, a=2.0, b=1.0, lam=3.0, seed=0):
        self.D, self.a, self.b = D, a, b
        self.ys = np.random.default_rng(seed).poisson(lam, size=D).astype(np.float64)
        self.S = float(self.ys.sum())
        self.post = (a + self.S, b + D)  # (shape, rate)
        lg = lambda v: float(_lgamma(v))  # noqa: E731
        self.log_z = a * math.log(b) - lg(a) + lg(a + self.S) - (a + self.S) * math.log(b + D) - float(_lgamma(self.ys + 1.0).sum())
        self.post_mean = self.post[0] / self.post[1]
        self.pred_mean = self.post_mean
        self.pred_var = self.post_mean * (1.0 + 1.0 / self.post[1])
        al, be = a + self.S - self.ys, b + D - 1.0
        self.loo = (_lgamma(self.ys + al) - _lgamma(self.ys + 1.0) - _lgamma(al) + al * math.log(be / (be + 1.0))
                    - self.ys * math.log(be + 1.0))

    def log_prior(self, lam):
        with np.errstate(all="ignore"):
            v = (self.a - 1.0) * np.log(lam) - self.b * lam + self.a * math.log(self.b) - float(_lgamma(self.a))
        return np.where(lam > 0, v, -np.inf)

    def log_lik(self, lam):
        with np.errstate(all="ignore"):
            return self.S * np.log(lam) - self.D * lam - float(_lgamma(self.ys + 1.0).sum())

    def terms(self, lam):
        """t[d, i] = log Poisson(y_d; lam_i), float64 [D, n]."""
        return poisson_logpmf(self.ys[:, None], np.asarray(lam, dtype=np.float64)[None, :])

    def exact_draws(self, n, rng):
        return rng.gamma(self.post[0], 1.0 / self.post[1], size=n)


def tempered_f64(model: GammaPoisson, n, n_moves, ess_target, rng):
    """tests/temper_ref.py tempered_f64 — the sampler of genjax/_amd/temper.py in float64 numpy, numpy's own generator —
    over the ONE Gamma latent of GammaPoisson (temper_ref's is written for the two Normal latents of its regression): the same
    schedule rule, systematic resampling, 2.38 weighted-deviation scale, K random-walk sweeps per stage, the last stage moved."""
    import temper_ref as T
    from genjax._amd import temper

    lam = rng.gamma(model.a, 1.0 / model.b, size=n)
    lp, ll = model.log_prior(lam), model.log_lik(lam)
    beta, log_z = 0.0, 0.0
    while beta < 1.0:
        nb = temper.next_beta(beta, ess_target * n, lambda deltas: temper.ess_of(*T.ladder_ref(ll, deltas)[:2]))[0]
        lw = (nb - beta) * ll
        mx = lw.max()
        wt = np.exp(lw - mx)
        log_z += mx + math.log(wt.sum()) - math.log(n)
        wt /= wt.sum()
        mean = (lam * wt).sum()
        sc = 2.38 * math.sqrt((((lam - mean) ** 2) * wt).sum())
        a = T.systematic(rng, wt)
        lam, lp, ll = lam[a], lp[a], ll[a]
        for _ in range(n_moves):
            y = lam + sc * rng.standard_normal(n)
            lpn, lln = model.log_prior(y), model.log_lik(y)
            with np.errstate(invalid="ignore"):
                d = (lpn + nb * lln) - (lp + nb * ll)
                acc = (d >= 0.0) | (np.log(rng.random(n)) < d)
            lam, lp, ll = np.where(acc, y, lam), np.where(acc, lpn, lp), np.where(acc, lln, ll)
        beta = nb
    return dict(log_z=log_z, lam=lam)


E2E_N, E2E_SEEDS, E2E_FACTOR = 4096, tuple(range(9000, 9024)), 4.0


def e2e_statistics(model: GammaPoisson, lam, rng=None, pred=None, loo=None):
    """The statistics the end-to-end test compares, as deviations from the closed forms: the posterior mean of lam; the
    root-mean-square over the rows of the per-row predictive mean / variance deviation and the deviation of their averages
    over the rows (from `pred` = (mean [D], var [D]), or replicated here from `lam` with `rng`); sum_d elpd_loo_d (from `loo`,
    or the numpy PSIS of psis_ref over the float64 terms rounded to f32)."""
    import psis_ref as S

    n = len(lam)
    if pred is None:
        y = rng.poisson(np.broadcast_to(lam[None, :], (model.D, n))).astype(np.float64)
        pred = (y.mean(axis=1), y.var(axis=1, ddof=1))
    if loo is None:
        loo = float(S.psis(model.terms(lam).astype(np.float32), S.tail_len(n))["elpd"].sum())
    dm, dv = pred[0] - model.pred_mean, pred[1] - model.pred_var
    return dict(post_mean=float(np.mean(lam) - model.post_mean), pred_mean_rows=float(np.sqrt(np.mean(dm * dm))),
                pred_var_rows=float(np.sqrt(np.mean(dv * dv))), pred_mean_pooled=float(dm.mean()), pred_var_pooled=float(dv.mean()),
                elpd=float(loo - model.loo.sum()))


def e2e_rms(model=None, n=E2E_N, seeds=E2E_SEEDS):
    """What E2E_RMS records: per statistic the root-mean-square over `seeds` of its value on n EXACT posterior draws
    (float64 numpy); for log Z, where exact draws give no estimate, of the error of tempered_f64 (K = 2, ESS target 0.5)."""
    model = model or GammaPoisson()
    rows = []
    for s in seeds:
        rng = np.random.default_rng(s)
        st = e2e_statistics(model, model.exact_draws(n, rng), rng)
        st["log_z"] = tempered_f64(model, n, 2, 0.5, np.random.default_rng(s + 100))["log_z"] - model.log_z
        rows.append(st)
    return {k: float(np.sqrt(np.mean([r[k] ** 2 for r in rows]))) for k in rows[0]}


# e2e_rms() as run when this file was written
E2E_RMS = {
    "post_mean": 0.0022113163617593274, "pred_mean_rows": 0.02793161014527561, "pred_var_rows": 0.07658472428903428,
    "pred_mean_pooled": 0.0026516015456033194, "pred_var_pooled": 0.006229579328355395, "elpd": 0.027957834120281622,
    "log_z": 0.028224826317906,
}
