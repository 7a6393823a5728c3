"""The references the covariance proposal of the tempered sampler (include/gjx_temper_cov.h) is held to.  Everything that is
not the proposal comes from tests/temper_ref.py, unchanged.

(a) move_cov_ref: temper_ref.move_ref with "propose" replaced by the header's rule — eps_l from the oracle's unchanged
    gjx_sample_logpdf_normal at loc 0, scale 1, the triangle accumulated in numpy f32.
(b) factor_ref: the header's Cholesky rule in numpy float64, operation by operation, fallback included.
(c) moments_ref: a two-pass float64 numpy computation, weights exp(lw - max) in float64.
(d) tempered_cov_f64: temper_ref.tempered_f64 with the covariance proposal (numpy's own generator: it shares no stream with the
    library), the library's schedule rule temper.next_beta; it returns the acceptance rate of every stage, and restates the
    diagonal sampler too so that both rates come from one piece of code.
(e) the correlated regression: a design that is not centred, as a site table and as a plated site."""

import math

import numpy as np
import torch

import temper_ref as R
from genjax._amd import prng, temper
from genjax._amd.ops import KeyBatch


def tri(l, j):
    """The packed position of entry (l, j), j <= l."""
    return l * (l + 1) // 2 + j


def unpack(packed, L):
    """A packed lower triangle -> [L, L] (zeros above the diagonal)."""
    out = np.zeros((L, L), dtype=np.asarray(packed).dtype)
    for l in range(L):
        for j in range(l + 1):
            out[l, j] = packed[tri(l, j)]
    return out


def pack(full):
    L = len(full)
    return np.array([full[l][j] for l in range(L) for j in range(l + 1)])


# ---- (a) the replay of the move -----------------------------------------------------------------------------------------
def move_cov_ref(oracle_ops, assess, key, x, lp, ll, beta, n_moves, factor, ancestors=None, recompute=False, stats=None):
    """gjx_temper_move_cov from oracle pieces.  factor: packed f32 [L (L + 1) / 2]; -> (x, lp, ll, n_accept int32), numpy."""
    n, L = len(x[0]), len(x)
    F = np.asarray(factor, dtype=np.float32)
    assert F.shape == (L * (L + 1) // 2,)
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
        eps = []
        for l in range(L):
            kb = KeyBatch(key.impl, 1, parent=(pr.k0, pr.k1), first=0, fold=(l + 1 if key.impl == 0 else l), parent_lane=pr.lane)
            eps.append(oracle_ops.sample_logpdf("normal", kb, n, 0.0, 1.0, want_score=False)[0].numpy().copy())
        y = []
        with np.errstate(invalid="ignore", over="ignore"):
            for l in range(L):
                t = (F[tri(l, 0)] * eps[0]).astype(np.float32)
                for j in range(1, l + 1):
                    t = (t + (F[tri(l, j)] * eps[j]).astype(np.float32)).astype(np.float32)
                y.append((x[l] + t).astype(np.float32))
        lpn, lln = assess(y)
        if stats is not None:
            stats["outside"] = stats.get("outside", 0) + int(np.isneginf(lpn).sum())
        bits = oracle_ops.rng_bits(KeyBatch(key.impl, 1, parent=(ar.k0, ar.k1), first=0, parent_lane=ar.lane), n, 0)
        u = torch.from_numpy(R.uniform01(bits.numpy()).copy())
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


# ---- (b) the factor -----------------------------------------------------------------------------------------------------
def factor_ref(S, L):
    """The header's rule on a packed float64 covariance S -> (c * G packed, float64; n_degenerate).  Python floats are IEEE
    doubles: every operation below rounds once."""
    S = [float(v) for v in np.asarray(S, dtype=np.float64)]
    assert len(S) == L * (L + 1) // 2
    G = [0.0] * len(S)
    ndeg = 0
    for l in range(L):
        for j in range(l):
            t = 0.0
            for k in range(j):
                t = t + G[tri(l, k)] * G[tri(j, k)]
            g = G[tri(j, j)]
            G[tri(l, j)] = 0.0 if g == 0.0 else _div(S[tri(l, j)] - t, g)
        t = 0.0
        for k in range(l):
            t = t + G[tri(l, k)] * G[tri(l, k)]
        sll = S[tri(l, l)]
        p = sll - t
        if not p > 2.0 ** -40 * sll:
            for j in range(l):
                G[tri(l, j)] = 0.0
            G[tri(l, l)] = math.sqrt(sll) if (sll > 0.0 and sll < math.inf) else 0.0
            ndeg += 1
        else:
            G[tri(l, l)] = math.sqrt(p)
    c = 2.38 / math.sqrt(float(L))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.array([c * g for g in G], dtype=np.float64), ndeg


def _div(a, b):
    return float(np.float64(a) / np.float64(b))  # (IEEE: no ZeroDivisionError, inf and NaN pass through)


def scales_ref(S, L):
    c = 2.38 / math.sqrt(float(L))
    return np.array([c * math.sqrt(S[tri(l, l)]) if S[tri(l, l)] > 0.0 else 0.0 for l in range(L)]).astype(np.float32)


# ---- (c) the moments ----------------------------------------------------------------------------------------------------
def moments_ref(x, lw=None):
    """Two passes in float64 -> (weight sum relative to the maximum, means [L], covariance packed).  Entries whose weight is
    -inf or NaN contribute nothing; no entry above -inf: zeros."""
    cols = np.stack([np.asarray(c, dtype=np.float64) for c in x])
    L, n = cols.shape
    if lw is None:
        w, ok = np.ones(n), np.ones(n, dtype=bool)
    else:
        lw = np.asarray(lw, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            ok = lw > -np.inf
        if not ok.any():
            return 0.0, np.zeros(L), np.zeros(L * (L + 1) // 2)
        w = np.where(ok, np.exp(np.where(ok, lw, 0.0) - lw[ok].max()), 0.0)
    cols, w = cols[:, ok], w[ok]
    ws = w.sum()
    mean = (cols * w).sum(axis=1) / ws
    dev = cols - mean[:, None]
    S = (dev * w) @ dev.T / ws
    return float(ws), mean, pack(S)


# ---- (d) the float64 restatement ----------------------------------------------------------------------------------------
def tempered_cov_f64(model, n, n_moves, ess_target, rng, betas=None, proposal="covariance"):
    """temper_ref.tempered_f64 with x' = x + F eps, F = 2.38 / sqrt(2) times the Cholesky factor (factor_ref) of the weighted
    population covariance before resampling; `proposal="diagonal"` is tempered_f64 itself, draw for draw (the same calls of
    `rng` in the same order), kept here for the acceptance rates tempered_f64 does not return.
    -> dict(log_z, betas, w, b, accept [one rate per stage])."""
    w, b = model.prior_sd * rng.standard_normal(n), model.prior_sd * rng.standard_normal(n)
    lp, ll = model.log_prior(w, b), model.log_lik(w, b)
    beta, out_betas, log_z, accept = 0.0, [0.0], 0.0, []
    fixed = None if betas is None else [float(x) for x in betas if x > 0.0]

    def ess_fn(deltas):
        s1, s2, _ = R.ladder_ref(ll, deltas)
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
        if proposal == "covariance":
            dev = cols - mean
            F = unpack(factor_ref(pack((dev * wt) @ dev.T), 2)[0], 2)
        else:
            sc = 2.38 / math.sqrt(2.0) * np.sqrt((((cols - mean) ** 2) * wt).sum(axis=1))
            F = np.diag(sc)
        a = R.systematic(rng, wt)
        w, b, lp, ll = w[a], b[a], lp[a], ll[a]
        n_acc = 0
        for _ in range(n_moves):
            e0, e1 = rng.standard_normal(n), rng.standard_normal(n)
            wn, bn = w + F[0, 0] * e0, b + (F[1, 0] * e0 + F[1, 1] * e1 if proposal == "covariance" else F[1, 1] * e1)
            lpn, lln = model.log_prior(wn, bn), model.log_lik(wn, bn)
            d = (lpn + nb * lln) - (lp + nb * ll)
            acc = (d >= 0.0) | (np.log(rng.random(n)) < d)
            w, b, lp, ll = np.where(acc, wn, w), np.where(acc, bn, b), np.where(acc, lpn, lp), np.where(acc, lln, ll)
            n_acc += int(acc.sum())
        accept.append(n_acc / (n * n_moves) if n_moves else 0.0)
        beta = nb
        out_betas.append(nb)
    return dict(log_z=log_z, betas=out_betas, w=w, b=b, accept=accept)


# The restatement on the correlated regression (correlated() below) at n = 4096, K = 2, ESS target 0.5 over the 64 seeds
# default_rng(1000 .. 1063) — measured on the CPU with numpy's generator, not on the code under test
# (profiles/temper_cov_summary.md; tests/test_temper_cov_cpu.py re-measures and prints them):
SEEDS = range(1000, 1064)
COV_RMS_LOG_Z = 0.0954       # covariance proposal: RMS error of log Z (errors -0.245 .. +0.192, mean -0.007)
COV_MIN_ACCEPT = 0.3409      # ... last-stage acceptance over the seeds 0.3409 / 0.3563 / 0.3723 (min / mean / max)
DIAG_RMS_LOG_Z = 0.2855      # diagonal proposal (tempered_f64): RMS error of log Z (errors -0.641 .. +0.484)
DIAG_MAX_ACCEPT = 0.0737     # ... last-stage acceptance 0.0380 / 0.0534 / 0.0736, the maximum rounded UP


def restatement_figures(proposal, seeds=SEEDS, n=4096, n_moves=2):
    """-> (log Z errors, last-stage acceptances, mean errors in posterior deviations [seeds, 2], variance ratios [seeds, 2])."""
    model = correlated()
    sd = np.sqrt(np.diag(model.post_cov))
    ez, acc, em, vr = [], [], [], []
    for s in seeds:
        r = tempered_cov_f64(model, n, n_moves, 0.5, np.random.default_rng(s), proposal=proposal)
        ez.append(r["log_z"] - model.log_z)
        acc.append(r["accept"][-1])
        em.append([(r["w"].mean() - model.post_mean[0]) / sd[0], (r["b"].mean() - model.post_mean[1]) / sd[1]])
        vr.append([r["w"].var() / sd[0] ** 2, r["b"].var() / sd[1] ** 2])
    return np.asarray(ez), np.asarray(acc), np.asarray(em), np.asarray(vr)


# ---- (e) the correlated regression --------------------------------------------------------------------------------------
NOISE, PRIOR_SD = 0.1, 2.0


def correlated_data(D=20):
    """(xs, ys) as f32 columns: xs = linspace(2, 3, D), ys drawn from default_rng(0) as temper_ref.Regression draws them
    (w = 0.7, b = -0.3, noise 0.1).  The closed form is taken at exactly these f32 numbers."""
    rng = np.random.default_rng(0)
    xs = np.linspace(2.0, 3.0, D)
    ys = 0.7 * xs - 0.3 + NOISE * rng.standard_normal(D)
    return xs.astype(np.float32), ys.astype(np.float32)


def correlated(D=20):
    """The closed form: a DesignRegression over X = [xs, 1].  The posterior correlation of (w, b) is -0.99 at D = 20."""
    xs, ys = (c.astype(np.float64) for c in correlated_data(D))
    X = np.stack([xs, np.ones(D)], axis=1)
    return R.DesignRegression(X, ys, np.full(D, float(np.float32(NOISE))), prior_sd=PRIOR_SD)


def correlated_target(D=20, plated=False):
    """The correlated regression as a Target: one observed site per row (the site-table form: the body of
    temper_ref.models()["regression"]), or one plated site over the data columns."""
    from genjax import ChoiceMap, Target, gen, normal

    xs, ys = correlated_data(D)
    if plated:
        @gen
        def regression_plated(xs, s):
            w = normal(0.0, 2.0) @ "w"
            b = normal(0.0, 2.0) @ "b"
            normal(w * xs + b, s) @ "y"

        return Target(regression_plated, (torch.from_numpy(xs), NOISE), ChoiceMap.d({"y": torch.from_numpy(ys)}))

    @gen
    def regression(xs, s):
        w = normal(0.0, 2.0) @ "w"
        b = normal(0.0, 2.0) @ "b"
        for i, x in enumerate(xs):
            normal(w * x + b, s) @ ("y", i)

    return Target(regression, ([float(x) for x in xs], NOISE), ChoiceMap.d({("y", i): float(y) for i, y in enumerate(ys)}))


def gaussian_chain_target(L):
    """L latents normal(0, 2), one observed normal(x_l + 0.5 x_{l-1}, 1) site per latent: a table whose packed factor index
    is exercised beyond L = 2."""
    from genjax import ChoiceMap, Target, gen, normal

    @gen
    def chain(L):
        xs = [normal(0.0, 2.0) @ ("x", l) for l in range(L)]
        for l in range(L):
            normal(xs[l] + 0.5 * xs[l - 1] if l else xs[l], 1.0) @ ("y", l)

    return Target(chain, (L,), ChoiceMap.d({("y", l): float(0.3 * ((l % 5) - 2)) for l in range(L)}))
