"""The references the pointwise kernels (include/gjx_pointwise.h, genjax/_amd/temper.py TemperedSMC.pointwise) are held to.

1. The TERMS t[d, i]: plate_ref.Assess.row_terms — one oracle run per data row through unchanged oracle entry points gives
   the bit-exact f32 log-density of a plated site at every particle; plans with more than one plated site add them in f32
   in table order.
2. The REDUCTIONS over the particles in float64 numpy: the log-sum-exp over the entries above -inf, the sum, the sum of
   squares and the count — and the bounds a float64 accumulation in ANY order keeps to them.
3. The closed form of the conjugate regression (plate_ref.conjugate): with (w, b) ~ N(mu, Sigma) the posterior,
   lppd_d -> log N(y_d; x_d' mu, noise^2 + x_d' Sigma x_d), and the Monte-Carlo spread of a population of 8192 around it."""

import math

import numpy as np

# Tolerances of the pin (tests/test_gpu_pointwise.py), derived, not tuned.
#   s1, s2   a float64 sum of n terms in any order is within (n - 1) u sum|v| of the exact one to first order, u = 2^-53;
#            the bound used is n 2^-52 sum|v| (reference and kernel each carry such an error), for s2 over v = t^2 with one
#            more rounding per product (a factor 1 + 2^-52 the n 2^-52 already exceeds; one extra unit is added).  One f32
#            ulp of ONE term moves the sum by 2^-24 |t|: these bounds pin the terms themselves.
#   lse      1e-4 absolute: the bound tests/test_gpu_temper.py::test_ess_ladder derives for an f32 exponential whose
#            argument is rounded in f32 (relative error of each exponential <= 2^-23 (1 + |t - m|), |t - m| < ~100 nats).
#            The pin asserts that spread on its reference.  (Beyond it the bound still holds — an entry more than 86 below
#            the running maximum is 0 to the spec's exponential and weighs less than e^-86 in truth — which is what the
#            edge cases, whose populations plate_ref.columns prescribes, rely on.)
LSE_TOL = 1e-4
LSE_MAX_SPREAD = 100.0
U52 = 2.0 ** -52

# Four times this is the bound of test_closed_form (tests/test_gpu_pointwise.py): the root-mean-square error, bias included,
# of sum_d lppd_d against the closed form on plate_ref.conjugate(500) over 24 populations of n = 8192 drawn from the exact
# posterior (default_rng(5000 .. 5023)), computed by closed_form_errors below — float64 numpy, not the code under test
# (2 s for the 24 populations; errors between -0.0020 and +0.0017, mean -0.00009).  The sum over the 500 rows is 435.137; the
# relative margin of the p_waic comparison is FACTOR * SPREAD / |sum| = 7.9e-6.
SPREAD_LPPD_SUM = 0.000864
CLOSED_FORM_FACTOR = 4.0
CLOSED_FORM_SEEDS = tuple(range(5000, 5024))


def terms(assess, cols):
    """t[d, i], float32 [D, n]: the f32 sum, in table order, of the plated sites' row terms (one site: its terms)."""
    import torch

    n = len(cols[0])
    ins = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)) for c in cols]
    out = None
    with np.errstate(invalid="ignore", over="ignore"):
        for plan, plated in assess.observed:
            if not plated:
                continue
            t = assess.row_terms(plan, ins, n)
            out = t if out is None else (out + t).astype(np.float32)
    assert out is not None
    return out


def reduce64(t):
    """-> float64 [4, D]: lse over the entries above -inf (-inf when none), sum, sum of squares, count."""
    t64 = np.asarray(t, dtype=np.float64)
    D = t64.shape[0]
    out = np.empty((4, D), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            v = t64[d]
            live = v[v > -np.inf]  # (false on NaN)
            if live.size:
                m = live.max()
                out[0, d] = m + math.log(np.exp(live - m).sum())
            else:
                out[0, d] = -np.inf
            out[1, d], out[2, d], out[3, d] = v.sum(), (v * v).sum(), live.size
    return out


def moment_bounds(t):
    """-> (bound of |s1 - ref|, bound of |s2 - ref|) per row, float64 [D] each (rows with NaN or infinite terms: NaN)."""
    t64 = np.abs(np.asarray(t, dtype=np.float64))
    n = t64.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        return n * U52 * t64.sum(axis=1), (n + 1) * U52 * (t64 * t64).sum(axis=1)


def spread(t):
    """max - min of the finite entries per row (the lse tolerance holds while it is below LSE_MAX_SPREAD)."""
    t64 = np.asarray(t, dtype=np.float64)
    fin = np.isfinite(t64)
    hi = np.where(fin, t64, -np.inf).max(axis=1)
    lo = np.where(fin, t64, np.inf).min(axis=1)
    return np.where(fin.any(axis=1), hi - lo, 0.0)


# Populations for the pin: the latents of a plate_ref model around the values plate_ref.target generates its data from, a
# tenth of a unit wide (the Gamma latent of `hetero` log-normal around 1) — a row's terms then spread a few nats to a few
# tens: new running maxima keep arriving (the rescale is exercised) and the spread stays below LSE_MAX_SPREAD, which
# plate_ref.columns (1.5 units wide: residuals of tens of noise deviations, thousands of nats) does not.
CENTRES = {"normal": (0.7, -0.3), "hetero": (0.7, 1.0), "logistic": (1.5, -1.0, 0.2), "gamma_rate": (0.5,)}


def centred_columns(name, n, rng, width=0.1):
    cols = [(c + width * rng.standard_normal(n)).astype(np.float32) for c in CENTRES[name]]
    if name == "hetero":
        cols[1] = np.exp(width * rng.standard_normal(n)).astype(np.float32)
    return cols


# ---- 3. the closed form ----------------------------------------------------------------------------------------------------
def closed_form_lppd(model):
    """float64 [D]: log N(y_d; x_d' mu, noise^2 + x_d' Sigma x_d) with x_d = (xs_d, 1) and (mu, Sigma) the posterior."""
    X = np.stack([model.xs, np.ones(model.m)], axis=1)
    var = model.noise ** 2 + np.einsum("di,ij,dj->d", X, model.post_cov, X)
    r = model.ys - X @ model.post_mean
    return -0.5 * (np.log(2 * np.pi * var) + r * r / var)


def posterior_columns(model, n, seed):
    """(w, b) float32 [n] each, drawn from the exact posterior with numpy's generator."""
    z = np.random.default_rng(seed).multivariate_normal(model.post_mean, model.post_cov, n)
    return [np.ascontiguousarray(z[:, 0], dtype=np.float32), np.ascontiguousarray(z[:, 1], dtype=np.float32)]


def terms_f64(model, cols):
    """The regression's log-densities in float64 numpy at the (f32) columns: [D, n]."""
    w, b = (np.asarray(c, dtype=np.float64) for c in cols)
    r = model.ys[:, None] - (model.xs[:, None] * w[None, :] + b[None, :])
    return -0.5 * (r / model.noise) ** 2 - (0.5 * math.log(2 * math.pi) + math.log(model.noise))


def closed_form_errors(model, n, seeds):
    """sum_d lppd_d of a posterior population minus the closed form, per seed."""
    exact = closed_form_lppd(model).sum()
    return np.asarray([(reduce64(terms_f64(model, posterior_columns(model, n, s)))[0] - math.log(n)).sum() - exact for s in seeds])
