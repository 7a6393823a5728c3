"""The references the PSIS-LOO kernels (include/gjx_psis.h, genjax/_amd/temper.py TemperedSMC.loo) are held to: the header's
specification restated in float64 numpy, written from the header and sharing nothing with temper.py.

1. The TERMS t[d, i] are pointwise_ref.terms (bit-exact f32, replayed from unchanged oracle entry points).
2. SELECTION is np.sort under the header's integer key.
3. The body sum, the Zhang-Stephens fit, the smoothed weights and the estimate, with every sum in index order or, `rev`, in
   reversed order — the difference between the two is float64 reordering noise, which the tolerances below are a multiple of.
4. The closed-form leave-one-out of the conjugate regression (plate_ref.conjugate): the posterior refitted without row d,
   Gaussian predictive at row d.
5. The launch GEOMETRY as the headers state it (chunks of particles, rounds of 256 per chunk, keys sorted per row), so that
   the suites can assert which loops of the kernels a case runs more than once."""

import math

import numpy as np

MAX_TAIL = 4095
U52 = 2.0 ** -52

# ---- tolerances (tests/test_gpu_psis.py), derived or measured on the reference, never on the code under test ---------------
#   tail     bit for bit.
#   B        body_bound below: every term is an f32 exponential of an f32 argument — relative error <= 2^-23 (1 + |arg|), as
#            pointwise_ref.LSE_TOL is derived; a term whose argument is below -86 is 0 to the spec's exponential: its whole value
#            is the error — plus the float64 summation bound n 2^-52 sum for an accumulation in any order.
#   khat, sigma, elpd_loo   float64 arithmetic on bit-identical inputs: REORDER_FACTOR = 2^10 times the largest difference
#            between the reference's two evaluations (sums in index order / reversed) over the cases of the GPU suite, per
#            quantity, floor REORDER_FLOOR = 1e-11.  Measured by reorder_noise on those cases (n = 4096, 4099, 25; the four
#            plate_ref models and two_plate; centred, duplicated and outlier populations):
#                khat 2.9e-14, sigma 3.1e-14 (relative to sigma), elpd_loo 5.5e-14
#            (the largest on the `normal` model's rows, whose khat is between 0.9 and 3.5 at this population width; rows with
#            khat below 0.5 stay under 5e-15), so 2^10 times each is 3.0e-11, 3.2e-11, 5.6e-11: above the floor.  (The fit
#            amplifies: the candidates' weights are exponentials of M times a mean.)
REORDER_FACTOR = 2.0 ** 10
REORDER_FLOOR = 1e-11
MEASURED_REORDER = dict(khat=2.9e-14, sigma=3.1e-14, elpd=5.5e-14)
TOL = {q: max(REORDER_FACTOR * v, REORDER_FLOOR) for q, v in MEASURED_REORDER.items()}
# The same measurement on the cases of tests/test_gpu_psis_shapes.py (tail lengths up to 4095, n up to 526000), by reorder_noise
# on the reference's terms of every case; tests/test_psis_cpu.py::test_recorded_noise_covers_a_fresh_measurement repeats it.
# All three maxima come from ONE case, the `normal` model at n = 4200, M = 4095 (khat 1.9 .. 2.4: nearly the whole row is
# "tail", 93 candidates whose weights are exponentials of 4095 times a mean): khat 2.45e-13, sigma 2.46e-13, elpd 1.76e-12.
# Next: n = 4096, M = 4095 (9.9e-14, 9.9e-14, 2.0e-13) and M = 2047 (3.8e-14, 3.8e-14, 1.3e-13); the trip-count cases stay at
# or below the old table (n = 4099, D = 1100: 3.7e-14, 3.9e-14, 5.9e-14; the others under 5e-15), the key-space cases under
# 1e-14 (elpd 2.3e-14), the public call's population (n = 20000, M = 425, khat <= 0.15) under 3e-15.  So the table is LOOSER
# than the old one at the longest tails — by the reference's own measure, not by the kernel's — and the old one is untouched.
MEASURED_REORDER_LARGE = dict(khat=2.5e-13, sigma=2.5e-13, elpd=1.8e-12)
MEASURED_REORDER_LARGE_CASE = dict(khat=("normal", 4200, 4095), sigma=("normal", 4200, 4095), elpd=("normal", 4200, 4095))
TOL_LARGE = {q: max(REORDER_FACTOR * v, REORDER_FLOOR) for q, v in MEASURED_REORDER_LARGE.items()}

# The end-to-end case (tests/test_gpu_psis.py::test_end_to_end): plate_ref.conjugate(40), n = 4096.  Four times this is the bound:
# the root-mean-square error, bias included, of sum_d elpd_loo_d against the closed-form leave-one-out sum (closed_form_loo:
# 41.4803) over 24 populations of temper_ref.tempered_f64 (n = 4096, K = 2, ESS target 0.5, default_rng(8000 .. 8023)) through
# the numpy PSIS below — float64 numpy, not the code under test (e2e_errors; 2 s): errors between -0.084 and +0.079, mean
# -0.020.  The largest khat over those 24 populations and 40 rows is 0.302, below the threshold min(1 - 1 / log10(4096),
# 0.7) = 0.7: the case's condition n_high == 0 holds on the reference.  p_loo on the same populations: 1.16 .. 1.28, mean 1.231.
E2E_SPREAD_ELPD = 0.0410
E2E_FACTOR = 4.0
E2E_SEEDS = tuple(range(8000, 8024))
E2E_MAX_KHAT = 0.302

# The spread of the REFERENCE on populations from the exact posterior (tests/test_psis_cpu.py): the RMS error of sum_d elpd_loo_d
# against the closed form on plate_ref.conjugate(40) over 24 populations of n = 8192 (pointwise_ref.posterior_columns, seeds
# 5000 .. 5023): 0.0182 on a sum of 41.4803 (errors between -0.038 and +0.022, mean -0.0087; khat at most 0.23).
SPREAD_ELPD_SUM = 0.0182
CLOSED_FORM_FACTOR = 4.0
# The same at n = 20000 (M = 425; tests/test_gpu_psis_shapes.py::test_public_call_at_a_production_tail), same model, same 24
# seeds, closed_form_errors (4 s): 0.0104 (errors between -0.0266 and +0.0148, mean -0.0019; khat at most 0.314).
SPREAD_ELPD_SUM_20000 = 0.0104

# The two cases whose khat the GPU suite requires on both sides of the scale, chosen here on the CPU with this reference
# (tests/test_gpu_psis.py::test_khat_range): the `normal` model, D = 64 rows of plate_ref.target(seed=1), n = 4096,
#   high    centred_columns at width 0.1 with row 5's observed value moved by +0.5 (five noise deviations): reference khat
#           of that row 3.54 (every row of this population is above 0.7: it is as wide as the noise; the smallest is 0.71);
#   low     centred_columns at width 0.002 (a population far narrower than the noise): the tail is short and bounded,
#           the smallest reference khat is -0.303 (< 0), the largest 0.084.
HIGH_K = dict(width=0.1, row=5, shift=0.5)
LOW_K = dict(width=0.002)


def khat_case(which, data, population, n=4096, seed=34):
    """-> (latent columns, data columns) of the HIGH_K / LOW_K case.  `data`: the `normal` model's columns (xs, ys) of its 64
    rows; `population(name, n, kind, rng, width)`: the suite's population builder."""
    data = [np.array(c, dtype=np.float32) for c in data]
    spec = HIGH_K if which == "high" else LOW_K
    if which == "high":
        data[-1][spec["row"]] += np.float32(spec["shift"])
    return population("normal", n, "centred", np.random.default_rng(seed), spec["width"]), data


def tail_len(n, r_eff=1.0):
    """gjx_psis_tail_len: min(floor(0.2 n), ceil(3 sqrt(n / r_eff)), 4095), 0 below 5."""
    m = min(math.floor(0.2 * n), math.ceil(3.0 * math.sqrt(n / r_eff)), MAX_TAIL)
    return 0 if m < 5 else int(m)


def keys(t):
    """The header's total order: uint32 keys of f32 entries, every NaN 0xFFFFFFFF."""
    t = np.ascontiguousarray(t, dtype=np.float32)
    b = t.view(np.uint32)
    k = np.where(b >> 31 != 0, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(t)] = np.uint32(0xFFFFFFFF)
    return k


def select(row, M):
    """-> (tail f32 [M + 1] ascending, c_less) of one row of f32 entries."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    k = keys(row)
    order = np.argsort(k, kind="stable")
    tail = row[order[:M + 1]].copy()
    return tail, int((k < k[order[M]]).sum())


def body(row, M):
    """-> (B, its bound, bad) of one row: the float64 sum of exp at the f32-rounded arguments tT - t over the finite entries
    at or above the cutoff, minus the tail members tied with the cutoff."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    k = keys(row)
    tail, c_less = select(row, M)
    fin = np.isfinite(row)
    take = (k >= keys(tail[M:M + 1])[0]) & fin
    with np.errstate(invalid="ignore", over="ignore"):
        arg = (tail[M] - row[take]).astype(np.float32).astype(np.float64)
    e = np.exp(arg)
    G = float(e.sum())
    err = np.where(arg >= -86.0, e * 2.0 ** -23 * (1.0 + np.abs(arg)), e).sum() + len(row) * U52 * G
    return G - float(M - c_less), float(err), int((~fin).sum())


def _sum(v, rev, axis=None):
    v = np.asarray(v, dtype=np.float64)
    if rev:
        v = np.ascontiguousarray(v[..., ::-1])
    return v.sum(axis=axis)


def fit(tail, n, B, bad=0, rev=False):
    """The fit, the weights and the estimate of one row from its tail (f32 [M + 1] ascending) and body sum B.
    -> dict(elpd, khat, sigma, lw [M] (lw_j, j = 1 .. M), t [M] (t_j))."""
    M = len(tail) - 1
    t64 = np.asarray(tail, dtype=np.float64)
    s, tT = t64[0], t64[M]
    tj = t64[M - 1::-1]  # t_j = tail[M - j], j = 1 .. M
    if bad > 0:
        return dict(elpd=math.nan, khat=math.inf, sigma=math.nan, lw=np.full(M, math.nan), t=tj)
    e_cut = math.exp(s - tT)
    x = np.exp(s - tj) - e_cut
    xM, xstar = x[M - 1], x[int(math.floor(M / 4 + 0.5)) - 1]
    khat, sigma = math.inf, math.nan
    lw = s - tj
    if xM > 0.0 and xstar > 0.0:
        Gn = 30 + int(math.floor(math.sqrt(M)))
        j = np.arange(1, Gn + 1, dtype=np.float64)
        theta = 1.0 / xM + (1.0 - np.sqrt(Gn / (j - 0.5))) / (3.0 * xstar)
        kj = _sum(np.log1p(-theta[:, None] * x[None, :]), rev, axis=1) / M
        lj = M * (np.log(-theta / kj) - kj - 1.0)
        wj = 1.0 / _sum(np.exp(lj[None, :] - lj[:, None]), rev, axis=1)
        th = float(_sum(theta * wj, rev))
        k = float(_sum(np.log1p(-th * x), rev)) / M
        sigma = -k / th
        khat = (k * M + 5.0) / (M + 10.0)
        lp = np.log1p(-(np.arange(1, M + 1) - 0.5) / M)
        q = -sigma * lp if khat == 0.0 else sigma * np.expm1(-khat * lp) / khat
        with np.errstate(divide="ignore"):
            lw = np.minimum(np.log(q + e_cut), 0.0)
    e1 = lw + tj
    m1 = max(s, e1.max())
    m2 = max(s - tT, lw.max())
    s1 = float(_sum(np.exp(e1 - m1), rev)) + (n - M) * math.exp(s - m1)
    s2 = float(_sum(np.exp(lw - m2), rev)) + B * math.exp(s - tT - m2)
    return dict(elpd=(m1 + math.log(s1)) - (m2 + math.log(s2)), khat=khat, sigma=sigma, lw=lw, t=tj)


def psis(t, M, rev=False):
    """The whole header over a table t f32 [D, n] -> dict of float64 [D] arrays elpd, khat, sigma, s, tT, B, B_bound, bad and
    tail f32 [D, M + 1]."""
    t = np.ascontiguousarray(t, dtype=np.float32)
    D, n = t.shape
    out = {q: np.empty(D) for q in ("elpd", "khat", "sigma", "s", "tT", "B", "B_bound", "bad")}
    out["tail"] = np.empty((D, M + 1), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for d in range(D):
            tail, _ = select(t[d], M)
            B, bound, bad = body(t[d], M)
            f = fit(tail, n, B, bad, rev)
            out["tail"][d] = tail
            for q, v in (("elpd", f["elpd"]), ("khat", f["khat"]), ("sigma", f["sigma"]), ("s", tail[0]), ("tT", tail[M]), ("B", B),
                         ("B_bound", bound), ("bad", bad)):
                out[q][d] = v
    return out


def direct(row, M):
    """elpd_loo of one row by the DIRECT form, log sum_i w_i p_i - log sum_i w_i over all n entries in float64 (finite rows
    only): the raw log-weights s - t_i with the M largest replaced by the smoothed ones."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    tail, _ = select(row, M)
    B, _, bad = body(row, M)
    f = fit(tail, len(row), B, bad)
    ts = np.sort(row.astype(np.float64))
    lw = ts[0] - ts
    lw[:M] = f["lw"][::-1]  # (lw_j belongs to t_j = tail[M - j])
    a, b = lw + ts, lw
    return (a.max() + math.log(np.exp(a - a.max()).sum())) - (b.max() + math.log(np.exp(b - b.max()).sum()))


def reorder_noise(t, M):
    """The largest difference between the two evaluations (sums in index order / reversed) over the rows of t:
    dict(khat, sigma (relative), elpd) — rows that are not smoothed on either side give 0."""
    a, b = psis(t, M), psis(t, M, rev=True)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(a["khat"]) & np.isfinite(b["khat"])
        dk = np.abs(a["khat"] - b["khat"])[fin]
        ds = (np.abs(a["sigma"] - b["sigma"]) / np.abs(a["sigma"]))[fin]
        ok = np.isfinite(a["elpd"])
        de = np.abs(a["elpd"] - b["elpd"])[ok]
    return dict(khat=float(dk.max()) if dk.size else 0.0, sigma=float(ds.max()) if ds.size else 0.0, elpd=float(de.max()) if de.size else 0.0)


# ---- 5. the launch geometry (include/gjx_psis.h "body", gjx_pointwise.h "chunks"), restated from the headers' text -------------
def chunks(n, D):
    """-> (W, per): tiles = ceil(D / 4) row blocks, W = min(ceil(n / 256), max(1, ceil(2048 / tiles))) chunks of per =
    ceil(n / W) particles (the last ones shorter, or empty)."""
    tiles = -(-D // 4)
    W = min(-(-n // 256), max(1, -(-2048 // tiles)))
    return W, -(-n // W)


def chunk_sizes(n, D):
    """The particles of chunk c = 0 .. W - 1: lo = min(c per, n) .. min(lo + per, n)."""
    W, per = chunks(n, D)
    return [min((c + 1) * per, n) - min(c * per, n) for c in range(W)]


def trips(n, D):
    """The largest number of rounds of 256 particles a workgroup walks (lane l takes lo + l, lo + l + 256, ...)."""
    return max(-(-c // 256) for c in chunk_sizes(n, D))


def empty_chunks(n, D):
    return sum(c == 0 for c in chunk_sizes(n, D))


def first_trip(n, D):
    """bool [n]: the particles a workgroup reaches in its FIRST round of 256 — all of them exactly when trips(n, D) == 1."""
    W, per = chunks(n, D)
    i = np.arange(n)
    return i - (i // per) * per < 256


def sort_size(M):
    """The power of two at or above M + 1, at least 8: the keys one workgroup sorts (M + 1 tail entries, then padding)."""
    P = 8
    while P < M + 1:
        P *= 2
    return P


def candidates(M):
    """Gn of the fit."""
    return 30 + int(math.floor(math.sqrt(M)))


# ---- 4. the closed form ----------------------------------------------------------------------------------------------------
def closed_form_loo(model):
    """float64 [D]: log N(y_d; x_d' mu_-d, noise^2 + x_d' Sigma_-d x_d) with (mu_-d, Sigma_-d) the posterior of the conjugate
    regression (temper_ref.Regression) refitted without row d."""
    X = np.stack([model.xs, np.ones(model.m)], axis=1)
    out = np.empty(model.m)
    for d in range(model.m):
        keep = np.arange(model.m) != d
        Xk, yk = X[keep], model.ys[keep]
        cov = np.linalg.inv(Xk.T @ Xk / model.noise ** 2 + np.eye(2) / model.prior_sd ** 2)
        mu = cov @ (Xk.T @ yk) / model.noise ** 2
        var = model.noise ** 2 + X[d] @ cov @ X[d]
        r = model.ys[d] - X[d] @ mu
        out[d] = -0.5 * (math.log(2 * math.pi * var) + r * r / var)
    return out


def loo_f64(model, cols, r_eff=1.0):
    """The numpy PSIS over the regression's float64 log-densities at the columns, rounded to f32 as the kernels' terms are."""
    import pointwise_ref as W

    t = W.terms_f64(model, cols).astype(np.float32)
    return psis(t, tail_len(t.shape[1], r_eff))


def closed_form_errors(model, n, seeds):
    """sum_d elpd_loo_d of a population from the exact posterior minus the closed form, per seed."""
    import pointwise_ref as W

    exact = closed_form_loo(model).sum()
    return np.asarray([loo_f64(model, W.posterior_columns(model, n, s))["elpd"].sum() - exact for s in seeds])


def e2e_errors(model, n, seeds):
    """-> (errors of sum_d elpd_loo_d against the closed form, the largest khat, p_loo) per seed, over populations of
    temper_ref.tempered_f64 (K = 2, ESS target 0.5)."""
    import pointwise_ref as W
    import temper_ref as R

    exact = closed_form_loo(model).sum()
    err, kmax, p_loo = [], [], []
    for s in seeds:
        r = R.tempered_f64(model, n, 2, 0.5, np.random.default_rng(s))
        cols = [r["w"].astype(np.float32), r["b"].astype(np.float32)]
        out = loo_f64(model, cols)
        lppd = W.reduce64(W.terms_f64(model, cols))[0] - math.log(n)
        err.append(out["elpd"].sum() - exact)
        kmax.append(out["khat"].max())
        p_loo.append((lppd - out["elpd"]).sum())
    return np.asarray(err), np.asarray(kmax), np.asarray(p_loo)
