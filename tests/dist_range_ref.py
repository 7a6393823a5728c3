"""The distribution sites over the whole parameter range: the grid, plain float64 references and the checks that the CPU
suite (test_dist_range_cpu.py: the oracle against float64) and the GPU suite (test_gpu_dist_range.py: the HIP library against
the oracle, bit for bit, and against float64) share.

The grid leaves the band every other test stays in (positive arguments in about [0.05, 4]) on purpose: shapes on both sides
of the `conc < 1` boost of the gamma sampler (0.999 / 1 / 1.001) and of m_lgamma's switch from the recurrence to Stirling's
series (7.99 / 8 / 8.01), shapes whose draws underflow f32 (0.01, 0.05) and shapes where lgamma(a) + lgamma(b) - lgamma(a + b)
cancels (1e3, 1e4).  Expected log-densities are float64 scipy values committed as tests/golden/logpdf_wide.json (written by
tests/golden/make_golden.py from `density_cases` below), so nothing here needs scipy except `clipped_ks`."""

import json
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SHAPES = [0.01, 0.05, 0.2, 0.999, 1.0, 1.001, 7.99, 8.0, 8.01, 50.0, 1e3, 1e4]
RATES = [1e-3, 1.0, 1e3]
BETA_PAIRS = [(0.01, 0.01), (0.05, 0.05), (0.1, 5.0), (5.0, 0.1), (30.0, 0.3), (0.999, 1.001), (50.0, 80.0), (1e3, 1e3), (1e4, 3.0),
              (0.01, 1e4)]
BERNOULLI_P = [0.0, 2.0**-24, 1e-3, 0.5, 1.0 - 2.0**-24, 1.0]
NORMAL_SCALES = [1e-20, 1e-3, 1.0, 1e3, 1e20]  # (parity only)
NORMAL_LOCS = [0.0, 1e6, -1e6]
QUANTILES = [1e-6, 1e-3, 0.1, 0.5, 0.9, 0.999, 1.0 - 1e-6]
F32_MIN_NORMAL = 2.0**-126
F32_MIN_SUBNORMAL = 2.0**-149
# windows of the clipped Kolmogorov statistic.  Below 2^-100 a draw is an atom f32 rounding made (0, subnormals); above
# 1 - 2^-12 the floats are so coarse that, for b = 0.1, 1.6 % of Beta's mass lies between two ADJACENT floats below 1 and a
# window reaching 1 - 2^-23 fails on rounding alone (D = 0.012 there); at 1 - 2^-12 the mass per ulp is below 1e-4.
GAMMA_WINDOW = (2.0**-100, math.inf)
BETA_WINDOW = (2.0**-100, 1.0 - 2.0**-12)

N_LOG_SPACED = (0.01, 1e4)


def f32(x):
    """x rounded to f32, as the float64 number every reference is evaluated at."""
    return float(np.float32(x))


def gamma_sampler_cases():
    """(shape, rate) of the sampler checks: every shape, the rate cycling through the three rates."""
    return [(a, RATES[i % len(RATES)]) for i, a in enumerate(SHAPES)]


def gamma_density_params():
    return [(a, r) for a in SHAPES for r in RATES]


def _points(ppf, edges):
    xs = [f32(q) for q in ppf(np.array(QUANTILES, dtype=np.float64))] + [f32(e) for e in edges]
    out = []
    for x in xs:  # (quantiles of the small shapes round to 0 or 1: kept once)
        if x not in out:
            out.append(x)
    return out


def density_cases():
    """The fixture's content (needs scipy: called by tests/golden/make_golden.py only).  Every x and parameter is an f32
    value written as a double; `logpdf` is scipy's float64 log-density at exactly those numbers (+-inf as strings)."""
    from scipy import stats

    def enc(v):
        v = float(v)
        return v if math.isfinite(v) else ("inf" if v > 0 else "-inf")

    gam, bet = [], []
    with np.errstate(all="ignore"):
        for a, r in gamma_density_params():
            a32, r32 = f32(a), f32(r)
            d = stats.gamma(a32, scale=1.0 / r32)
            xs = _points(d.ppf, [0.0, F32_MIN_NORMAL, F32_MIN_SUBNORMAL])
            gam.append({"concentration": a32, "rate": r32, "x": xs, "logpdf": [enc(d.logpdf(x)) for x in xs]})
        for a, b in BETA_PAIRS:
            a32, b32 = f32(a), f32(b)
            d = stats.beta(a32, b32)
            xs = _points(d.ppf, [0.0, 1.0, F32_MIN_NORMAL, F32_MIN_SUBNORMAL])
            bet.append({"a": a32, "b": b32, "x": xs, "logpdf": [enc(d.logpdf(x)) for x in xs]})
    return {"gamma": gam, "beta": bet}


def golden():
    with open(os.path.join(HERE, "golden", "logpdf_wide.json")) as f:
        return json.load(f)


# ---- the tolerance of a log-density, from bounds the suite already pins (test_math_spec_accuracy), never from the code under
# test:  lgamma is pinned to 1e-5 * max(1, |lgamma|), so each lgamma the formula evaluates may contribute that;  log is pinned
# to 2e-7 * max(1, |log|), so a term c * log(y) is off by at most 2e-7 * (|c| + |c log y|), plus the f32 roundings of the
# product, of c = a - 1 and of 1 - x (6e-8 relative each, the last one 6e-8 * |c| absolute), plus the roundings of the sums
# (6e-8 of the partial sums): together below 1e-6 * (sum |other terms| + sum |their coefficients|).

def _abs_lgamma(a):
    """|lgamma(a)| in float64 for a number or an array (torch's: nothing here needs scipy)."""
    return torch.lgamma(torch.as_tensor(np.asarray(a, dtype=np.float64))).abs().numpy()


def gamma_tolerance(x, a, r):
    """x, a, r: numbers or arrays that broadcast (the grid passes two numbers and the points; tests/temper_fuzz.py whole tables)."""
    x, a, r = (np.asarray(v, dtype=np.float64) for v in (x, a, r))
    with np.errstate(all="ignore"):
        lx = np.where(x > 0, np.log(np.where(x > 0, x, 1.0)), 0.0)
        terms = np.abs((a - 1.0) * lx) + np.abs(r * x) + np.abs(a * np.log(r))
        return 1e-5 * np.maximum(1.0, _abs_lgamma(a)) + 1e-6 * (terms + np.abs(a - 1.0) + np.abs(a))


def beta_tolerance(x, a, b):
    x, a, b = (np.asarray(v, dtype=np.float64) for v in (x, a, b))
    with np.errstate(all="ignore"):
        lx = np.where(x > 0, np.log(np.where(x > 0, x, 1.0)), 0.0)
        l1x = np.where(x < 1, np.log1p(-np.where(x < 1, x, 0.0)), 0.0)
        terms = np.abs((a - 1.0) * lx) + np.abs((b - 1.0) * l1x)
        lg = sum(1e-5 * np.maximum(1.0, _abs_lgamma(v)) for v in (a, b, a + b))
        return lg + 1e-6 * (terms + np.abs(a - 1.0) + np.abs(b - 1.0))


def compare_logpdf(got, ref, tol, what):
    """`got` (f32 from the code under test) against the float64 `ref`: where the reference is infinite the same infinity,
    exactly; a NaN nowhere; elsewhere within `tol`.  Returns the largest finite error / tolerance ratio."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    assert not np.isnan(got).any(), f"{what}: NaN log-density at {np.flatnonzero(np.isnan(got))[:5].tolist()}"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), f"{what}: at the support's edge {got[inf][:8].tolist()} != {ref[inf][:8].tolist()}"
    fin = ~inf
    if not fin.any():
        return 0.0
    err = np.abs(got[fin] - ref[fin])
    worst = int(np.argmax(err / tol[fin]))
    assert (err <= tol[fin]).all(), (f"{what}: |{got[fin][worst]!r} - {ref[fin][worst]!r}| = {err[worst]:.3g} > "
                                    f"{tol[fin][worst]:.3g}")
    return float((err / tol[fin]).max())


def _dec(v):
    return float(v)  # ("inf" / "-inf" strings included)


def check_logpdf_grid(ops):
    """Shared by both suites: `ops.logpdf` of Gamma and Beta on the whole grid against logpdf_wide.json, and Bernoulli on its
    p grid against float64 log / log1p."""
    dev = ops.device()
    g = golden()
    for r in g["gamma"]:
        a, rate = r["concentration"], r["rate"]
        x = torch.tensor(r["x"], dtype=torch.float32)
        got = ops.logpdf("gamma", x.numel(), x.to(dev), a, rate).cpu().numpy()
        compare_logpdf(got, [_dec(v) for v in r["logpdf"]], gamma_tolerance(r["x"], a, rate), f"gamma({a}, {rate})")
    for r in g["beta"]:
        a, b = r["a"], r["b"]
        x = torch.tensor(r["x"], dtype=torch.float32)
        got = ops.logpdf("beta", x.numel(), x.to(dev), a, b).cpu().numpy()
        compare_logpdf(got, [_dec(v) for v in r["logpdf"]], beta_tolerance(r["x"], a, b), f"beta({a}, {b})")
    check_bernoulli_logpdf(ops)


def bernoulli_ref(e, p):
    """float64 log p / log(1 - p) at the f32 p, -inf at the impossible outcome."""
    p = f32(p)
    with np.errstate(all="ignore"):
        return float(np.log(np.float64(p))) if e else float(np.log1p(-np.float64(p)))


def check_bernoulli_logpdf(ops):
    for p in BERNOULLI_P:
        for e in (0, 1):
            got = float(ops.logpdf("bernoulli", 1, bool(e), f32(p)).cpu())
            ref = bernoulli_ref(e, p)
            # log: 2e-7 * max(1, |log|); the f32 rounding of 1 - p: 6e-8 relative in the argument = 6e-8 absolute in the log
            compare_logpdf([got], [ref], 2e-7 * max(1.0, abs(ref)) + 1e-7 if math.isfinite(ref) else 0.0, f"bernoulli({p}) e={e}")


def clipped_ks(samples, cdf, lo, hi):
    """The Kolmogorov statistic taken only at points of [lo, hi], and kstwo's survival function of it (conservative: a sup
    over a subset).  Inside the window both one-sided limits of the ECDF at every sample point, and the window's two ends;
    samples below lo and above hi count in the ECDF, so mass that f32 cannot represent (exact zeros, subnormals, ones) is
    lumped at the window's ends and not penalised."""
    from scipy import stats

    x = np.sort(np.asarray(samples, dtype=np.float64))
    n = x.size
    inside = x[(x >= lo) & (x <= hi)]
    pts = np.concatenate([[lo], inside, [hi]])
    with np.errstate(all="ignore"):
        F = np.asarray(cdf(pts), dtype=np.float64)
    right = np.searchsorted(x, pts, side="right") / n  # P(X <= pt)
    left = np.searchsorted(x, pts, side="left") / n    # P(X < pt)
    D = float(max(np.abs(right - F).max(), np.abs(left - F).max()))
    return D, float(stats.kstwo.sf(D, n))


def log_spaced(n, lo=N_LOG_SPACED[0], hi=N_LOG_SPACED[1], shift=0):
    """n shapes log-spaced over [lo, hi], cycling with a period of 61 lanes (odd: no alignment with waves, rows or quads), so
    that neighbouring particles sit on different sides of the boost branch and of the lgamma switch.  The grid's own values
    are planted at the head.  `shift` rotates the cycle (a second column then pairs every shape with another one)."""
    k = (torch.arange(n, dtype=torch.float64) + shift) % 61
    t = torch.exp(math.log(lo) + k / 60.0 * (math.log(hi) - math.log(lo))).to(torch.float32)
    head = torch.tensor(SHAPES, dtype=torch.float32)
    m = min(n, head.numel())
    if shift == 0:
        t[:m] = head[:m]
    return t


# ---- the plans of the GPU suite (site tables are host objects: the CPU suite compiles them offline) -------------------------

N_PARAMS = 3
PARAM_ROWS = [(1e-3, 0.05, 0.05), (1.0, 0.01, 1e4), (1e3, 30.0, 0.3), (1.0, 0.999, 1.001)]  # (gamma rate, beta a, beta b)
N_INPUTS = 4  # columns: gamma shapes, beta a, beta b, the observation
OBS_SCALE_C = 0.5


def _site(dist, a0, a1=None, obs=None, out_col=-1):
    from genjax._amd import abi

    s = abi.Site()
    s.dist, s.observed, s.out_col = dist, 0 if obs is None else 1, out_col
    s.arg[0] = a0
    if a1 is not None:
        s.arg[1] = a1
    if obs is not None:
        s.obs = obs
    return s


def importance_sites(kind):
    """-> (sites, value dtypes).  A Gamma site, a Beta site, a Bernoulli on the Beta, and an observed Normal whose scale is
    gamma * c + c.
      'inputs'      shapes from input columns (log-spaced per particle), the rate and a second Beta's shapes launch parameters
      'site_shape'  the Beta's first shape IS the Gamma draw: zeros, subnormals and tiny values feed a shape
      'lit_beta'    Beta(0.05, 0.05) as literals (the constant-hoisting path; the log-space branch compiled in)
      'lit_gamma'   Gamma(1e3, rate 1e-3) as literals"""
    from genjax._amd import abi

    A = abi.Arg
    c = lambda v: A(abi.ARG_CONST, 0, 0.0, v, None)  # noqa: E731
    inp = lambda i: A(abi.ARG_INPUT, i, 1.0, 0.0, None)  # noqa: E731
    par = lambda i: A(abi.ARG_PARAM, i, 1.0, 0.0, None)  # noqa: E731
    site = lambda i, sc=1.0, off=0.0: A(abi.ARG_SITE, i, sc, off, None)  # noqa: E731
    G, B, BE, NO = abi.DIST_GAMMA, abi.DIST_BETA, abi.DIST_BERNOULLI, abi.DIST_NORMAL
    f, i32 = torch.float32, torch.int32
    if kind == "inputs":
        return [_site(G, inp(0), par(0), out_col=0), _site(B, inp(1), inp(2), out_col=1), _site(BE, site(1), out_col=2),
                _site(B, par(1), par(2), out_col=3),
                _site(NO, c(0.0), site(0, OBS_SCALE_C, OBS_SCALE_C), obs=inp(3))], [f, f, i32, f]
    if kind == "site_shape":
        return [_site(G, inp(0), par(0), out_col=0), _site(B, site(0), inp(2), out_col=1), _site(BE, site(1), out_col=2),
                _site(NO, c(0.0), site(0, OBS_SCALE_C, OBS_SCALE_C), obs=inp(3))], [f, f, i32]
    if kind == "lit_beta":
        return [_site(G, inp(0), c(1.0), out_col=0), _site(B, c(0.05), c(0.05), out_col=1), _site(BE, site(1), out_col=2),
                _site(NO, c(0.0), site(0, OBS_SCALE_C, OBS_SCALE_C), obs=inp(3))], [f, f, i32]
    if kind == "lit_gamma":
        return [_site(G, c(1e3), c(1e-3), out_col=0), _site(B, inp(1), inp(2), out_col=1), _site(BE, site(1), out_col=2),
                _site(NO, c(0.0), site(0, OBS_SCALE_C * 1e-6, OBS_SCALE_C), obs=inp(3))], [f, f, i32]
    raise ValueError(kind)


IMPORTANCE_KINDS = ["inputs", "site_shape", "lit_beta", "lit_gamma"]


def input_columns(n):
    g = torch.Generator().manual_seed(n)
    a, b = log_spaced(n), log_spaced(n, shift=17)
    m = min(n, len(BETA_PAIRS))  # (the grid's own pairs at the head)
    a[:m] = torch.tensor([p[0] for p in BETA_PAIRS[:m]], dtype=torch.float32)
    b[:m] = torch.tensor([p[1] for p in BETA_PAIRS[:m]], dtype=torch.float32)
    return [log_spaced(n), a, b, torch.randn(n, generator=g)]


def carry_sites(init):
    """Gamma(0.05, .) and Beta(0.05, 0.05) feeding the carry, and an observed Normal: the step table of the scan plan and of
    the generated SMC filter (init=True: the filter's first step, which has no carry to read)."""
    from genjax._amd import abi

    A = abi.Arg
    c = lambda v: A(abi.ARG_CONST, 0, 0.0, v, None)  # noqa: E731
    rate = c(1.0) if init else A(abi.ARG_STATE, 0, 1.0, 1.0, None)
    loc = c(0.0) if init else A(abi.ARG_STATE, 1, 1.0, 0.0, None)
    return [_site(abi.DIST_GAMMA, c(0.05), rate, out_col=-1 if init else 0), _site(abi.DIST_BETA, c(0.05), c(0.05), out_col=-1 if init else 1),
            _site(abi.DIST_NORMAL, loc, A(abi.ARG_SITE, 0, OBS_SCALE_C, OBS_SCALE_C, None), obs=A(abi.ARG_OBS, 0, 1.0, 0.0, None))]


def carry_next():
    from genjax._amd import abi

    return [abi.Arg(abi.ARG_SITE, 0, 1.0, 0.0, None), abi.Arg(abi.ARG_SITE, 1, 1.0, 0.0, None)]
