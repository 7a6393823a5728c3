"""References of include/gjx_group_cov.h: the per-group weighted covariance and its Cholesky factor in two-pass float64 numpy,
the standard-Normal draws of a proposal key from the oracle's entry point, and the proposal z' = z + F eps replayed in f32 with
one rounding per product and per sum."""

import math

import numpy as np
import torch

from genjax._amd.ops import KeyBatch


def tri(s, j):
    return s * (s + 1) // 2 + j


def inputs(S, G, n, seed, weighted):
    """-> (z: S arrays f32 [G, n], lw f32 [n] or None).  Every group's covariance has condition number <= 1e4 (singular values
    of its mixing matrix within 1 .. 100 times a random size), its means are up to 1e3 times its deviations.  lw: multiples of
    2^-10 in (-8, 0], so that f32(lw_i - m_b) is exact and a weight differs from the float64 exponential by the f32 exp's own
    rounding alone; from n = 255 on, a tenth of the entries -inf and one NaN (never entry 0)."""
    rng = np.random.default_rng(seed)
    z = np.empty((S, G, n), dtype=np.float32)
    for g in range(G):
        q, _ = np.linalg.qr(rng.normal(size=(S, S)))
        size = 10.0 ** rng.uniform(-2, 1)
        mix = q @ np.diag(size * 10.0 ** rng.uniform(0, 2, S))
        z[:, g, :] = (mix @ rng.normal(size=(S, n)) + (size * 1e3 * rng.uniform(-1, 1, S))[:, None]).astype(np.float32)
    if not weighted:
        return list(z), None
    lw = (-np.floor(rng.uniform(0, 8, n) * 1024) / 1024).astype(np.float32)
    if n >= 255:
        holes = 1 + rng.permutation(n - 1)[:n // 10]
        lw[holes] = -np.inf
        lw[holes[0]] = np.nan
    return list(z), lw


def moments_ref(z, lw):
    """-> (factor f64 [G, S, S] lower-triangular: 2.38 / sqrt(S) times the Cholesky factor of every group's weighted covariance;
    scales f64 [S, G]).  Two passes, centred, float64; a group whose covariance is zero throughout (n = 1) gets zeros."""
    z = np.stack([np.asarray(c, dtype=np.float64) for c in z])
    S, G, n = z.shape
    w = np.ones(n)
    if lw is not None:
        lw = np.asarray(lw, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            ok = lw > -np.inf
        w = np.where(ok, np.exp(np.where(ok, lw, 0.0) - lw[ok].max()), 0.0)
    c = 2.38 / math.sqrt(S)
    factor, scales = np.zeros((G, S, S)), np.zeros((S, G))
    for g in range(G):
        cols = z[:, g, w > 0]
        dev = cols - ((cols * w[w > 0]).sum(axis=1) / w.sum())[:, None]
        cov = (dev * w[w > 0]) @ dev.T / w.sum()
        scales[:, g] = c * np.sqrt(np.diag(cov))
        if cov.any():
            factor[g] = c * np.linalg.cholesky(cov)
    return factor, scales


def draws(oracle_ops, pkey, count, n):
    """eps_s, s = 0 .. count-1: element i of the standard-Normal batch of the proposal key `pkey` with fold s + 1 (THREEFRY) /
    s (PHILOX) — the draws of tests/group_ref.py move_ref at loc 0, scale 1."""
    zero = torch.zeros(n, dtype=torch.float32)
    out = []
    for s in range(count):
        kb = KeyBatch(pkey.impl, 1, parent=(pkey.k0, pkey.k1), first=0, fold=(s + 1 if pkey.impl == 0 else s), parent_lane=pkey.lane)
        out.append(oracle_ops.sample_logpdf("normal", kb, n, zero, 1.0, want_score=False)[0].numpy().copy())
    return out


def propose(cur, F, eps):
    """cur: S f32 arrays [n]; F: packed f32 triangle; eps: S f32 arrays -> z'_s = f32(z_s + t_s), t_s = f32(F[s][0] * eps_0), then
    t_s = f32(t_s + f32(F[s][j] * eps_j)) for j = 1 .. s in order."""
    F = np.asarray(F, dtype=np.float32)
    out = []
    for s in range(len(cur)):
        t = (F[tri(s, 0)] * eps[0]).astype(np.float32)
        for j in range(1, s + 1):
            t = (t + (F[tri(s, j)] * eps[j]).astype(np.float32)).astype(np.float32)
        out.append((np.asarray(cur[s], dtype=np.float32) + t).astype(np.float32))
    return out


# ---- the intercept-and-slope model: closed form and the float64 restatement of the block sampler ---------------------------------
class Slopes:
    """mu ~ N(0, 2), b ~ N(0, 2), a_g ~ N(mu, 0.7), c_g ~ N(b, 0.5), y_d ~ N(a[g_d] + c[g_d] x_d, 0.5) (group_ref.body("slope")):
    theta = (mu, b, a_0 .. a_{G-1}, c_0 .. c_{G-1}) is jointly Gaussian with y — log Z and the posterior in closed form."""
    s_mu, s_b, tau, ups, noise = 2.0, 2.0, float(np.float32(0.7)), 0.5, 0.5

    def __init__(self, xs, g, ys, G):
        self.xs, self.ys, self.g, self.G, self.D = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64), np.asarray(g), G, len(ys)
        self.off = np.concatenate([[0], np.cumsum(np.bincount(self.g, minlength=G))])
        M = np.zeros((2 + 2 * G, 2 + 2 * G))  # theta = M (standard normals)
        M[0, 0], M[1, 1] = self.s_mu, self.s_b
        M[2:2 + G, 0], M[2 + G:, 1] = self.s_mu, self.s_b
        M[2:2 + G, 2:2 + G], M[2 + G:, 2 + G:] = self.tau * np.eye(G), self.ups * np.eye(G)
        cov = M @ M.T
        H = np.zeros((self.D, 2 + 2 * G))
        H[np.arange(self.D), 2 + self.g], H[np.arange(self.D), 2 + G + self.g] = 1.0, self.xs
        C = self.noise ** 2 * np.eye(self.D) + H @ cov @ H.T
        self.log_z = float(-0.5 * (self.D * math.log(2 * math.pi) + np.linalg.slogdet(C)[1] + self.ys @ np.linalg.solve(C, self.ys)))
        K = cov @ H.T
        self.post_mean, self.post_cov = K @ np.linalg.solve(C, self.ys), cov - K @ np.linalg.solve(C, K.T)
        self.post_sd = np.sqrt(np.diag(self.post_cov))

    @staticmethod
    def _ln(v, loc, sd):
        return -0.5 * ((v - loc) / sd) ** 2 - (0.5 * math.log(2 * math.pi) + math.log(sd))

    def lp_flat(self, mu, b):
        return self._ln(mu, 0.0, self.s_mu) + self._ln(b, 0.0, self.s_b)

    def lpz(self, mu, b, ag, cg):
        return self._ln(ag, mu, self.tau) + self._ln(cg, b, self.ups)

    def acc(self, ag, cg, k):
        rows = slice(self.off[k], self.off[k + 1])
        return self._ln(self.ys[None, rows], ag[:, None] + cg[:, None] * self.xs[None, rows], self.noise).sum(axis=1)


def e2e_model(D=200, G=8, seed=0):
    """The model of the end-to-end test: x in [2, 3] (not centred), sorted groups of unequal sizes, f32 data."""
    rng = np.random.default_rng(seed)
    g = np.sort(rng.integers(0, G, D))
    xs = rng.uniform(2.0, 3.0, D).astype(np.float32)
    a, c = 0.4 + 0.7 * rng.standard_normal(G), 0.6 + 0.5 * rng.standard_normal(G)
    return Slopes(xs, g, (a[g] + c[g] * xs + 0.5 * rng.standard_normal(D)).astype(np.float32), G)


def tempered_block_f64(model: Slopes, n, n_moves, ess_target, rng, proposal="block"):
    """group_ref.tempered_f64 on the intercept-and-slope model with the block proposal of genjax/_amd/temper.py, in float64 numpy:
    per stage, 2.38 / sqrt(2) times the Cholesky factor of the weighted covariance of (mu, b) and, per group, of (a_g, c_g) —
    both of the population BEFORE resampling; `proposal="diagonal"` keeps the diagonals of those covariances alone (the
    diagonal route).  -> dict(log_z, mu, b, a, c, accept_groups [one rate per stage])."""
    import temper_ref as R
    from genjax._amd import temper

    G, c238 = model.G, 2.38 / math.sqrt(2.0)
    mu, b = model.s_mu * rng.standard_normal(n), model.s_b * rng.standard_normal(n)
    a, c = mu + model.tau * rng.standard_normal((G, n)), b + model.ups * rng.standard_normal((G, n))

    def sums(mu, b):  # LZ and A of the state: per group, then summed
        lz = [model.lpz(mu, b, a[k], c[k]) for k in range(G)]
        return sum(lz), sum(model.acc(a[k], c[k], k) for k in range(G))

    def factor(cols, wt):
        dev = cols - (cols * wt).sum(axis=1, keepdims=True)
        cov = (dev * wt) @ dev.T
        return c238 * (np.linalg.cholesky(cov) if proposal == "block" else np.diag(np.sqrt(np.diag(cov))))

    LZ, ll = sums(mu, b)
    lp = model.lp_flat(mu, b) + LZ
    beta, log_z, rates = 0.0, 0.0, []
    while beta < 1.0:
        nb = temper.next_beta(beta, ess_target * n, lambda d: temper.ess_of(*R.ladder_ref(ll, d)[:2]))[0]
        lw = (nb - beta) * ll
        wt = np.exp(lw - lw.max())
        log_z += lw.max() + math.log(wt.sum()) - math.log(n)
        wt /= wt.sum()
        Fx, Fz = factor(np.stack([mu, b]), wt), [factor(np.stack([a[k], c[k]]), wt) for k in range(G)]
        k = R.systematic(rng, wt)
        mu, b, a, c, lp, ll = mu[k], b[k], a[:, k], c[:, k], lp[k], ll[k]
        moved = 0
        for _ in range(n_moves):
            e = rng.standard_normal((2, n))
            mun, bn = mu + Fx[0, 0] * e[0], b + Fx[1, 0] * e[0] + Fx[1, 1] * e[1]
            LZn, _ = sums(mun, bn)  # (the likelihood does not read the scalars)
            d = (model.lp_flat(mun, bn) + LZn) - lp
            ok = (d >= 0.0) | (np.log(rng.random(n)) < d)
            mu, b = np.where(ok, mun, mu), np.where(ok, bn, b)
            LZ, A = np.zeros(n), np.zeros(n)
            for g in range(G):
                e = rng.standard_normal((2, n))
                an, cn = a[g] + Fz[g][0, 0] * e[0], c[g] + Fz[g][1, 0] * e[0] + Fz[g][1, 1] * e[1]
                lz, lzn, ac, acn = model.lpz(mu, b, a[g], c[g]), model.lpz(mu, b, an, cn), model.acc(a[g], c[g], g), model.acc(an, cn, g)
                d = (lzn - lz) + nb * (acn - ac)
                ok = (d >= 0.0) | (np.log(rng.random(n)) < d)
                a[g], c[g] = np.where(ok, an, a[g]), np.where(ok, cn, c[g])
                LZ, A, moved = LZ + np.where(ok, lzn, lz), A + np.where(ok, acn, ac), moved + int(ok.sum())
            lp, ll = model.lp_flat(mu, b) + LZ, A
        rates.append(moved / (n * n_moves * G))
        beta = nb
    return dict(log_z=log_z, mu=mu, b=b, a=a, c=c, accept_groups=rates)


def e2e_errors(model, log_z, mu, b, a, c, last_rate):
    """-> (log Z error; posterior-mean errors [2 + 2 G] in posterior deviations; variance ratios of a_g, c_g [2 G]; the last
    stage's group accept rate) of one run, float64 numpy columns."""
    means = np.concatenate([[mu.mean(), b.mean()], a.mean(axis=1), c.mean(axis=1)])
    ratios = np.concatenate([a.var(axis=1), c.var(axis=1)]) / model.post_sd[2:] ** 2
    return log_z - model.log_z, (means - model.post_mean) / model.post_sd, ratios, last_rate


def restatement_errors(model, seeds, proposal="block", n=4096, n_moves=2):
    """e2e_errors of tempered_block_f64 over `seeds` (default_rng(seed)), stacked per quantity."""
    out = []
    for s in seeds:
        r = tempered_block_f64(model, n, n_moves, 0.5, np.random.default_rng(s), proposal)
        out.append(e2e_errors(model, r["log_z"], r["mu"], r["b"], r["a"], r["c"], r["accept_groups"][-1]))
    return tuple(np.asarray(v) for v in zip(*out))


# The restatement on e2e_model() at n = 4096, K = 2, ESS target 0.5 over the 24 seeds default_rng(6000 .. 6023) — measured on
# the CPU with numpy's generator, not on the code under test (profiles/group_cov_summary.md; 19 s; log Z = -171.5919; the
# posterior correlation of (a_g, c_g) is -0.980 .. -0.987).  Root-mean-square errors, bias included:
E2E_SEEDS, E2E_FACTOR = range(6000, 6024), 4.0
RMS_LOG_Z = 0.6596         # errors -1.777 .. +0.731, mean -0.260
RMS_MEAN = (0.2117, 0.1611, 0.1195, 0.1237, 0.1216, 0.1220, 0.1179, 0.1187, 0.1214, 0.1114,   # mu, b, a_0 .. a_7
            0.1174, 0.1229, 0.1187, 0.1204, 0.1164, 0.1182, 0.1203, 0.1109)                    # c_0 .. c_7, in posterior deviations
RMS_VAR_RATIO = (0.0435, 0.0487, 0.0435, 0.0448, 0.0479, 0.0474, 0.0489, 0.0446,             # a_0 .. a_7: of (ratio - 1)
                 0.0419, 0.0466, 0.0419, 0.0428, 0.0465, 0.0479, 0.0487, 0.0432)             # c_0 .. c_7 (ratios 0.886 .. 1.140)
MIN_LAST_RATE = 0.3255     # the last stage's group accept rate: 0.3256 / 0.3357 / 0.3415 (min / mean / max); the floor is half of it


# ---- what the GPU suite shares ------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


_SLOPE = []  # (the plan and the replay's assess, made once)


def slope_case(hip_ops, oracle_ops, seed, n=300):
    """The slope plan over group_ref.LAYOUTS[17] (empty groups) with parameters, data and groups set, and start columns with a
    permuted ancestors column -> (plan, rng, x, z, lp, ll, ancestors), numpy but for the plan."""
    import group_ref as GR
    from genjax._amd import temper
    from genjax._amd.runtime import use_ops

    if not _SLOPE:
        with use_ops(hip_ops):
            target, _, off = GR.target("slope", GR.LAYOUTS[17], seed=1)
            tracer = temper.lower(target, 64)
            plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            if tracer.params:
                plan.set_params(tracer.params)
            plan.set_data(tracer.data_columns(hip_ops.device()))
            plan.set_groups(tracer.group_offsets().to(hip_ops.device()))
        _SLOPE.extend([plan, GR.Assess(oracle_ops, tracer, [t.detach().to(torch.float32).numpy().copy() for t in tracer.data], off)])
    plan, assess = _SLOPE
    rng = np.random.default_rng(seed)
    x, z = GR.columns("slope", 17, n, rng)
    lp, ll = assess(x, z)
    return plan, rng, x, z, lp, ll, rng.permutation(n).astype(np.int32)
