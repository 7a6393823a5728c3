"""The references grouped tempered plans (include/gjx_group.h, genjax/_amd/temper.py) are held to.

1. The REPLAY of the header's specification from UNCHANGED oracle entry points (the oracle knows no gjx_group.h): the flat
   terms as tests/plate_ref.py composes them; per grouped site one single-site oracle importance plan that reads the group's
   values from input columns L + s (its log-weight column is the site's log-density at z[s][g]); per group-reading plated
   site one single-site plan that reads the row's data as launch parameters and the row's group values from the same
   columns.  numpy takes the f32 and float64 sums in the header's order; keys are prng.fold_in on the host; the proposals,
   the prior draws of `init` and the uniforms are the oracle's stand-alone sample / bits entry points.
2. A float64 numpy RESTATEMENT of the whole sampler with the same move structure (a scalar phase, then one
   Metropolis-within-Gibbs move per group) on the all-Gaussian random-intercept model, numpy's own generator.
3. The CLOSED FORM of that model: mu, b and a are jointly Gaussian, so Z is a multivariate-normal density of y and the
   posterior is Gaussian."""

import math

import numpy as np
import torch

import plate_ref as P
import temper_ref as R
from genjax._amd import abi, prng, temper
from genjax._amd.ops import KeyBatch

# The end-to-end tolerance (tests/test_gpu_group.py): E2E_FACTOR times the root-mean-square error (bias included) of the float64
# restatement tempered_f64 (below) against the closed form over 24 seeds (default_rng(5000 .. 5023)) on e2e_model(): D = 200,
# G = 8, n = 8192, K = 2, ESS target 0.5 — measured on the CPU with numpy's generator, not on the code under test
# (profiles/group_summary.md; 27 s for the 24 runs): log Z 0.0743 (errors between -0.174 and +0.101, mean -0.005; log Z =
# -168.061).  Posterior-mean errors in posterior standard deviations: mu, b, then a_0 .. a_7.
SPREAD_LOG_Z = 0.0743
SPREAD_MEAN = (0.0157, 0.0132, 0.0097, 0.0122, 0.0162, 0.0114, 0.0123, 0.0097, 0.0135, 0.0111)
E2E_FACTOR = 4.0
E2E_SEEDS = range(5000, 5024)


# ---- the models ----------------------------------------------------------------------------------------------------------------
MODELS = ("intercept", "slope", "gamma", "flat")
SCALARS = {"intercept": 2, "slope": 2, "gamma": 1, "flat": 2}
GROUPED = {"intercept": 1, "slope": 2, "gamma": 1, "flat": 1}


def body(name, G):
    from genjax import gamma, gen, normal

    @gen
    def intercept(xs, g):
        mu = normal(0.0, 2.0) @ "mu"
        b = normal(0.0, 2.0) @ "b"
        a = normal(mu, 0.7).repeat(n=G) @ "a"
        normal(a[g] + b * xs, 0.5) @ "y"

    @gen
    def slope(xs, g):  # S = 2: an intercept plus a slope per group
        mu = normal(0.0, 2.0) @ "mu"
        b = normal(0.0, 2.0) @ "b"
        a = normal(mu, 0.7).repeat(n=G) @ "a"
        c = normal(b, 0.5).repeat(n=G) @ "c"
        normal(a[g] + c[g] * xs, 0.5) @ "y"

    @gen
    def gamma_scale(xs, g):  # a Gamma grouped site: random-walk proposals leave its support
        w = normal(0.0, 2.0) @ "w"
        s = gamma(2.0, 2.0).repeat(n=G) @ "s"
        normal(w * xs, s[g]) @ "y"

    @gen
    def flat(xs, g):  # a flat plated site and a scalar observed site next to the grouped one
        mu = normal(0.0, 2.0) @ "mu"
        normal(mu * xs, 1.5) @ "u"
        b = normal(0.0, 2.0) @ "b"
        a = normal(mu, 0.7).repeat(n=G) @ "a"
        normal(mu + b, 1.0) @ "v"
        normal(a[g] + b * xs, 0.5) @ "y"

    return dict(intercept=intercept, slope=slope, gamma=gamma_scale, flat=flat)[name]


# group sizes drawn from {0, 1, 3, 4, 5, 9}: an empty first group, an empty last group, all rows in one group
LAYOUTS = {1: [9], 2: [5, 4], 5: [0, 3, 1, 9, 0], 17: [4, 0, 1, 5, 3, 9, 0, 0, 1, 4, 3, 5, 9, 1, 0, 4, 3]}


def group_column(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)


def target(name, sizes, seed=0):
    """-> (Target, [xs, ys] as f32 tensors, g int64 tensor, offsets int32 numpy [G + 1])."""
    from genjax import ChoiceMap, Target

    G = len(sizes)
    g = group_column(sizes)
    D = len(g)
    rng = np.random.default_rng(100 * seed + 7 * G + D)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    xs = rng.uniform(-1.0, 1.0, D)
    a = 0.4 + 0.7 * rng.standard_normal(G)
    if name == "gamma":
        ys = 0.7 * xs + rng.gamma(2.0, 0.5, G)[g] * rng.standard_normal(D)
    else:
        ys = a[g] + 0.6 * xs + 0.5 * rng.standard_normal(D)
    con = {"y": f(ys)}
    if name == "flat":
        con.update(u=f(0.3 * xs + 1.5 * rng.standard_normal(D)), v=0.25)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return Target(body(name, G), (f(xs), torch.from_numpy(g)), ChoiceMap.from_mapping(list(con.items()))), g, off


def columns(name, G, n, rng, outside=False):
    """Start columns, float32 numpy: (x: L arrays [n], z: S arrays [G, n]).  `outside`: every fourth value of a Gamma grouped
    component outside its support (negative, zero, NaN)."""
    x = [(1.5 * rng.standard_normal(n)).astype(np.float32) for _ in range(SCALARS[name])]
    z = [(1.5 * rng.standard_normal((G, n))).astype(np.float32) for _ in range(GROUPED[name])]
    if name == "gamma":
        z[0] = rng.gamma(2.0, 0.5, (G, n)).astype(np.float32)
        if outside:
            bad = np.array([-0.5, 0.0, np.nan, -1e-30], dtype=np.float32)
            flat = z[0].reshape(-1)
            flat[::4] = bad[np.arange(len(flat[::4])) % 4]
    return x, z


# ---- 1. the replay ---------------------------------------------------------------------------------------------------------------
def _latent_index(tracer):
    out = {}
    for q, m in enumerate(tracer.meta):
        if m["obs"] is None and not m.get("grouped"):
            out[q] = len(out)
    return out


def _reads_group(s):
    for a in (s.arg[0], s.arg[1]):
        if a.kind == abi.ARG_GROUP:
            return True
        if a.kind == abi.ARG_EXPR and any(o.op == abi.EXPR_GROUP for o in (abi.ExprOp * a.ref).from_address(a.table)):
            return True
    return False


def _arg(a, lat, base, L, keep):
    """An argument for an oracle plan: scalar latents from input columns 0 .. L-1, the group's values from input columns
    L + ref, DATA operands from launch parameters base + column."""
    if a.kind == abi.ARG_GROUP:
        return abi.Arg(abi.ARG_INPUT, L + a.ref, a.scale, a.offset, None)
    if a.kind == abi.ARG_EXPR:
        ops = (abi.ExprOp * a.ref).from_address(a.table)
        prog = [((abi.EXPR_INPUT, lat[o.ref], o.value) if o.op == abi.EXPR_SITE else
                 (abi.EXPR_PARAM, base + o.ref, o.value) if o.op == abi.EXPR_DATA else
                 (abi.EXPR_INPUT, L + o.ref, o.value) if o.op == abi.EXPR_GROUP else (o.op, o.ref, o.value)) for o in ops]
        return abi.expr_arg(prog, keep)
    return P._param_arg(a, lat, base, keep)


def _support(dist, v, term):
    """The header's support rule: -inf outside the OPEN support (a NaN included)."""
    if dist == abi.DIST_GAMMA:
        return np.where(v > 0, term, np.float32(-np.inf))
    if dist == abi.DIST_BETA:
        return np.where((v > 0) & (v < 1), term, np.float32(-np.inf))
    return term


class Assess:
    """assess(x, z) of a lowered grouped model from single-site oracle plans and numpy sums in the header's order."""

    def __init__(self, oracle_ops, tracer, data, offsets, impl=1):
        """`data`: the plan's data columns as float32 numpy arrays of one length D, in column order; `offsets`: int [G + 1]."""
        self.ops, self.impl, self.keep, self._tracer = oracle_ops, impl, [], tracer
        self.data = [np.ascontiguousarray(c, dtype=np.float32) for c in data]
        self.off = np.asarray(offsets, dtype=np.int64)
        self.G = len(self.off) - 1
        self.base = base = len(tracer.params)
        lat = _latent_index(tracer)
        self.L = L = len(lat)
        self.sites = tracer.sites
        # in table order: (kind, plan, dist) with kind in latent / observed / plated / grouped / reader
        self.terms = []
        for q, s in enumerate(tracer.sites):
            c = abi.Site.from_buffer_copy(s)
            c.arg[0], c.arg[1] = _arg(s.arg[0], lat, base, L, self.keep), _arg(s.arg[1], lat, base, L, self.keep)
            c.observed, c.out_col = 1, -1
            if q in lat:
                kind, c.obs = "latent", abi.Arg(abi.ARG_INPUT, lat[q], 1.0, 0.0, None)
            elif s.observed == abi.SITE_GROUPED:
                kind, c.obs = "grouped", abi.Arg(abi.ARG_INPUT, L + sum(k == "grouped" for k, _, _ in self.terms), 1.0, 0.0, None)
            elif s.observed == abi.SITE_PLATED:
                assert s.obs.kind == abi.ARG_DATA
                kind, c.obs = ("reader" if _reads_group(s) else "plated"), abi.Arg(abi.ARG_PARAM, base + s.obs.ref, s.obs.scale, s.obs.offset, None)
            else:
                kind = "observed"
            plan = oracle_ops.plan_create([c])
            if tracer.params and kind in ("latent", "observed", "grouped"):
                plan.set_params(tracer.params)
            self.terms.append((kind, plan, s.dist))
        self.S = sum(k == "grouped" for k, _, _ in self.terms)

    def _logw(self, plan, ins, n):
        kb = prng.split_lazy(prng.key(0, self.impl), n)  # (no latent site: no draw is made)
        return self.ops.importance_run(plan, kb, n, ins, [], want_score=False, want_max_partials=False)[2].numpy().copy()

    @staticmethod
    def _ins(x, zg=()):
        return [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)) for c in list(x) + list(zg)]

    def _row(self, plan, d, ins, n):
        plan.set_params(list(self._tracer.params) + [float(c[d]) for c in self.data])
        return self._logw(plan, ins, n)

    def flat(self, x):
        """-> (lp_flat, ll_flat) float32."""
        n = len(x[0])
        ins = self._ins(x)
        lp, ll = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        l = 0
        with np.errstate(invalid="ignore", over="ignore"):
            for kind, plan, dist in self.terms:
                if kind == "latent":
                    lp = (lp + _support(dist, np.asarray(x[l], dtype=np.float32), self._logw(plan, ins, n))).astype(np.float32)
                    l += 1
                elif kind == "observed":
                    ll = (ll + self._logw(plan, ins, n)).astype(np.float32)
                elif kind == "plated":
                    acc = np.zeros(n, dtype=np.float64)
                    for d in range(len(self.data[0])):
                        acc = acc + self._row(plan, d, ins, n).astype(np.float64)
                    ll = (ll + acc.astype(np.float32)).astype(np.float32)
        return lp, ll

    def lpz(self, x, zg):
        """lpz_g at the group's values zg (S arrays [n]): the f32 sum from +0 over the grouped sites in table order."""
        n = len(x[0])
        ins = self._ins(x, zg)
        out, s = np.zeros(n, dtype=np.float32), 0
        with np.errstate(invalid="ignore", over="ignore"):
            for kind, plan, dist in self.terms:
                if kind == "grouped":
                    out = (out + _support(dist, np.asarray(zg[s], dtype=np.float32), self._logw(plan, ins, n))).astype(np.float32)
                    s += 1
        return out

    def acc(self, x, zg, g):
        """acc_g at the group's values zg: the float64 sum over the rows of group g, in order, and within a row over the
        group-reading sites in table order."""
        n = len(x[0])
        ins = self._ins(x, zg)
        out = np.zeros(n, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            for d in range(int(self.off[g]), int(self.off[g + 1])):
                for kind, plan, _ in self.terms:
                    if kind == "reader":
                        out = out + self._row(plan, d, ins, n).astype(np.float64)
        return out

    def sums(self, x, z):
        """-> (LZ, A) float64: the sums over the groups in order."""
        n = len(x[0])
        LZ, A = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            for g in range(self.G):
                zg = [c[g] for c in z]
                LZ = LZ + self.lpz(x, zg).astype(np.float64)
                A = A + self.acc(x, zg, g)
        return LZ, A

    @staticmethod
    def total(flat, s):
        with np.errstate(invalid="ignore", over="ignore"):
            return (flat + s.astype(np.float32)).astype(np.float32)

    def __call__(self, x, z):
        lpf, llf = self.flat(x)
        LZ, A = self.sums(x, z)
        return self.total(lpf, LZ), self.total(llf, A)


def _arg_value(a, x, lat, params, n):
    """The f32 value of a grouped site's argument at the particles' scalars: a literal, a parameter or an affine read of a
    scalar latent (multiply, then add: one rounding each)."""
    if a.kind == abi.ARG_CONST:
        return float(np.float32(a.offset))
    if a.kind == abi.ARG_PARAM:
        return float(np.float32(np.float32(a.scale) * np.float32(params[a.ref]) + np.float32(a.offset)))
    assert a.kind == abi.ARG_SITE, a.kind
    v = (np.float32(a.scale) * np.asarray(x[lat[a.ref]], dtype=np.float32)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray((v + np.float32(a.offset)).astype(np.float32)))


def init_ref(oracle_ops, tracer, init_key, x, G):
    """The prior draws of `init`: z[s][g] = the oracle's gjx_sample_logpdf_<dist> over the lazy children of
    fold_in(init_key, g) with fold s + 1 (THREEFRY) / s (PHILOX), at the site's arguments evaluated at x."""
    lat = _latent_index(tracer)
    n = len(x[0])
    sites = [s for s in tracer.sites if s.observed == abi.SITE_GROUPED]
    names = {abi.DIST_NORMAL: "normal", abi.DIST_GAMMA: "gamma", abi.DIST_BETA: "beta"}
    z = [np.empty((G, n), dtype=np.float32) for _ in sites]
    for g in range(G):
        kg = prng.fold_in(init_key, g)
        for s, st in enumerate(sites):
            kb = KeyBatch(init_key.impl, 1, parent=(kg.k0, kg.k1), first=0, fold=(s + 1 if init_key.impl == 0 else s), parent_lane=kg.lane)
            a0, a1 = (_arg_value(st.arg[k], x, lat, tracer.params, n) for k in range(2))
            z[s][g] = oracle_ops.sample_logpdf(names[st.dist], kb, n, a0, a1, want_score=False)[0].numpy()
    return z


def move_ref(oracle_ops, assess, key, x, z, lp, ll, beta, n_moves, scales, z_scales, ancestors=None, recompute=False, init_key=None,
             stats=None):
    """gjx_temper_move_grouped from oracle pieces.  x: L float32 numpy columns; z: S arrays [G, n] (None with init_key);
    z_scales: [S, G].  -> (x, z, lp, ll, n_accept, n_accept_z), numpy.  `stats` (a dict): group proposals whose lpz' is -inf
    are counted into stats["outside"]."""
    n, L, S, G = len(x[0]), len(x), assess.S, assess.G
    a = np.arange(n) if ancestors is None else np.minimum(np.asarray(ancestors).astype(np.int64) & 0xFFFFFFFF, n - 1)
    x = [np.asarray(c, dtype=np.float32)[a] for c in x]
    if init_key is not None:
        z = init_ref(oracle_ops, assess._tracer, init_key, x, G)
    else:
        z = [np.asarray(c, dtype=np.float32)[:, a] for c in z]
    if recompute:
        lp, ll = assess(x, z)
    else:
        lp, ll = np.asarray(lp, dtype=np.float32)[a], np.asarray(ll, dtype=np.float32)[a]
    lp, ll = lp.copy(), ll.copy()
    beta = np.float32(beta)
    acc_n, acc_z = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    impl = key.impl

    def logu(k):
        bits = oracle_ops.rng_bits(KeyBatch(impl, 1, parent=(k.k0, k.k1), first=0, parent_lane=k.lane), n, 0)
        u = torch.from_numpy(R.uniform01(bits.numpy()).copy())
        return oracle_ops.logpdf("bernoulli", n, 1, u).numpy()

    def propose(k, cols, sc):
        out = []
        for l, c in enumerate(cols):
            kb = KeyBatch(impl, 1, parent=(k.k0, k.k1), first=0, fold=(l + 1 if impl == 0 else l), parent_lane=k.lane)
            out.append(oracle_ops.sample_logpdf("normal", kb, n, torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)),
                                                float(np.float32(sc[l])), want_score=False)[0].numpy().copy())
        return out

    if n_moves:
        lpf, llf = assess.flat(x)
    for r in range(int(n_moves)):
        kr = prng.fold_in(key, r)
        # the scalar phase: the rule of gjx_temper.h with the full assess of (x', z)
        y = propose(prng.fold_in(kr, 0), x, scales)
        lpfn, llfn = assess.flat(y)
        LZn, An = assess.sums(y, z)
        lpn, lln = assess.total(lpfn, LZn), assess.total(llfn, An)
        lg = logu(prng.fold_in(kr, 1))
        with np.errstate(invalid="ignore", over="ignore"):
            h = (lp + (beta * ll).astype(np.float32)).astype(np.float32)
            hn = (lpn + (beta * lln).astype(np.float32)).astype(np.float32)
            d = (hn - h).astype(np.float32)
            ok = (d >= np.float32(0.0)) | (lg < d)
        x = [np.where(ok, y[l], x[l]) for l in range(L)]
        lpf, llf = np.where(ok, lpfn, lpf), np.where(ok, llfn, llf)
        acc_n += ok.astype(np.int32)
        # the group phase
        kz = prng.fold_in(kr, 2)
        LZ, A = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
        for g in range(G):
            kg = prng.fold_in(kz, g)
            zg = [c[g].copy() for c in z]
            zy = propose(prng.fold_in(kg, 0), zg, [z_scales[s][g] for s in range(S)])
            lz, lzn = assess.lpz(x, zg), assess.lpz(x, zy)
            ac, acn = assess.acc(x, zg, g), assess.acc(x, zy, g)
            if stats is not None:
                stats["outside"] = stats.get("outside", 0) + int(np.isneginf(lzn).sum())
            lg = logu(prng.fold_in(kg, 1))
            with np.errstate(invalid="ignore", over="ignore"):
                dz = (lzn - lz).astype(np.float32)
                da = (acn - ac).astype(np.float32)
                d = (dz + (beta * da).astype(np.float32)).astype(np.float32)
                ok = (d >= np.float32(0.0)) | (lg < d)
                for s in range(S):
                    z[s][g] = np.where(ok, zy[s], zg[s])
                acc_z += ok.astype(np.int32)
                LZ = LZ + np.where(ok, lzn, lz).astype(np.float64)
                A = A + np.where(ok, acn, ac)
        lp, ll = assess.total(lpf, LZ), assess.total(llf, A)
    return x, z, lp, ll, acc_n, acc_z


# ---- 3. the closed form of the random-intercept model -----------------------------------------------------------------------------
class Intercepts:
    """mu ~ N(0, s_mu), b ~ N(0, s_b), a_g ~ N(mu, tau), y_d ~ N(a[g_d] + b x_d, noise): theta = (mu, b, a_0 .. a_{G-1}) is
    jointly Gaussian with y, so log Z is a multivariate-normal density of y and the posterior of theta is Gaussian."""

    def __init__(self, xs, g, ys, G, s_mu=2.0, s_b=2.0, tau=0.7, noise=0.5):
        self.xs, self.g, self.ys = (np.asarray(v) for v in (xs, g, ys))
        self.xs, self.ys = self.xs.astype(np.float64), self.ys.astype(np.float64)
        self.G, self.D = G, len(self.ys)
        self.s_mu, self.s_b, self.tau, self.noise = (float(np.float32(v)) for v in (s_mu, s_b, tau, noise))
        self.off = np.concatenate([[0], np.cumsum(np.bincount(self.g, minlength=G))])
        # theta = M (mu, b, eta): a = mu + tau eta
        M = np.zeros((2 + G, 2 + G))
        M[0, 0], M[1, 1] = self.s_mu, self.s_b
        M[2:, 0], M[2:, 2:] = self.s_mu, self.tau * np.eye(G)
        cov = M @ M.T
        H = np.zeros((self.D, 2 + G))
        H[:, 1] = self.xs
        H[np.arange(self.D), 2 + self.g] = 1.0
        C = self.noise ** 2 * np.eye(self.D) + H @ cov @ H.T
        _, logdet = np.linalg.slogdet(C)
        self.log_z = float(-0.5 * (self.D * math.log(2 * math.pi) + logdet + self.ys @ np.linalg.solve(C, self.ys)))
        K = cov @ H.T
        self.post_mean = K @ np.linalg.solve(C, self.ys)
        self.post_cov = cov - K @ np.linalg.solve(C, K.T)
        self.post_sd = np.sqrt(np.diag(self.post_cov))

    @staticmethod
    def _ln(v, loc, sd):
        return -0.5 * ((v - loc) / sd) ** 2 - (0.5 * math.log(2 * math.pi) + math.log(sd))

    def lp_flat(self, mu, b):
        return self._ln(mu, 0.0, self.s_mu) + self._ln(b, 0.0, self.s_b)

    def lpz(self, mu, ag):
        return self._ln(ag, mu, self.tau)

    def acc(self, b, ag, k):
        rows = slice(self.off[k], self.off[k + 1])
        return self._ln(self.ys[None, rows], ag[:, None] + b[:, None] * self.xs[None, rows], self.noise).sum(axis=1)

    def assess(self, mu, b, a):
        """a: [G, n] -> (lp, ll) float64."""
        lp = self.lp_flat(mu, b) + sum(self.lpz(mu, a[k]) for k in range(self.G))
        return lp, sum(self.acc(b, a[k], k) for k in range(self.G))


def e2e_model(D=200, G=8, seed=0):
    """The model of the end-to-end test: sorted groups of unequal sizes, f32 data (the closed form is taken at these numbers)."""
    rng = np.random.default_rng(seed)
    g = np.sort(rng.integers(0, G, D))
    xs = rng.uniform(-1.0, 1.0, D).astype(np.float32)
    a = 0.4 + 0.7 * rng.standard_normal(G)
    ys = (a[g] + 0.6 * xs + 0.5 * rng.standard_normal(D)).astype(np.float32)
    return Intercepts(xs, g, ys, G)


# ---- 2. the float64 restatement ---------------------------------------------------------------------------------------------------
def tempered_f64(model: Intercepts, n, n_moves, ess_target, rng):
    """The grouped sampler of genjax/_amd/temper.py in float64 numpy: the schedule rule (temper.next_beta), systematic
    resampling, 2.38 / sqrt(L) weighted-deviation scales for the scalars and 2.38 / sqrt(S) for every group's component, per
    sweep a scalar phase (both scalars at once, the full assess) and then one Metropolis-within-Gibbs move per group against
    the group's own rows; the last stage moved too.  -> dict(log_z, betas, mu, b, a [G, n])."""
    G = model.G
    mu, b = model.s_mu * rng.standard_normal(n), model.s_b * rng.standard_normal(n)
    a = mu[None, :] + model.tau * rng.standard_normal((G, n))
    lp, ll = model.assess(mu, b, a)
    beta, out_betas, log_z = 0.0, [0.0], 0.0

    def ess_fn(deltas):
        s1, s2, _ = R.ladder_ref(ll, deltas)
        return temper.ess_of(s1, s2)

    def wsd(cols, wt):  # the weighted standard deviation along the last axis
        mean = (cols * wt).sum(axis=-1, keepdims=True)
        return np.sqrt((((cols - mean) ** 2) * wt).sum(axis=-1))

    while beta < 1.0:
        nb = temper.next_beta(beta, ess_target * n, ess_fn)[0]
        lw = (nb - beta) * ll
        mx = lw.max()
        wt = np.exp(lw - mx)
        log_z += mx + math.log(wt.sum()) - math.log(n)
        wt /= wt.sum()
        sc = 2.38 / math.sqrt(2.0) * wsd(np.stack([mu, b]), wt)
        zsc = 2.38 / math.sqrt(1.0) * wsd(a, wt)
        k = R.systematic(rng, wt)
        mu, b, a, lp, ll = mu[k], b[k], a[:, k], lp[k], ll[k]
        for _ in range(n_moves):
            mun, bn = mu + sc[0] * rng.standard_normal(n), b + sc[1] * rng.standard_normal(n)
            lpn, lln = model.assess(mun, bn, a)
            d = (lpn + nb * lln) - (lp + nb * ll)
            ok = (d >= 0.0) | (np.log(rng.random(n)) < d)
            mu, b = np.where(ok, mun, mu), np.where(ok, bn, b)
            LZ, A = np.zeros(n), np.zeros(n)
            for g in range(G):
                an = a[g] + zsc[g] * rng.standard_normal(n)
                lz, lzn = model.lpz(mu, a[g]), model.lpz(mu, an)
                ac, acn = model.acc(b, a[g], g), model.acc(b, an, g)
                d = (lzn - lz) + nb * (acn - ac)
                ok = (d >= 0.0) | (np.log(rng.random(n)) < d)
                a[g] = np.where(ok, an, a[g])
                LZ, A = LZ + np.where(ok, lzn, lz), A + np.where(ok, acn, ac)
            lp, ll = model.lp_flat(mu, b) + LZ, A
        beta = nb
        out_betas.append(nb)
    return dict(log_z=log_z, betas=out_betas, mu=mu, b=b, a=a)


def restatement_errors(model: Intercepts, n, n_moves, seeds):
    """-> (log Z errors [seeds], posterior-mean errors [seeds, 2 + G] in posterior standard deviations) of tempered_f64."""
    ez, em = [], []
    for s in seeds:
        r = tempered_f64(model, n, n_moves, 0.5, np.random.default_rng(s))
        ez.append(r["log_z"] - model.log_z)
        means = np.concatenate([[r["mu"].mean(), r["b"].mean()], r["a"].mean(axis=1)])
        em.append((means - model.post_mean) / model.post_sd)
    return np.asarray(ez), np.asarray(em)
