"""The tempered lowering held to float64 without a GPU (tests/temper_fuzz.py): random bodies and the fixed `interleaved` body
are lowered on the oracle backend, replayed (plate_ref.Assess / temper_ref.Assess / pointwise_ref.terms) and compared with the
float64 evaluation of their own source text; five mutations of the tracer's table must each FAIL that comparison; stage 0 of
`interleaved` drawn from temper.prior_table has the conditional law the source text states; and the float64 restatement of
the sampler recovers the closed form of the two-plate regression the GPU suite runs end to end."""

import numpy as np
import pytest
import torch

import plate_ref as P
import pointwise_ref as W
import temper_fuzz as F
import temper_ref as R
from genjax._amd import abi, prng, temper
from genjax._amd.plan import PlanUnsupported, _make_plan
from genjax._amd.runtime import use_ops

SEEDS = (11, 12, 13, 14)
PER_SEED = 50
MAX_DROPPED, MAX_UNLOWERED = 0.10, 0.15  # shares of the generated cases


def _assess(oracle_ops, table, data):
    return P.Assess(oracle_ops, table, data) if data else R.Assess(oracle_ops, table)


def _compare(oracle_ops, tracer, src, latents, obs, args, ref, D=None, context=""):
    """lp, ll and (plated bodies) the pointwise terms of the replay against float64 -> the largest err / tol."""
    assess = _assess(oracle_ops, tracer, F.data_of(tracer, D))
    cols = F.columns_of(tracer, latents)
    lp, ll = assess(cols)
    worst = max(F.check64(lp, what="lp", ref=ref, context=context), F.check64(ll, what="ll", ref=ref, context=context))
    if tracer.data:
        worst = max(worst, F.check64(W.terms(assess, cols), what="terms", ref=ref, context=context))
    return worst


def test_random_bodies(oracle_ops):
    """200 random bodies (4 seeds x 50; n = 64, D in {2, 5, 9}; every fourth case with every fourth Gamma / Beta latent value
    outside its support): lp, ll and the pointwise terms of the replay within the derived tolerance of float64.  At most 10 % of
    the cases may be dropped for conditioning and at most 15 % may fail to lower."""
    n, compared, unlowered, dropped, worst = 64, 0, [], [], 0.0
    with use_ops(oracle_ops):
        for seed in SEEDS:
            rng = np.random.default_rng(seed)
            for i in range(PER_SEED):
                D, outside = (2, 5, 9)[i % 3], i % 4 == 3
                src, sites = F.random_tempered_model(rng)
                args, obs = F.random_inputs(rng, sites, D)
                latents = F.latent_columns(rng, sites, n, outside=outside)
                try:
                    tracer = temper.lower(F.target_of(src, args, obs), n)
                except PlanUnsupported as e:
                    unlowered.append(f"seed {seed} case {i}: {e}")
                    continue
                assert [m["addr"] for m in tracer.meta] == [s[0] for s in sites]
                ref = F.Reference(src, latents, obs, args, live=F.inside(sites, latents))
                if not ref.kept:
                    dropped.append(f"seed {seed} case {i}: {'; '.join(ref.reasons)}")
                    continue
                worst = max(worst, _compare(oracle_ops, tracer, src, latents, obs, args, ref,
                                            context=f"seed {seed} case {i} D {D} outside {outside}\n{src}\nargs {args[3:]} observed {obs}"))
                compared += 1
    total = len(SEEDS) * PER_SEED
    print(f"compared {compared}, unlowered {len(unlowered)} ({len(unlowered) / total:.3f}, cap {MAX_UNLOWERED}), dropped {len(dropped)} "
          f"({len(dropped) / total:.3f}, cap {MAX_DROPPED}); worst err / tol {worst:.3f}")
    for r in unlowered + dropped:
        print("  ", r)
    assert len(unlowered) <= MAX_UNLOWERED * total and len(dropped) <= MAX_DROPPED * total
    assert compared + len(unlowered) + len(dropped) == total


# ---- the interleaved body -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interleaved(oracle_ops):
    n, D = 257, 65
    rng = np.random.default_rng(77)
    args, obs = F.random_inputs(rng, F.INTERLEAVED_SITES, D)
    latents = F.latent_columns(rng, F.INTERLEAVED_SITES, n)
    with use_ops(oracle_ops):
        tracer = temper.lower(F.target_of(F.INTERLEAVED, args, obs), n)
    return dict(n=n, D=D, args=args, obs=obs, latents=latents, tracer=tracer, ref=F.Reference(F.INTERLEAVED, latents, obs, args))


def test_interleaved_lowers_whole(interleaved):
    """Nine sites, the last one included: a plated Beta whose second shape reads the VALUE of an earlier plate as data."""
    tr = interleaved["tracer"]
    assert [m["addr"] for m in tr.meta] == [s[0] for s in F.INTERLEAVED_SITES]
    assert [s.observed for s in tr.sites] == [0, abi.SITE_PLATED, 0, 1, 0, abi.SITE_PLATED, 0, abi.SITE_PLATED, abi.SITE_PLATED]
    assert [s.dist for s in tr.sites][5:] == [abi.DIST_GAMMA, abi.DIST_BETA, abi.DIST_BERNOULLI, abi.DIST_BETA]
    assert interleaved["ref"].kept, interleaved["ref"].reasons


def test_interleaved(oracle_ops, interleaved):
    c = interleaved
    worst = _compare(oracle_ops, c["tracer"], F.INTERLEAVED, c["latents"], c["obs"], c["args"], c["ref"])
    print(f"interleaved, n = {c['n']}, D = {c['D']}: worst err / tol {worst:.3f}; f32 floors {c['ref'].floor}")


def test_interleaved_outside_support(oracle_ops, interleaved):
    c = interleaved
    latents = F.latent_columns(np.random.default_rng(78), F.INTERLEAVED_SITES, c["n"], outside=True)
    ok = F.inside(F.INTERLEAVED_SITES, latents)
    ref = F.Reference(F.INTERLEAVED, latents, c["obs"], c["args"], live=ok)
    assert ref.kept, ref.reasons
    assert np.all(np.isneginf(ref.ref["lp"][~ok]) | np.isnan(ref.ref["lp"][~ok])) and np.isneginf(ref.ref["lp"]).sum() >= c["n"] // 8
    worst = _compare(oracle_ops, c["tracer"], F.INTERLEAVED, latents, c["obs"], c["args"], ref)
    print(f"interleaved, latents outside their support: worst err / tol {worst:.3f}")


class _Table:
    """What the replays read of a tracer, over a MUTATED copy of its site table (the product is not touched)."""

    def __init__(self, tracer):
        self.sites = [abi.Site.from_buffer_copy(s) for s in tracer.sites]
        self.meta, self.params, self.keep, self._tracer = list(tracer.meta), tracer.params, [], tracer


def _prog(a):
    return [(o.op, o.ref, o.value) for o in (abi.ExprOp * a.ref).from_address(a.table)]


def _map_progs(table, fn, sites=None):
    """Every program argument of `sites` rebuilt from fn(program)."""
    for s in table.sites if sites is None else sites:
        for k in range(2):
            if s.arg[k].kind == abi.ARG_EXPR:
                s.arg[k] = abi.expr_arg(fn(_prog(s.arg[k])), table.keep)


def _mutate(tracer, which, args):
    t = _Table(tracer)
    q = {m["addr"]: i for i, m in enumerate(tracer.meta)}
    if which == "swap_args":            # (a) arg[0] / arg[1] of the plated Gamma
        s = t.sites[q["y2"]]
        a0, a1 = abi.Arg.from_buffer_copy(s.arg[0]), abi.Arg.from_buffer_copy(s.arg[1])
        s.arg[0], s.arg[1] = a1, a0
    elif which == "wrong_latent":       # (b) b's ARG_SITE reference to `a` points at `g`
        a = t.sites[q["b"]].arg[0]
        assert a.kind == abi.ARG_SITE and a.ref == q["a"]
        a.ref = q["g"]
    elif which == "swap_columns":       # (c) xs and zs change places wherever they are read
        col = {k: next(i for i, c in enumerate(F.data_of(tracer)) if np.array_equal(c, args[k])) for k in (0, 1)}
        sw = {col[0]: col[1], col[1]: col[0]}
        _map_progs(t, lambda p: [(op, sw.get(ref, ref) if op == abi.EXPR_DATA else ref, v) for op, ref, v in p])
        for s in t.sites:
            for a in (s.arg[0], s.arg[1], s.obs):
                if a.kind == abi.ARG_DATA:
                    a.ref = sw.get(a.ref, a.ref)
    elif which == "reverse_sub":        # (d) b * xs - u becomes u - b * xs: the exact negation of the difference
        def rev(p):
            k = [op for op, _, _ in p].index(abi.EXPR_SUB)
            return p[:k + 1] + [(abi.EXPR_NEG, 0, 0.0)] + p[k + 1:]
        _map_progs(t, rev, [t.sites[q["y3"]]])
    elif which == "drop_plate":         # (e) the plated Gamma leaves the table; later references are renumbered
        k = q["y2"]
        del t.sites[k], t.meta[k]
        dn = lambda r: r - 1 if r > k else r  # noqa: E731
        _map_progs(t, lambda p: [(op, dn(ref) if op == abi.EXPR_SITE else ref, v) for op, ref, v in p])
        for s in t.sites:
            for a in (s.arg[0], s.arg[1]):
                if a.kind == abi.ARG_SITE:
                    a.ref = dn(a.ref)
    else:
        raise ValueError(which)
    return t


MUTATIONS = ("swap_args", "wrong_latent", "swap_columns", "reverse_sub", "drop_plate")


@pytest.mark.parametrize("which", MUTATIONS)
def test_mutations_fail_the_float64_check(oracle_ops, interleaved, which):
    """A replay built from a mutated copy of the tracer's table — the mistakes the check exists for — misses the float64
    reference by at least 10 x tol on more than half of the particles (and the unmutated table passes: test_interleaved)."""
    c = interleaved
    t = _mutate(c["tracer"], which, c["args"])
    lp, ll = P.Assess(oracle_ops, t, F.data_of(c["tracer"]))(F.columns_of(c["tracer"], c["latents"]))
    ref = c["ref"]
    share = {w: float(F.misses(g, ref.ref[w], ref.tol[w], factor=10.0).mean()) for w, g in (("lp", lp), ("ll", ll))}
    print(f"{which}: share of particles that miss by 10 x tol: {share}")
    assert max(share.values()) > 0.5
    with pytest.raises(AssertionError, match="miss the float64 reference"):
        F.check64(lp, what="lp", ref=ref)
        F.check64(ll, what="ll", ref=ref)


# ---- stage 0 through the renumbering of temper.prior_table -------------------------------------------------------------------
def test_prior_table_renumbers(interleaved):
    tr = interleaved["tracer"]
    pt = temper.prior_table(tr)
    q = {m["addr"]: i for i, m in enumerate(tr.meta)}
    assert (q["a"], q["g"], q["b"], q["u"]) == (0, 2, 4, 6)
    assert not any(s.observed == abi.SITE_PLATED for s in pt.sites) and len(pt.sites) == 5  # a, g, o1, b, u
    a, g, o1, b, u = pt.sites
    assert [s.out_col for s in pt.sites] == [0, 1, -1, 2, 3] and o1.observed == 1
    assert (b.arg[0].kind, b.arg[0].ref) == (abi.ARG_SITE, 0)          # b reads a: position 0 stays 0
    assert (tr.sites[q["b"]].arg[1].kind, tr.sites[q["b"]].arg[1].ref) == (abi.ARG_SITE, 2) and (b.arg[1].kind, b.arg[1].ref) == (abi.ARG_SITE, 1)
    assert (tr.sites[q["u"]].arg[0].kind, tr.sites[q["u"]].arg[0].ref) == (abi.ARG_SITE, 2) and (u.arg[0].kind, u.arg[0].ref) == (abi.ARG_SITE, 1)
    old = [ref for op, ref, _ in _prog(tr.sites[q["u"]].arg[1]) if op == abi.EXPR_SITE]
    new = [ref for op, ref, _ in _prog(u.arg[1]) if op == abi.EXPR_SITE]
    assert old == [4, 4] and new == [3, 3]                             # u reads b inside a program: position 4 becomes 3


@pytest.mark.parametrize("impl", ["threefry", "philox"])
def test_stage0_has_the_conditional_law(oracle_ops, interleaved, impl):
    """20 000 draws of stage 0 exactly as TemperedSMC.run makes them, from the table without its plated sites: every Normal and
    Gamma latent's probability-integral transform GIVEN ITS PARENTS (float64, from the source text: temper_fuzz.evaluate64)
    is uniform — Kolmogorov distance <= 1.95 / sqrt(n), the 0.1 % point of the Kolmogorov law; the keys are fixed.  `b`, declared
    after a plate, reads `g` for its scale: a reference prior_table moves from position 2 to 1, so a renumbering that reads the
    wrong site (`a` or the observed `o1` for `g`) gives `b` another conditional law and fails here."""
    import genjax

    n, c = 20000, interleaved
    tr = c["tracer"]
    key = genjax.random.key(2026, impl)

    def distances(table):
        with use_ops(oracle_ops):
            vals = oracle_ops.importance_run(_make_plan(table), prng.split_lazy(prng.fold_in(key, 0), n), n, [], [torch.float32] * tr.n_out,
                                             want_score=False, want_max_partials=False)[0]
        latents = {m["addr"]: vals[m["out_col"]].numpy().copy() for m in tr.meta if m["obs"] is None}
        assert set(latents) == {"a", "g", "b", "u"}
        assert (latents["g"] > 0).all() and ((latents["u"] > 0) & (latents["u"] < 1)).all()
        ev = F.evaluate64(F.INTERLEAVED, latents, c["obs"], c["args"])
        assert set(ev.pit) == {"a", "g", "b"}
        k = np.arange(1, n + 1)
        return {name: max(np.max(k / n - np.sort(u)), np.max(np.sort(u) - (k - 1) / n)) for name, u in ev.pit.items()}

    bound = 1.95 / np.sqrt(n)
    for name, dist in distances(temper.prior_table(tr)).items():
        print(f"{impl}: Kolmogorov distance of {name} given its parents {dist:.5f} (bound {bound:.5f})")
        assert dist <= bound, name
    # the control: the same table with b's reference to g left at its OLD position (2: the observed o1 there) or at a's
    for wrong in (2, 0):
        table = temper.prior_table(tr)
        assert table.sites[3].arg[1].ref == 1
        table.sites[3].arg[1].ref = wrong
        d = distances(table)
        print(f"{impl}: with b's scale read from position {wrong}: Kolmogorov distance of b {d['b']:.4f}, of a and g {d['a']:.5f} {d['g']:.5f}")
        assert d["b"] > 5 * bound and d["a"] <= bound and d["g"] <= bound


# ---- the float64 restatement on the two-plate regression (the bound of the end-to-end GPU test) -----------------------------
def test_restatement_recovers_the_two_plate_closed_form():
    """temper_ref's float64 sampler on plate_ref.two_plate() at the GPU test's n = 4096 and K = 2: two seeds outside the 24 the
    spread was measured over land within the end-to-end bound (four times that spread)."""
    model = P.two_plate()
    ez, em = P.restatement_errors(model, 4096, 2, (4000, 4001))
    print("log Z errors", ez, "mean errors / sd", em[:, :2], "sd errors", em[:, 2:])
    assert np.all(np.abs(ez) <= P.E2E_FACTOR * P.TWO_PLATE_SPREAD_LOG_Z)
    assert np.all(np.abs(em[:, :2]) <= P.E2E_FACTOR * np.asarray(P.TWO_PLATE_SPREAD_MEAN))
    assert np.all(np.abs(em[:, 2:]) <= P.E2E_FACTOR * np.asarray(P.TWO_PLATE_SPREAD_SD))
