"""Grouped tempered plans held to float64 without a GPU (tests/group_fuzz.py): the fixed body GROUPED_INTERLEAVED and random
grouped bodies are lowered on the oracle backend, replayed (group_ref.Assess, group_checks_ref.terms) and compared with the
float64 evaluation of their own source text; six mutations of the tracer's table and inputs must each FAIL that comparison;
the prior draws of `init` (group_ref.init_ref) have the conditional law the source text states; and the generated kernels of
the fixed body compile for gfx950 without scratch."""

import numpy as np
import pytest

import genjax
import group_checks_ref as GC
import group_fuzz as GF
import group_ref as GR
import ssm_fuzz as S
import temper_fuzz as F
from genjax._amd import abi, temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from offline import kernel_notes, ops  # noqa: F401  (ops: a fixture)

SEEDS = (31, 32, 33, 34)
PER_SEED = 50
MIN_KEPT = 0.5     # of the generated bodies (tests/group_fuzz.py's argument ranges are chosen so that this holds)
N = 257
GS = (1, 2, 5, 17)
CHECK_KERNELS = (("pointwise", 0, "gjx_pointwise_grouped_kernel"), ("psis", 0, "gjx_psis_grouped_kernel"),
                 ("predictive", 0, "gjx_predictive_grouped_kernel"), ("predictive", 1, "gjx_predictive_grouped_kernel"))


def _case(oracle_ops, G, seed=77):
    sizes = GR.LAYOUTS[G]
    args, obs = GF.random_inputs(np.random.default_rng(seed + G), GF.GROUPED_SITES, sizes)
    with use_ops(oracle_ops):
        tracer = temper.lower(GF.target_of(GF.GROUPED_INTERLEAVED, args, obs, G), 64)
    off = GF.offsets_of(sizes)
    return dict(G=G, sizes=sizes, args=args, obs=obs, tracer=tracer, off=off, assess=GR.Assess(oracle_ops, tracer, F.data_of(tracer), off))


@pytest.fixture(scope="module")
def fixed(oracle_ops):
    return {G: _case(oracle_ops, G) for G in GS}


def _prog(a):
    assert a.kind == abi.ARG_EXPR
    return [(o.op, o.ref) for o in (abi.ExprOp * a.ref).from_address(a.table)]


def _compare(c, latents, ref, context=""):
    """lp, ll and the pointwise terms of the replay against float64 -> the largest err / tol per quantity."""
    x, z = GF.columns_of(c["tracer"], latents)
    lp, ll = c["assess"](x, z)
    t = GC.terms(c["assess"], x, z)
    return {"lp": F.check64(lp, what="lp", ref=ref, context=context), "ll": F.check64(ll, what="ll", ref=ref, context=context),
            "terms": F.check64(t, what="terms", ref=ref, context=context)}


def test_fixed_body_lowers_whole(ops, fixed, tmp_path):  # noqa: F811
    """Fifteen sites, S = 4, every kind; an affine read of ONE grouped value is the GROUP operand with its scale and offset, a
    grouped value inside anything else a program leaf; the move kernel and the three grouped check kernels compile for gfx950
    without scratch."""
    tr = fixed[5]["tracer"]
    assert [m["addr"] for m in tr.meta] == [s[0] for s in GF.GROUPED_SITES] and len(tr.sites) == 15
    assert tr.n_grouped == 4 == abi.GROUP_MAX_SITES and tr.n_groups == 5 and len(tr.data) == 13 and tr.lf_cols == {9: 8, 12: 11}
    mode = {"latent": 0, "scalar": 1, "plated": abi.SITE_PLATED, "reader": abi.SITE_PLATED, "grouped": abi.SITE_GROUPED}
    dist = {"normal": abi.DIST_NORMAL, "gamma": abi.DIST_GAMMA, "beta": abi.DIST_BETA, "flip": abi.DIST_BERNOULLI,
            "poisson": abi.DIST_POISSON, "negative_binomial": abi.DIST_NEGATIVE_BINOMIAL}
    assert [(s.dist, s.observed) for s in tr.sites] == [(dist[k], mode[r]) for _, r, k in GF.GROUPED_SITES]
    q = {m["addr"]: tr.sites[i] for i, m in enumerate(tr.meta)}
    arg = lambda a: (a.kind, a.ref, a.scale, a.offset)  # noqa: E731
    # the grouped sites: literal, affine read of a scalar latent (by table position), program, parameter
    assert [q["u"].arg[k].kind for k in (0, 1)] == [abi.ARG_CONST] * 2
    assert arg(q["a"].arg[0]) == (abi.ARG_SITE, 0, 0.5, np.float32(0.2))
    assert set(_prog(q["a"].arg[1])[:2]) == {(abi.EXPR_SITE, 3), (abi.EXPR_CONST, 0)} and _prog(q["a"].arg[1])[2:] == [(abi.EXPR_MUL, 0), (abi.EXPR_EXP, 0)]
    assert arg(q["sg"].arg[0]) == (abi.ARG_SITE, 2, 1.5, 0.5) and q["c"].arg[0].kind == abi.ARG_PARAM
    # y1: both operands bare — grouped site 1 (a) as 2 z - 0.5, grouped site 2 (sg) as z + 0.1
    assert arg(q["y1"].arg[0]) == (abi.ARG_GROUP, 1, 2.0, -0.5) and arg(q["y1"].arg[1]) == (abi.ARG_GROUP, 2, 1.0, np.float32(0.1))
    leaves = lambda a: [ref for op, ref in _prog(a) if op == abi.EXPR_GROUP]  # noqa: E731
    assert leaves(q["y2"].arg[1]) == [1] and leaves(q["y3"].arg[0]) == [1] and leaves(q["y4"].arg[0]) == [0]
    assert leaves(q["y5"].arg[0]) == [1, 3] and leaves(q["y6"].arg[1]) == [3] and q["y4"].arg[1].kind == abi.ARG_DATA
    assert not any(a.kind == abi.ARG_GROUP for s in tr.sites if s is not q["y1"] for a in (s.arg[0], s.arg[1]))
    with use_ops(ops):
        c = fixed[5]
        t2 = temper.lower(GF.target_of(GF.GROUPED_INTERLEAVED, c["args"], c["obs"], 5), 64)
        plan = ops.temper_plan_create(t2.sites, keep=(t2.keep, t2))
    assert plan.n_latents == 3 and plan.n_grouped == 4
    for impl in (0, 1):
        assert plan.compile_check(impl) == 0, impl
        src = plan.source(impl)
        assert all(f"gz_{k}" in src for k in range(4)) and "gz_4" not in src
        notes = kernel_notes(src, tmp_path, f"gfuzz_move_{impl}")["gjx_temper_move_grouped_kernel"]
        print(f"move kernel impl {impl}: {notes}")
        assert notes["private_segment_fixed_size"] == 0, (impl, notes)
    for kern, impl, entry in CHECK_KERNELS[:2]:
        assert plan.group_checks_compile_check(kern, impl) == 0, (kern, impl)
        notes = kernel_notes(plan.group_checks_source(kern, impl), tmp_path, f"gfuzz_{kern}_{impl}")[entry]
        print(f"{kern} kernel impl {impl}: {notes}")
        assert notes["private_segment_fixed_size"] == 0, (kern, impl, notes)


@pytest.mark.parametrize("impl", [0, 1])
def test_fixed_body_predictive_kernel_has_no_scratch(ops, fixed, tmp_path, impl):  # noqa: F811
    """The grouped predictive kernel of the fixed body compiles for gfx950 — and is held to the condition the four hand-written
    models are held to: no scratch.  The regression case of a finding: with seven drawn sites (a Poisson and a
    negative-binomial draw among them) and the particle function inlined five times — a block of four and the rest loop — the
    THREEFRY kernel took 512 VGPRs, 256 AGPRs and 176 bytes of scratch per lane.  A table with more than four drawn sites now
    walks its particles one by one, in the same order (GenPredictive::kBlockedSites): 315 VGPRs, no scratch; tables of up to
    four drawn sites keep the block of four."""
    c = fixed[5]
    with use_ops(ops):
        t2 = temper.lower(GF.target_of(GF.GROUPED_INTERLEAVED, c["args"], c["obs"], 5), 64)
        plan = ops.temper_plan_create(t2.sites, keep=(t2.keep, t2))
        small = GR.target("slope", GR.LAYOUTS[5])[0]
        t3 = temper.lower(small, 64)
        blocked = ops.temper_plan_create(t3.sites, keep=(t3.keep, t3)).group_checks_source("predictive", impl)
    kern, _, entry = CHECK_KERNELS[2]
    src = plan.group_checks_source(kern, impl)
    assert "PredictiveAcc qA[7], qB[7];" in src and "hi - i >= 4u" not in src and src.count("pd_particle(a, prm") == 1
    assert "hi - i >= 4u" in blocked and blocked.count("pd_particle(a, prm") == 5
    assert plan.group_checks_compile_check(kern, impl) == 0
    notes = kernel_notes(plan.group_checks_source(kern, impl), tmp_path, f"gfuzz_{kern}_{impl}")[entry]
    print(f"{kern} kernel impl {impl}: {notes}")
    assert notes["private_segment_fixed_size"] == 0, (kern, impl, notes)


@pytest.mark.parametrize("G", GS)
def test_fixed_body_against_truth(fixed, G):
    """G in {1, 2, 5, 17} (empty first and last groups, a one-row group) x n in {1, 257}: the replay's lp, ll and terms within
    Reference's tolerance of float64."""
    c = fixed[G]
    for n in (1, N):
        latents = GF.latent_columns(np.random.default_rng(100 * G + n), GF.GROUPED_SITES, n, G)
        ref = F.Reference(GF.GROUPED_INTERLEAVED, latents, c["obs"], c["args"])
        assert ref.kept or n == 1, (G, n, ref.reasons)
        worst = _compare(c, latents, ref, context=str((G, n)))
        print(f"G = {G}, n = {n}: worst err / tol {worst}; f32 floors {ref.floor}")


@pytest.mark.parametrize("G", GS)
def test_fixed_body_outside_support(fixed, G):
    """Every fourth particle's grouped Gamma and Beta values outside their support, NaN included: lp is -inf exactly where
    float64 has it (check64 compares infinite entries exactly) and finite on the live particles."""
    c = fixed[G]
    for n in (1, N):
        latents = GF.latent_columns(np.random.default_rng(200 * G + n), GF.GROUPED_SITES, n, G, outside=True)
        ok = GF.inside(GF.GROUPED_SITES, latents)
        assert (~ok).sum() == -(-n // 4)
        ref = F.Reference(GF.GROUPED_INTERLEAVED, latents, c["obs"], c["args"], live=ok)
        assert ref.kept or n == 1, (G, n, ref.reasons)
        assert np.isneginf(ref.ref["lp"][~ok]).all() and np.isfinite(ref.ref["lp"][ok]).all()
        x, z = GF.columns_of(c["tracer"], latents)
        lp, ll = c["assess"](x, z)
        F.check64(lp, what="lp", ref=ref)
        F.check64(ll, what="ll", ref=ref)
        assert np.isneginf(lp[~ok]).all() and np.isfinite(lp[ok]).all() and not np.isnan(lp).any()


def test_random_bodies(oracle_ops):
    """200 random grouped bodies (4 seeds x 50) at n = 257 on LAYOUTS[5] (D = 13) and LAYOUTS[17] (D = 52); every fourth with
    grouped Gamma / Beta values outside their support.  No body fails to lower but for the documented refusal; at least half
    are kept by Reference (on both layouts); every kept body's lp, ll and terms lie within tolerance; every reader kind, every
    grouped kind and S = 4 occur."""
    layouts = (5, 17)
    kept, dropped, unlowered, worst = {s: 0 for s in SEEDS}, [], [], {"lp": 0.0, "ll": 0.0, "terms": 0.0}
    readers, grouped, s_values = set(), set(), set()
    with use_ops(oracle_ops):
        for seed in SEEDS:
            rng = np.random.default_rng(seed)
            for i in range(PER_SEED):
                outside = i % 4 == 3
                src, sites = GF.random_grouped_model(rng)
                readers |= {k for _, r, k in sites if r == "reader"}
                grouped |= {k for _, r, k in sites if r == "grouped"}
                s_values.add(sum(r == "grouped" for _, r, _ in sites))
                cases, reasons = [], []
                for G in layouts:
                    sizes = GR.LAYOUTS[G]
                    args, obs = GF.random_inputs(rng, sites, sizes)
                    latents = GF.latent_columns(rng, sites, N, G, outside=outside)
                    ref = F.Reference(src, latents, obs, args, live=GF.inside(sites, latents))
                    reasons += ref.reasons
                    cases.append((G, sizes, args, obs, latents, ref))
                try:
                    tracers = [temper.lower(GF.target_of(src, args, obs, G), N) for G, _, args, obs, _, _ in cases]
                except PlanUnsupported as e:
                    unlowered.append(f"seed {seed} case {i}: {e}\n{src}")
                    continue
                if reasons:
                    dropped.append(f"seed {seed} case {i}: {'; '.join(reasons)}")
                    continue
                for tracer, (G, sizes, args, obs, latents, ref) in zip(tracers, cases):
                    assert [m["addr"] for m in tracer.meta] == [s[0] for s in sites]
                    off = GF.offsets_of(sizes)
                    c = dict(tracer=tracer, assess=GR.Assess(oracle_ops, tracer, F.data_of(tracer), off))
                    w = _compare(c, latents, ref, context=f"seed {seed} case {i} G {G} outside {outside}\n{src}\nargs {args[3:5]}")
                    worst = {k: max(worst[k], w[k]) for k in worst}
                kept[seed] += 1
    print(f"kept per seed {kept} of {PER_SEED}; dropped {len(dropped)}; unlowered {len(unlowered)}; worst err / tol {worst}")
    print(f"reader kinds {sorted(readers)}; grouped kinds {sorted(grouped)}; S values {sorted(s_values)}")
    for r in unlowered + dropped:
        print("  ", r)
    assert not unlowered
    assert sum(kept.values()) >= MIN_KEPT * len(SEEDS) * PER_SEED
    assert readers == {"normal", "gamma", "beta", "flip", "poisson", "negative_binomial"} and grouped == {"normal", "gamma", "beta"}
    assert 4 in s_values and 1 in s_values


# ---- mutations -----------------------------------------------------------------------------------------------------------------------
class _Table:
    """What the replays read of a tracer, over a MUTATED copy of its site table (the product is not touched)."""

    def __init__(self, tracer):
        self.sites = [abi.Site.from_buffer_copy(s) for s in tracer.sites]
        self.meta, self.params, self.keep, self.lf_cols = list(tracer.meta), tracer.params, [], tracer.lf_cols


def _full_prog(a):
    return [(o.op, o.ref, o.value) for o in (abi.ExprOp * a.ref).from_address(a.table)]


def _mutated(c, which):
    """-> (table, data columns, offsets) of the fixed body's case with ONE mistake planted."""
    tr = c["tracer"]
    t, data, off = _Table(tr), F.data_of(tr), c["off"].copy()
    q = {m["addr"]: i for i, m in enumerate(tr.meta)}
    if which == "swap_group_refs":      # y5 reads c[g] where it should read a[g] and the reverse (both Normal)
        s = t.sites[q["y5"]]
        sw = {1: 3, 3: 1}
        s.arg[0] = abi.expr_arg([(op, sw[ref] if op == abi.EXPR_GROUP else ref, v) for op, ref, v in _full_prog(s.arg[0])], t.keep)
    elif which == "shift_offsets":      # every inner boundary one row later: a group's first row is scored at the group before it
        off[1:-1] = np.minimum(off[1:-1] + 1, off[-1])
    elif which == "swap_grouped_args":  # the grouped Gamma's shape and rate
        s = t.sites[q["sg"]]
        a0, a1 = abi.Arg.from_buffer_copy(s.arg[0]), abi.Arg.from_buffer_copy(s.arg[1])
        s.arg[0], s.arg[1] = a1, a0
    elif which == "wrong_scalar":       # the grouped Normal's location reads `ls` for `m`
        a = t.sites[q["a"]].arg[0]
        assert a.kind == abi.ARG_SITE and a.ref == q["m"]
        a.ref = q["ls"]
    elif which == "drop_reader":        # the flip reader leaves acc (no later site refers to a position behind it)
        del t.sites[q["y3"]], t.meta[q["y3"]]
    elif which == "swap_count_columns":  # y5's observed column and its log k! column
        k = tr.sites[q["y5"]].obs.ref
        data[k], data[k + 1] = data[k + 1], data[k]
    else:
        raise ValueError(which)
    return t, data, off


MUTATIONS = ("swap_group_refs", "shift_offsets", "swap_grouped_args", "wrong_scalar", "drop_reader", "swap_count_columns")


@pytest.fixture(scope="module")
def mutation_case(fixed):
    c = fixed[5]
    latents = GF.latent_columns(np.random.default_rng(91), GF.GROUPED_SITES, N, 5)
    return c, latents, F.Reference(GF.GROUPED_INTERLEAVED, latents, c["obs"], c["args"])


@pytest.mark.parametrize("which", MUTATIONS)
def test_mutations_fail_the_float64_check(oracle_ops, mutation_case, which):
    """A replay built from a mutated copy of the table, offsets or columns — the mistakes a replay built from the tracer's own
    table shares with the kernel — misses the float64 reference (the unmutated case passes: test_fixed_body_against_truth)."""
    c, latents, ref = mutation_case
    assert ref.kept, ref.reasons
    t, data, off = _mutated(c, which)
    assess = GR.Assess(oracle_ops, t, data, off)
    x, z = GF.columns_of(c["tracer"], latents)
    lp, ll = assess(x, z)
    got = {"lp": lp, "ll": ll, "terms": GC.terms(assess, x, z)}
    share = {w: float(F.misses(g, ref.ref[w], ref.tol[w], factor=10.0).mean()) for w, g in got.items()}
    print(f"{which}: share of entries that miss by 10 x tol: {share}")
    with pytest.raises(AssertionError, match="miss the float64 reference"):
        for w, g in got.items():
            F.check64(g, what=w, ref=ref)


# ---- init ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["threefry", "philox"])
def test_init_has_the_conditional_law(oracle_ops, fixed, impl):
    """init_ref's draws at n = 1000, G = 17 (17000 per grouped site): every site's probability-integral transform under the
    float64 arguments the SOURCE TEXT gives it at the particle's scalars, and the conditional residuals against those
    arguments and every scalar latent, at ssm_fuzz.check_laws' derived bounds.  `a` reads `m` by position 0 and `ls` (table
    position 3, latent 2) inside a program; `sg` reads `r` (position 2, latent 1): a wrong renumbering gives another law."""
    n, c = 1000, fixed[17]
    assert n * 17 >= F.LAW_MIN_DRAWS
    tr = c["tracer"]
    latents = GF.latent_columns(np.random.default_rng(92), GF.GROUPED_SITES, n, 17)
    x, _ = GF.columns_of(tr, latents)
    z = GR.init_ref(oracle_ops, tr, genjax.random.key(2027, impl), x, 17)
    addrs = [m["addr"] for m in tr.meta if m.get("grouped")]
    assert addrs == ["u", "a", "sg", "c"] and all(v.shape == (17, n) and np.isfinite(v).all() for v in z)
    scalars = {k: v for k, v in latents.items() if np.ndim(v) == 1}
    laws = GF.init_laws(GF.GROUPED_INTERLEAVED, scalars, c["obs"], c["args"], dict(zip(addrs, z)))
    assert {"u", "a", "sg", "c", ("a", "latent", "m"), ("a", "latent", "ls"), ("sg", "latent", "r")} <= set(laws)
    worst = S.check_laws(laws, f"init {impl}")
    print(f"init {impl}: {worst}")
    # the control: the draws of `a` against the law of a body whose `a` reads `r` for `m` fail
    wrong = GF.GROUPED_INTERLEAVED.replace("normal(0.5 * m + 0.2,", "normal(0.5 * r + 0.2,")
    assert wrong != GF.GROUPED_INTERLEAVED
    with pytest.raises(AssertionError, match="law of"):
        S.check_laws(GF.init_laws(wrong, scalars, c["obs"], c["args"], dict(zip(addrs, z))))
