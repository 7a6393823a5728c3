"""The grouped tempered kernels held to float64 on the GPU (tests/group_fuzz.py): the fixed body GROUPED_INTERLEAVED — S = 4
grouped sites of every kind, a grouped Beta before a scalar latent, a program and an affine read as a grouped site's arguments,
readers of every plated kind (Poisson and negative binomial among them), bare affine GROUP operands, a grouped value under a
nonlinear function — and random grouped bodies through gjx_temper_move_grouped (assess, the prior draws of `init`, K = 3 sweeps)
and gjx_temper_pointwise_grouped: bit for bit against the replay tests/group_ref.py builds from the tracer's table, AND within
temper_fuzz.Reference's tolerance of the float64 evaluation of the body's own source text, which shares nothing with the
lowering.  The predictive kernel is compared for the fixed body without its count readers (the oracle the replays are built
from draws no counts)."""

import time

import numpy as np
import pytest
import torch

import genjax
import group_checks_ref as GC
import group_fuzz as GF
import group_ref as GR
import ssm_fuzz as S
import temper_fuzz as F
from genjax._amd import temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from test_gpu_temper_fuzz import _ancestors, _pointwise_case, _same

pytestmark = pytest.mark.gpu

NS = (1, 257, 1000)
GS = (1, 2, 5, 17)
SEEDS = (41, 42, 43, 44)
BODIES = 3                    # per (seed, generator): see test_random_bodies
SCALE = {"normal": 0.3, "gamma": 0.2, "beta": 0.1}
IMPL = {0: "threefry", 1: "philox"}
LAYOUTS = GC.LAYOUTS          # group_ref's four and the WIDE one (G = 7, D = 401)


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).cuda() for c in cols]


def _lower(hip_ops, src, args, obs, G):
    """-> (tracer, plan with parameters, data and groups set): lowered on the HIP backend from device tensors."""
    with use_ops(hip_ops):
        tracer = temper.lower(GF.target_of(src, args, obs, G, device="cuda"), 64)
        plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
        if tracer.params:
            plan.set_params(tracer.params)
        plan.set_data(tracer.data_columns(hip_ops.device()))
        plan.set_groups(tracer.group_offsets().to(hip_ops.device()))
    return tracer, plan


_FIXED = {}


def _fixed(hip_ops, oracle_ops, G):
    """The fixed body over LAYOUTS[G] (the inputs of tests/test_group_fuzz_cpu.py for group_ref's layouts), made once."""
    if G not in _FIXED:
        sizes = LAYOUTS[G]
        args, obs = GF.random_inputs(np.random.default_rng(77 + G), GF.GROUPED_SITES, sizes)
        tracer, plan = _lower(hip_ops, GF.GROUPED_INTERLEAVED, args, obs, G)
        assert [m["addr"] for m in tracer.meta] == [s[0] for s in GF.GROUPED_SITES] and plan.n_grouped == 4
        off = GF.offsets_of(sizes)
        _FIXED[G] = dict(G=G, sizes=sizes, args=args, obs=obs, tracer=tracer, plan=plan, off=off,
                         assess=GR.Assess(oracle_ops, tracer, F.data_of(tracer), off),
                         scales=[SCALE[k] for _, role, k in GF.GROUPED_SITES if role == "latent"])
    return _FIXED[G]


def _assess_case(hip_ops, plan, assess, x, z, impls, ref, case, times=None):
    """K = 0, recompute = 1: x and z come back unchanged, (lp, ll) bit-equal to the replay's and within Reference's tolerance of
    float64 -> (worst err / tol, lp_ref, ll_ref)."""
    lp_ref, ll_ref = assess(x, z)
    worst = 0.0
    for impl in impls:
        t0 = time.time()
        xo, zo, lp, ll, acc, accz = hip_ops.temper_move_grouped(plan, genjax.random.key(3, IMPL[impl]), _dev(x), _dev(z), None, None, 0.37, 0,
                                                                recompute=True)
        lp, ll = lp.cpu().numpy(), ll.cpu().numpy()
        if times is not None:
            times.append(time.time() - t0)
        assert all(_same(a.cpu().numpy(), b) for a, b in zip(xo, x)) and all(_same(a.cpu().numpy(), b) for a, b in zip(zo, z)), case
        assert _same(lp, lp_ref), (case, impl, lp[:4], lp_ref[:4])
        assert _same(ll, ll_ref), (case, impl, ll[:4], ll_ref[:4])
        assert int(acc.sum()) == 0 and int(accz.sum()) == 0
        if ref is not None:
            worst = max(worst, F.check64(lp, what="lp", ref=ref, context=str(case)), F.check64(ll, what="ll", ref=ref, context=str(case)))
    return worst, lp_ref, ll_ref


def _sweep_case(hip_ops, oracle_ops, plan, assess, x, z, scales, impl, seed, case, grids=(0,)):
    """K = 3 sweeps through an ancestors column with repeats and out-of-range words: group_ref.move_ref's, bit for bit
    -> (the reference, its statistics)."""
    n, K, beta = len(x[0]), 3, 0.37
    rng = np.random.default_rng(seed)
    lp0, ll0 = assess(x, z)
    anc = _ancestors(n, rng)
    zsc = rng.uniform(0.2, 0.6, (len(z), assess.G)).astype(np.float32)
    key = genjax.random.key(1000 + seed, IMPL[impl])
    stats = {}
    ref = GR.move_ref(oracle_ops, assess, key, x, z, lp0, ll0, beta, K, scales, zsc, ancestors=anc, stats=stats)
    for wg in grids:
        xo, zo, lp, ll, acc, accz = hip_ops.temper_move_grouped(plan, key, _dev(x), _dev(z), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(),
                                                                beta, K, scales, torch.from_numpy(zsc).cuda(), ancestors=torch.from_numpy(anc).cuda(),
                                                                max_workgroups=wg)
        assert np.array_equal(acc.cpu().numpy(), ref[4]), (case, wg)
        assert np.array_equal(accz.cpu().numpy(), ref[5]), (case, wg, accz.cpu().numpy()[:8], ref[5][:8])
        assert all(_same(a.cpu().numpy(), b) for a, b in zip(xo, ref[0])), (case, wg)
        assert all(_same(a.cpu().numpy(), b) for a, b in zip(zo, ref[1])), (case, wg)
        assert _same(lp.cpu().numpy(), ref[2]) and _same(ll.cpu().numpy(), ref[3]), (case, wg)
    return ref, stats


# ---- the fixed body ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", GS)
def test_fixed_assess(hip_ops, oracle_ops, G):
    """n in {1, 257, 1000} x G in {1, 2, 5, 17}, both generators: x and z back unchanged, (lp, ll) bit-equal to the replay and
    within Reference's tolerance of float64."""
    c, worst = _fixed(hip_ops, oracle_ops, G), 0.0
    for n in NS:
        latents = GF.latent_columns(np.random.default_rng(300 * G + n), GF.GROUPED_SITES, n, G)
        ref = F.Reference(GF.GROUPED_INTERLEAVED, latents, c["obs"], c["args"])
        assert ref.kept or n == 1, (n, G, ref.reasons)
        x, z = GF.columns_of(c["tracer"], latents)
        w, _, _ = _assess_case(hip_ops, c["plan"], c["assess"], x, z, (0, 1), ref, ("fixed", n, G))
        worst = max(worst, w)
    print(f"fixed body assess, G = {G}: worst err / tol {worst:.3f}")


def test_fixed_outside_support(hip_ops, oracle_ops):
    """n = 1000, G = 5, every fourth particle's grouped Gamma / Beta values outside their support (NaN included): lp is -inf
    exactly as float64 has it and never NaN on the live particles."""
    n, G = 1000, 5
    c = _fixed(hip_ops, oracle_ops, G)
    latents = GF.latent_columns(np.random.default_rng(35), GF.GROUPED_SITES, n, G, outside=True)
    ok = GF.inside(GF.GROUPED_SITES, latents)
    ref = F.Reference(GF.GROUPED_INTERLEAVED, latents, c["obs"], c["args"], live=ok)
    assert ref.kept, ref.reasons
    x, z = GF.columns_of(c["tracer"], latents)
    worst, lp_ref, _ = _assess_case(hip_ops, c["plan"], c["assess"], x, z, (0, 1), ref, "outside")
    assert (~ok).sum() == n // 4 and np.isneginf(lp_ref[~ok]).all() and np.isneginf(ref.ref["lp"][~ok]).all()
    assert np.isfinite(lp_ref[ok]).all() and not np.isnan(lp_ref).any()
    print(f"outside support: worst err / tol {worst:.3f}")


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("G", (5, 17))
def test_fixed_sweeps(hip_ops, oracle_ops, G, impl):
    """K = 3 at n = 257, ancestors with repeats and out-of-range words, whatever the grid: everything bit-equal to
    group_ref.move_ref; some group proposals accepted and some rejected; the Gamma and Beta grouped sites' random walks leave
    their supports (lpz' = -inf, counted by the replay)."""
    n = 257
    c = _fixed(hip_ops, oracle_ops, G)
    latents = GF.latent_columns(np.random.default_rng(32 + G), GF.GROUPED_SITES, n, G)
    x, z = GF.columns_of(c["tracer"], latents)
    ref, stats = _sweep_case(hip_ops, oracle_ops, c["plan"], c["assess"], x, z, c["scales"], impl, 5 + G, ("fixed", G, impl), grids=(0, 1, 7))
    assert 0 < int(ref[4].sum()) < n * 3 and 0 < int(ref[5].sum()) < n * 3 * G
    assert stats["outside"] > 0


@pytest.mark.parametrize("impl", [0, 1])
def test_fixed_init(hip_ops, oracle_ops, impl):
    """n in {257, 1000}, G = 17: z is bit-equal to group_ref.init_ref (a grouped site's program argument through a single-site
    oracle plan), (lp, ll) is the replay's assess of what was drawn, and the n = 1000 draws have the conditional law the source
    text states (the call of tests/test_group_fuzz_cpu.py)."""
    G = 17
    c = _fixed(hip_ops, oracle_ops, G)
    tr = c["tracer"]
    addrs = [m["addr"] for m in tr.meta if m.get("grouped")]
    for n in (257, 1000):
        rng = np.random.default_rng(21 + n)
        latents = GF.latent_columns(rng, GF.GROUPED_SITES, n, G)
        x, _ = GF.columns_of(tr, latents)
        anc = _ancestors(n, rng)
        key, ik = genjax.random.key(5, IMPL[impl]), genjax.random.key(77, IMPL[impl])
        ref = GR.move_ref(oracle_ops, c["assess"], key, x, None, None, None, 0.5, 0, None, None, ancestors=anc, recompute=True, init_key=ik)
        xo, zo, lp, ll, _, _ = hip_ops.temper_move_grouped(c["plan"], key, _dev(x), None, None, None, 0.5, 0, ancestors=torch.from_numpy(anc).cuda(),
                                                           recompute=True, init_key=ik)
        case = ("init", impl, n)
        assert all(_same(a.cpu().numpy(), b) for a, b in zip(xo, ref[0])), case
        assert all(_same(a.cpu().numpy(), b) for a, b in zip(zo, ref[1])), case
        assert _same(lp.cpu().numpy(), ref[2]) and _same(ll.cpu().numpy(), ref[3]), case
        if n == 1000:
            assert n * G >= F.LAW_MIN_DRAWS
            scalars = {m["addr"]: col for m, col in zip([m for m in tr.meta if m["obs"] is None and not m.get("grouped")], ref[0])}
            z = {a: v.cpu().numpy() for a, v in zip(addrs, zo)}
            worst = S.check_laws(GF.init_laws(GF.GROUPED_INTERLEAVED, scalars, c["obs"], c["args"], z), str(case))
            print(f"init {IMPL[impl]}: {worst}")


@pytest.mark.parametrize("G", (1, 5, 17, 7))
def test_fixed_pointwise(hip_ops, oracle_ops, G):
    """n in {5, 257, 1000} x G in {1, 5, 17, 7 (WIDE: D = 401, a group across the kernel's row tiles)} on a centred population:
    gjx_temper_pointwise_grouped at pointwise_ref's tolerances against float64 reductions of the replay's terms, and those terms
    within Reference's tolerance of float64."""
    c, rng, worst = _fixed(hip_ops, oracle_ops, G), np.random.default_rng(33 + G), 0.0
    ns = (5, 257, 1000)
    pops = [GF.latent_columns(rng, GF.GROUPED_SITES, n, G, centred=True) for n in ns]
    cols = [GF.columns_of(c["tracer"], p) for p in pops]
    for n, latents, (x, z), t in zip(ns, pops, cols, GC.terms_many(c["assess"], cols)):
        assert t.shape == (len(c["args"][-1]), n)
        got = hip_ops.temper_pointwise(c["plan"], _dev(x), z=_dev(z)).cpu().numpy()
        _pointwise_case(got, t, ("fixed", n, G), min_share=0.9)
        ref = F.Reference(GF.GROUPED_INTERLEAVED, latents, c["obs"], c["args"])
        worst = max(worst, F.check64(t, what="terms", ref=ref, context=str((n, G))))
    print(f"fixed body pointwise terms, G = {G}: worst err / tol {worst:.3f}")


def test_fixed_inf_row(hip_ops, oracle_ops):
    """One +inf observed value in the Normal reader's column: that row's lse is -inf and its count 0."""
    n, G = 257, 5
    c = _fixed(hip_ops, oracle_ops, G)
    tr = c["tracer"]
    data = F.data_of(tr)
    D = len(data[0])
    k = next(i for i, col in enumerate(data) if np.array_equal(col, c["obs"]["y1"]))
    r = D // 2
    data[k][r] = np.inf
    try:
        c["plan"].set_data(_dev(data))
        assess = GR.Assess(oracle_ops, tr, data, c["off"])
        latents = GF.latent_columns(np.random.default_rng(34), GF.GROUPED_SITES, n, G, centred=True)
        x, z = GF.columns_of(tr, latents)
        _, lp_ref, ll_ref = _assess_case(hip_ops, c["plan"], assess, x, z, (0, 1), None, "inf_row")
        assert np.isfinite(lp_ref).all() and np.isneginf(ll_ref).all()
        t = GC.terms(assess, x, z)
        assert np.isneginf(t[r]).all() and np.isfinite(np.delete(t, r, axis=0)).all()
        got = hip_ops.temper_pointwise(c["plan"], _dev(x), z=_dev(z)).cpu().numpy()
        assert got[0][r] == -np.inf and got[3][r] == 0.0
        assert _pointwise_case(got, t, "inf_row") == (D - 1) / D
    finally:
        with use_ops(hip_ops):
            c["plan"].set_data(tr.data_columns(hip_ops.device()))


# ---- the predictive kernel of a table with more than four drawn sites ------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1])
def test_float_readers_predictive(hip_ops, oracle_ops, impl):
    """The fixed body without its two count readers (the oracle draws no counts): five drawn sites, so the generated predictive
    kernel walks its particles one by one (GenPredictive::kBlockedSites) where the four hand-written models take blocks of
    four.  n in {5, 257} on G = 17 and G = 5, stored strides 1 and 7: the draws bit-equal to group_checks_ref.Replay, the row
    statistics at predictive_ref's tolerances."""
    import predictive_ref as PR

    src = "".join(line + "\n" for line in GF.GROUPED_INTERLEAVED.splitlines() if '@ "y5"' not in line and '@ "y6"' not in line)
    sites = tuple(s for s in GF.GROUPED_SITES if s[0] not in ("y5", "y6"))
    key = genjax.random.key(7, IMPL[impl])
    for G in (17, 5):
        sizes = LAYOUTS[G]
        args, obs = GF.random_inputs(np.random.default_rng(177 + G), sites, sizes)
        tracer, plan = _lower(hip_ops, src, args, obs, G)
        assert "hi - i >= 4u" not in plan.group_checks_source("predictive", impl)
        replay = GC.Replay(oracle_ops, tracer, F.data_of(tracer), GF.offsets_of(sizes), key.impl)
        assert replay.addrs == ["w", "y1", "y2", "y3", "y4"]
        rng = np.random.default_rng(44 + G)
        for n in (5, 257):
            x, z = GF.columns_of(tracer, GF.latent_columns(rng, sites, n, G, centred=True))
            y = replay.draws(key, x, z)
            assert y.shape == (5, len(args[-1]), n) and np.isfinite(y).all()
            for k in (1, 7):
                out, draws = hip_ops.temper_predictive(plan, key, _dev(x), k, z=_dev(z))
                assert PR.same_bits(draws.cpu().numpy(), np.transpose(y, (0, 2, 1))[:, ::k]), (G, impl, n, k)
                PR.check(out.cpu().numpy(), y, replay.observed(), (G, impl, n, k))


# ---- random bodies -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("seed", SEEDS)
def test_random_bodies(hip_ops, oracle_ops, seed, impl):
    """The first BODIES kept bodies of the seed's stream (of at most 3 x BODIES generated; the shares are asserted on 200 bodies by
    tests/test_group_fuzz_cpu.py) at n = 257 on LAYOUTS[17] and LAYOUTS[5], the second without a compilation: assess bit-equal
    to the replay and within tolerance of float64; K = 3 sweeps bit-equal to group_ref.move_ref; the pointwise outputs on a
    centred population at pointwise_ref's tolerances, and that population's terms within tolerance of float64.
    Each body costs one compilation of its move kernel per generator and one of its pointwise kernel; the replay's oracle
    calls per row and group are CPU time.  The times of a run are printed; profiles/group_fuzz_summary.md records the measured
    range and why BODIES is what it is."""
    n, layouts = 257, (17, 5)
    rng = np.random.default_rng(seed)
    done, attempts, worst, refused, t_launch, t_body = 0, 0, 0.0, [], [], []
    while done < BODIES and attempts < 3 * BODIES:
        attempts += 1
        t_start = time.time()
        src, sites = GF.random_grouped_model(rng)
        cases, reasons = [], []
        for G in layouts:
            args, obs = GF.random_inputs(rng, sites, LAYOUTS[G], like=(cases[0][1], cases[0][2]) if cases else None)
            latents = GF.latent_columns(rng, sites, n, G)
            centred = GF.latent_columns(rng, sites, n, G, centred=True)
            refs = [F.Reference(src, pop, obs, args) for pop in (latents, centred)]
            reasons += refs[0].reasons + refs[1].reasons
            cases.append((G, args, obs, latents, centred, refs))
        if reasons:
            refused.append("dropped: " + "; ".join(reasons))
            continue
        scales = [SCALE[k] for _, role, k in sites if role == "latent"]
        compiles = None
        try:
            lowered = [_lower(hip_ops, src, args, obs, G) for G, args, obs, _, _, _ in cases]
        except PlanUnsupported as e:
            refused.append(f"unlowered: {e}")
            continue
        for (tracer, plan), (G, args, obs, latents, centred, refs) in zip(lowered, cases):
            case = f"seed {seed} body {attempts} impl {impl} G {G}\n{src}\nargs {args[3:5]}"
            assert [m["addr"] for m in tracer.meta] == [s[0] for s in sites]
            assess = GR.Assess(oracle_ops, tracer, F.data_of(tracer), GF.offsets_of(LAYOUTS[G]))
            x, z = GF.columns_of(tracer, latents)
            times = []
            w, _, _ = _assess_case(hip_ops, plan, assess, x, z, (impl,), refs[0], case, times=times)
            worst = max(worst, w)
            _sweep_case(hip_ops, oracle_ops, plan, assess, x, z, scales, impl, seed, case)
            cx, cz = GF.columns_of(tracer, centred)
            t = GC.terms(assess, cx, cz)
            got = hip_ops.temper_pointwise(plan, _dev(cx), z=_dev(cz)).cpu().numpy()
            _pointwise_case(got, t, case, min_share=0.9)
            worst = max(worst, F.check64(t, what="terms", ref=refs[1], context=case))
            if compiles is None:
                t_launch += times  # (the first launch of the body under this generator: its compilation)
                compiles = hip_ops.jit_stats()["compiles"]
            else:
                assert hip_ops.jit_stats()["compiles"] == compiles, case  # (another G, another D, other data: nothing compiled)
        t_body.append(time.time() - t_start)
        done += 1
    print(f"seed {seed} {IMPL[impl]}: {done} bodies of {attempts} generated; worst err / tol {worst:.3f}; first move launch of a body "
          f"(compilation included) {min(t_launch, default=0):.2f} .. {max(t_launch, default=0):.2f} s; a whole body, replay included, "
          f"{min(t_body, default=0):.2f} .. {max(t_body, default=0):.2f} s")
    for r in refused:
        print("  ", r)
    assert done == BODIES
