"""Grouped tempered plans on the GPU (include/gjx_group.h): assess, the prior draws of `init` and the sweeps held bit for bit
to the replay tests/group_ref.py builds from unchanged oracle entry points and numpy sums in the header's order; a Gamma
grouped site whose proposals leave its support; flat sites next to the grouped one; the grouped plan next to the unrolled plan
of the same data; no compilation for another data set; the launch counts of a stage; and the sampler end to end against the
closed form of the Gaussian random-intercept model."""

import numpy as np
import pytest
import torch

import genjax
import group_ref as GR
from genjax import ChoiceMap, Target, gen, normal
from genjax._amd import temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from group_ref import E2E_FACTOR, SPREAD_LOG_Z, SPREAD_MEAN
from test_gpu_guided import _kernel_nodes

pytestmark = pytest.mark.gpu

GS = (1, 2, 5, 17)
SCALES = (0.3, 0.3)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _equal(a, b):
    """Integer views, tolerance 0."""
    return np.array_equal(_bits(a), _bits(b))


def _same(a, b):
    """Integer views, tolerance 0 — except that a NaN equals a NaN (its payload is the platform's, not the specification's)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


def _key(seed, impl):
    return genjax.random.key(seed, "philox" if impl else "threefry")


_CASES = {}


def _case(hip_ops, oracle_ops, name, G):
    """-> (tracer, plan with parameters, data and groups set, the replay's assess, offsets), made once per (model, G)."""
    if (name, G) not in _CASES:
        with use_ops(hip_ops):
            target, g, off = GR.target(name, GR.LAYOUTS[G], seed=1)
            tracer = temper.lower(target, 64)
            plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            if tracer.params:
                plan.set_params(tracer.params)
            plan.set_data(tracer.data_columns(hip_ops.device()))
            plan.set_groups(tracer.group_offsets().to(hip_ops.device()))
        data = [t.detach().to(torch.float32).numpy().copy() for t in tracer.data]
        _CASES[name, G] = (tracer, plan, GR.Assess(oracle_ops, tracer, data, off), off)
    return _CASES[name, G]


def _z_scales(S, G, rng):
    return rng.uniform(0.2, 0.6, (S, G)).astype(np.float32)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("name", ("intercept", "slope"))
def test_assess_pin(hip_ops, oracle_ops, name, G):
    """K = 0, recompute = 1 on given columns: x and z come back as they went in, (lp, ll) are the replay's, bit for bit —
    n = 300 (a partial wave) and 512, both generators (no draw is made: one reference for both)."""
    _, plan, assess, _ = _case(hip_ops, oracle_ops, name, G)
    rng = np.random.default_rng(11 + G)
    for n in (300, 512):
        x, z = GR.columns(name, G, n, rng)
        lp_ref, ll_ref = assess(x, z)
        assert np.all(np.isfinite(lp_ref)) and np.all(np.isfinite(ll_ref))
        for impl in (0, 1):
            xo, zo, lp, ll, acc, accz = hip_ops.temper_move_grouped(plan, _key(3, impl), _dev(x), _dev(z), None, None, 0.37, 0, recompute=True)
            case = (name, G, n, impl)
            assert all(_equal(a.cpu().numpy(), b) for a, b in zip(xo, x)) and all(_equal(a.cpu().numpy(), b) for a, b in zip(zo, z)), case
            assert _equal(lp.cpu().numpy(), lp_ref), (case, lp.cpu().numpy()[:4], lp_ref[:4])
            assert _equal(ll.cpu().numpy(), ll_ref), (case, ll.cpu().numpy()[:4], ll_ref[:4])
            assert int(acc.sum()) == 0 and int(accz.sum()) == 0


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("name", ("slope", "gamma"))
def test_init_pin(hip_ops, oracle_ops, name, impl):
    """init: z[s][g] is element i of the stand-alone sample kernel (the oracle's gjx_sample_logpdf_normal / _gamma) under
    fold_in(init_key, g) with the grouped sites' own numbering, at the particle's scalars — read through the ancestors — and
    (lp, ll) is assess of what was drawn."""
    G = 5
    tracer, plan, assess, _ = _case(hip_ops, oracle_ops, name, G)
    for n in (300, 512):
        rng = np.random.default_rng(21 + n)
        x, _ = GR.columns(name, G, n, rng)
        anc = _ancestors(n, rng)
        key, ik = _key(5, impl), _key(77, impl)
        ref = GR.move_ref(oracle_ops, assess, key, x, None, None, None, 0.5, 0, None, None, ancestors=anc, recompute=True, init_key=ik)
        xo, zo, lp, ll, _, _ = hip_ops.temper_move_grouped(plan, key, _dev(x), None, None, None, 0.5, 0, ancestors=torch.from_numpy(anc).cuda(),
                                                           recompute=True, init_key=ik)
        case = (name, impl, n)
        assert all(_equal(a.cpu().numpy(), b) for a, b in zip(xo, ref[0])), case
        assert all(_equal(a.cpu().numpy(), b) for a, b in zip(zo, ref[1])), case
        assert _same(lp.cpu().numpy(), ref[2]) and _same(ll.cpu().numpy(), ref[3]), case
        # the draws are not one number repeated: groups and particles differ
        z0 = zo[0].cpu().numpy()
        assert len(np.unique(z0)) > z0.size // 2


def _ancestors(n, rng):
    """A random non-identity map with repeats and out-of-range words (they clamp to n - 1)."""
    a = rng.integers(0, max(1, n // 2), n).astype(np.int64)
    wild = np.array([-1, n, n + 5, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)
    a[rng.permutation(n)[:len(wild)]] = wild
    return a.astype(np.int32)


def _sweep(hip_ops, oracle_ops, name, G, impl, n, K, seed, outside=False, wgs=(0,)):
    tracer, plan, assess, _ = _case(hip_ops, oracle_ops, name, G)
    rng = np.random.default_rng(seed)
    x, z = GR.columns(name, G, n, rng, outside=outside)
    lp0, ll0 = assess(x, z)
    anc = _ancestors(n, rng)
    zsc = _z_scales(len(z), G, rng)
    sc = SCALES[:len(x)]
    key = _key(1000 + seed, impl)
    beta = 0.37
    stats = {}
    ref = GR.move_ref(oracle_ops, assess, key, x, z, lp0, ll0, beta, K, sc, zsc, ancestors=anc, stats=stats)
    for wg in wgs:
        out = hip_ops.temper_move_grouped(plan, key, _dev(x), _dev(z), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(), beta, K, sc,
                                          torch.from_numpy(zsc).cuda(), ancestors=torch.from_numpy(anc).cuda(), max_workgroups=wg)
        xo, zo, lp, ll, acc, accz = out
        case = (name, G, impl, n, K, wg)
        assert np.array_equal(acc.cpu().numpy(), ref[4]), case
        assert np.array_equal(accz.cpu().numpy(), ref[5]), (case, accz.cpu().numpy()[:8], ref[5][:8])
        assert all(_equal(a.cpu().numpy(), b) for a, b in zip(xo, ref[0])), case
        assert all(_same(a.cpu().numpy(), b) for a, b in zip(zo, ref[1])), case
        assert _same(lp.cpu().numpy(), ref[2]) and _same(ll.cpu().numpy(), ref[3]), case
    return ref, stats


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("name", ("intercept", "slope"))
def test_sweep_pin(hip_ops, oracle_ops, name, G, impl):
    """K = 1 (n = 512) and K = 3 (n = 300, a partial wave; whatever the grid) through an ancestors column with repeats and
    out-of-range words: x, z, lp, ll and both accept counts are group_ref.move_ref's, bit for bit."""
    for n, K, wgs in ((512, 1, (0,)), (300, 3, (0, 1))):
        ref, _ = _sweep(hip_ops, oracle_ops, name, G, impl, n, K, seed=200 + 10 * G + impl, wgs=wgs)
        assert 0 < int(ref[4].sum()) < n * K and 0 < int(ref[5].sum()) < n * K * G  # some accepted, some rejected, in both phases


@pytest.mark.parametrize("impl", [0, 1])
def test_gamma_group(hip_ops, oracle_ops, impl):
    """A Gamma grouped site: random-walk proposals leave its support and are rejected (lpz' = -inf); start values outside it
    (negative, zero, NaN) have lpz = -inf; lp is never NaN."""
    for G, n, K in ((5, 300, 3), (2, 512, 1)):
        ref, stats = _sweep(hip_ops, oracle_ops, "gamma", G, impl, n, K, seed=300 + G + impl, outside=True)
        assert stats["outside"] > 0 and not np.isnan(ref[2]).any()
        assert 0 < int(ref[5].sum()) < n * K * G


@pytest.mark.parametrize("impl", [0, 1])
def test_flat_sites(hip_ops, oracle_ops, impl):
    """A flat plated site and a scalar observed site next to the grouped one: they enter lp_flat / ll_flat as in an ungrouped plan."""
    _, _, assess, _ = _case(hip_ops, oracle_ops, "flat", 5)
    assert [k for k, _, _ in assess.terms] == ["latent", "plated", "latent", "grouped", "observed", "reader"]
    ref, _ = _sweep(hip_ops, oracle_ops, "flat", 5, impl, 300, 3, seed=400 + impl)
    assert 0 < int(ref[4].sum()) < 300 * 3
    rng = np.random.default_rng(3)
    x, z = GR.columns("flat", 5, 300, rng)
    _, plan, _, _ = _case(hip_ops, oracle_ops, "flat", 5)
    lp_ref, ll_ref = assess(x, z)
    _, _, lp, ll, _, _ = hip_ops.temper_move_grouped(plan, _key(3, impl), _dev(x), _dev(z), None, None, 0.0, 0, recompute=True)
    assert _equal(lp.cpu().numpy(), lp_ref) and _equal(ll.cpu().numpy(), ll_ref)


def test_equal_to_the_unrolled_plan(hip_ops):
    """G = 2 as a grouped plan and as a plain tempered plan with a0, a1 as scalar latents and two plated sites over the split
    data.  Every row's term is the same f32 number in both.  The grouped ll is f32(acc_0 + acc_1), the float64 sum rounded
    ONCE; the unrolled ll is f32(f32(acc_0) + f32(acc_1)): three roundings.  Every term is negative here (a Normal of scale
    0.5 has log-density <= -0.226), so |acc_k| <= |total| and each rounding is at most half an ulp of the total: the two
    sum orders alone allow 1.5 + 0.5 = 2 ulps of |ll|.  The bound asserted is the tighter one the feature is specified to:
    ONE f32 rounding (one ulp) of the total."""
    half, n = 5, 1000
    target, g, off = GR.target("intercept", [half, half], seed=2)
    xs, ys = target.args[0], target.constraint.get_submap("y").get_value()

    @gen
    def unrolled(x0, x1):
        mu = normal(0.0, 2.0) @ "mu"
        b = normal(0.0, 2.0) @ "b"
        a0 = normal(mu, 0.7) @ "a0"
        a1 = normal(mu, 0.7) @ "a1"
        normal(a0 + b * x0, 0.5) @ "y0"
        normal(a1 + b * x1, 0.5) @ "y1"

    plain = Target(unrolled, (xs[:half].clone(), xs[half:].clone()), ChoiceMap.d({"y0": ys[:half].clone(), "y1": ys[half:].clone()}))
    rng = np.random.default_rng(5)
    x, z = GR.columns("intercept", 2, n, rng)
    key = _key(3, 1)
    with use_ops(hip_ops):
        tg, tp = temper.lower(target, 64), temper.lower(plain, 64)
        pg = hip_ops.temper_plan_create(tg.sites, keep=(tg.keep, tg))
        pg.set_data(tg.data_columns(hip_ops.device()))
        pg.set_groups(tg.group_offsets().to(hip_ops.device()))
        pp = hip_ops.temper_plan_create(tp.sites, keep=(tp.keep, tp))
        pp.set_data(tp.data_columns(hip_ops.device()))
        _, _, lp_g, ll_g, _, _ = hip_ops.temper_move_grouped(pg, key, _dev(x), _dev(z), None, None, 0.0, 0, recompute=True)
        _, lp_u, ll_u, _ = hip_ops.temper_move(pp, key, _dev(x + [z[0][0], z[0][1]]), None, None, 0.0, 0, None, recompute=True)
    ll_g, ll_u = ll_g.cpu().numpy(), ll_u.cpu().numpy()
    ulps = np.abs(ll_g.astype(np.float64) - ll_u.astype(np.float64)) / np.spacing(np.abs(ll_u)).astype(np.float64)
    print(f"|ll_grouped - ll_unrolled| in ulps of |ll|: max {ulps.max():.1f}, mean {ulps.mean():.2f}; bit-equal {np.mean(ulps == 0):.2f}")
    assert np.all(np.isfinite(ll_u)) and np.all(ll_u < 0) and ulps.max() <= 1.0
    # (lp: a sequential f32 sum of four terms against f32(lp_flat + f32(lpz_0 + lpz_1)): four roundings against three)
    ulps_lp = np.abs(lp_g.cpu().numpy().astype(np.float64) - lp_u.cpu().numpy().astype(np.float64)) / np.spacing(np.abs(lp_u.cpu().numpy())).astype(np.float64)
    print(f"|lp_grouped - lp_unrolled| in ulps of |lp|: max {ulps_lp.max():.1f}")


def _e2e_target(model, G=None):
    G = model.G if G is None else G
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    return Target(GR.body("intercept", G), (f(model.xs), torch.from_numpy(np.asarray(model.g, dtype=np.int64))), ChoiceMap.d({"y": f(model.ys)}))


def test_no_compilation_for_another_data_set(hip_ops):
    """After one run, a second target with other values, another g and another D compiles nothing; an in-place update of the
    group tensor between two runs of ONE sampler is seen."""
    key = genjax.random.key(77, "philox")
    with use_ops(hip_ops):
        first = GR.target("intercept", [3, 4, 5, 1, 9], seed=2)[0]
        TemperedSMC(first, 512, n_moves=1).run(key)
        before = hip_ops.jit_stats()["compiles"]
        target, g, _ = GR.target("intercept", [9, 0, 5, 4, 3], seed=4)
        alg = TemperedSMC(target, 512, n_moves=1)
        a = alg.run(key)
        assert hip_ops.jit_stats()["compiles"] == before
        b = alg.run(key)
        assert a.log_marginal_likelihood == b.log_marginal_likelihood and torch.equal(a.ll, b.ll) and torch.equal(a.choices["a"], b.choices["a"])
        target.args[1][8] = 1  # (in place: the last row of group 0 moves to the empty group 1; still sorted)
        c = alg.run(key)
        assert hip_ops.jit_stats()["compiles"] == before
        assert c.log_marginal_likelihood != a.log_marginal_likelihood and not torch.equal(a.ll, c.ll)


@pytest.fixture(scope="module")
def end_to_end(hip_ops):
    model = GR.e2e_model()
    with use_ops(hip_ops):
        alg = TemperedSMC(_e2e_target(model), 8192, n_moves=2, ess_target=0.5)
        key = genjax.random.key(2026, "philox")
        return model, alg, key, alg.run(key), alg.run(key)


def test_end_to_end_random_intercepts(end_to_end):
    """D = 200, G = 8, n = 8192, K = 2: log Z and the posterior means of mu, b and every a_g within FOUR TIMES the spread of
    the float64 restatement (tests/group_ref.py: measured on the CPU over 24 seeds); two runs from one key are bit-equal."""
    model, alg, key, a, b = end_to_end
    assert a.log_marginal_likelihood == b.log_marginal_likelihood and a.betas == b.betas and a.accept_rate == b.accept_rate
    assert a.accept_rate_groups == b.accept_rate_groups and torch.equal(a.lp, b.lp) and torch.equal(a.ll, b.ll)
    assert torch.equal(a.choices["a"], b.choices["a"]) and tuple(a.choices["a"].shape) == (model.G, 8192) and a.choices["a"].dtype == torch.float32
    assert a.choices["a"].is_cuda and tuple(a.choices["mu"].shape) == (8192,)
    means = np.concatenate([[a.choices["mu"].double().mean().item(), a.choices["b"].double().mean().item()],
                            a.choices["a"].double().mean(dim=1).cpu().numpy()])
    em = (means - model.post_mean) / model.post_sd
    ez = a.log_marginal_likelihood - model.log_z
    print(f"stages {len(a.betas) - 1}, accept {a.accept_rate}, group accept {a.accept_rate_groups}")
    print(f"log Z-hat {a.log_marginal_likelihood:.4f} against {model.log_z:.4f} (error {ez:+.4f}, bound {E2E_FACTOR * SPREAD_LOG_Z:.4f}); "
          f"mean errors / sd {np.round(em, 4).tolist()}; bounds {[round(E2E_FACTOR * s, 4) for s in SPREAD_MEAN]}")
    assert a.betas[0] == 0.0 and a.betas[-1] == 1.0 and all(y > x for x, y in zip(a.betas, a.betas[1:]))
    assert len(a.accept_rate_groups) == len(a.betas) - 1 and all(0.0 < r < 1.0 for r in a.accept_rate_groups)
    assert abs(ez) <= E2E_FACTOR * SPREAD_LOG_Z
    assert all(abs(e) <= E2E_FACTOR * s for e, s in zip(em, SPREAD_MEAN))


def test_launch_counts(hip_ops, oracle_ops, end_to_end):
    """A grouped move call is ONE kernel node of a captured graph, and a run makes one grouped move call per stage (plus the
    init / K = 0 fill of stage 0), no ungrouped one, and at most two ladder calls per stage."""
    n, G = 1000, 5
    _, plan, _, _ = _case(hip_ops, oracle_ops, "intercept", G)
    x, z = GR.columns("intercept", G, n, np.random.default_rng(1))
    dx, dz = _dev(x), _dev(z)
    key = genjax.random.key(4, "philox")
    anc = torch.arange(n, dtype=torch.int32).cuda()
    zsc = torch.full((1, G), 0.3, dtype=torch.float32).cuda()
    _, _, lp_d, ll_d, _, _ = hip_ops.temper_move_grouped(plan, key, dx, dz, None, None, 0.5, 0, recompute=True)  # (compiled before the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=side):
        out = hip_ops.temper_move_grouped(plan, key, dx, dz, lp_d, ll_d, 0.5, 2, (0.1, 0.1), zsc, ancestors=anc)
    nodes = _kernel_nodes(g.raw_cuda_graph())
    g.replay()
    torch.cuda.synchronize()
    del g, out
    assert nodes == 1
    model, alg, key, a, _ = end_to_end
    calls = {"grouped": 0, "move": 0, "ladder": 0}
    grouped, move, ladder = hip_ops.temper_move_grouped, hip_ops.temper_move, hip_ops.temper_ess_ladder

    def count(name, fn):
        def wrapped(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)
        return wrapped

    hip_ops.temper_move_grouped, hip_ops.temper_move, hip_ops.temper_ess_ladder = count("grouped", grouped), count("move", move), count("ladder", ladder)
    try:
        with use_ops(hip_ops):
            res = alg.run(key)
    finally:
        del hip_ops.temper_move_grouped, hip_ops.temper_move, hip_ops.temper_ess_ladder
    stages = len(res.betas) - 1
    assert res.betas == a.betas and calls["grouped"] == stages + 1 and calls["move"] == 0 and stages <= calls["ladder"] <= 2 * stages - 1
