"""Plated tempered plans on the GPU (include/gjx_plate.h): assess and the sweeps held bit for bit to the replay
tests/plate_ref.py builds from unchanged oracle entry points and a float64 row sum in numpy, the plated regression next to
the unrolled plan of the same data, no compilation for another data set, the sampler end to end against the closed form of
the conjugate regression with 500 rows, and the launch counts of a stage."""

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import temper_ref as R
from genjax import ChoiceMap, Target
from genjax._amd import temper
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from test_gpu_guided import _kernel_nodes
from plate_ref import E2E_FACTOR, SPREAD_LOG_Z, SPREAD_MEAN, SPREAD_SD

pytestmark = pytest.mark.gpu

NS = (1, 257, 1000)
DS = (1, 2, 63, 64, 65, 257)  # a lone row, remainders of any unroll or 64-row chunk, one past a 256-row staging chunk
SCALES = {"normal": (0.3, 0.3), "hetero": (0.3, 0.3), "logistic": (0.5, 0.5, 0.5), "gamma_rate": (0.5,)}


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


def _f32(t):
    return t.detach().to(torch.float32).numpy().copy()


@pytest.fixture(scope="module")
def lowered(hip_ops):
    """Per model: (tracer, plan) lowered once, from 20 rows — the plan knows no length: data of any D is set per case."""
    out = {}
    with use_ops(hip_ops):
        for name in P.MODELS:
            target, _ = P.target(name, 20)
            tracer = temper.lower(target, 64)
            plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            if tracer.params:
                plan.set_params(tracer.params)
            out[name] = (tracer, plan)
    return out


def _case(lowered, oracle_ops, name, D, inf_row=False):
    """Data of D rows for a model: set on the plan; -> (plan, the replay's assess)."""
    tracer, plan = lowered[name]
    _, data = P.target(name, max(D, 2), seed=1, inf_row=False)
    data = [_f32(t)[:D] for t in data]
    if inf_row and name != "logistic":
        data[-1][D // 2] = np.inf
    plan.set_data(_dev(data))
    return plan, P.Assess(oracle_ops, tracer, data)


@pytest.mark.parametrize("name", P.MODELS)
def test_assess_pin(hip_ops, oracle_ops, lowered, name):
    """K = 0, recompute = 1 on given latent columns: lp is temper_ref's composition, ll the oracle's per-row log-density
    summed in float64 in row order, rounded once to f32 and added — bit for bit, both generators, with a Gamma latent
    outside its support (lp = -inf; ll NaN there: a negative scale) and one +inf observed value (ll = -inf)."""
    rng = np.random.default_rng(11)
    for D in DS:
        for variant in ("plain", "edge"):
            edge = variant == "edge"
            if edge and name == "logistic":
                continue  # (no Gamma latent and no float value: nothing new)
            plan, assess = _case(lowered, oracle_ops, name, D, inf_row=edge)
            for n in NS:
                cols = P.columns(name, n, rng, outside=edge)
                lp_ref, ll_ref = assess(cols)  # (no draw is made: one reference for both generators)
                assert not np.isnan(lp_ref).any()
                if edge and name == "hetero" and n >= 4:
                    assert np.isneginf(lp_ref).sum() >= n // 4
                if edge and name in ("normal", "gamma_rate"):
                    assert np.all(np.isneginf(ll_ref) | np.isnan(ll_ref))
                for impl in (0, 1):
                    x, lp, ll, acc = hip_ops.temper_move(plan, genjax.random.key(3, "philox" if impl else "threefry"), _dev(cols),
                                                         None, None, 0.37, 0, None, recompute=True)
                    case = (name, D, n, impl, variant)
                    assert all(_same(a.cpu().numpy(), b) for a, b in zip(x, cols)), case
                    assert _equal(lp.cpu().numpy(), lp_ref), case
                    got = ll.cpu().numpy()
                    assert (_same if np.isnan(ll_ref).any() else _equal)(got, ll_ref), (case, got[:4], ll_ref[:4])
                    assert int(acc.sum()) == 0


def _ancestors(n, rng):
    a = rng.integers(0, max(1, n // 2), n).astype(np.int64)  # repeats
    wild = np.array([-1, n, n + 5, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)  # out-of-range words: they clamp to n - 1
    a[rng.permutation(n)[:len(wild)]] = wild
    return a.astype(np.int32)


@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("name", P.MODELS)
def test_sweep_pin(hip_ops, oracle_ops, lowered, name, impl):
    """K = 3 sweeps through an ancestors column with repeats and out-of-range words, over 65 rows (blocks and a remainder):
    x, lp, ll and n_accept are temper_ref.move_ref's with the plated assess, bit for bit, whatever the grid."""
    n, D, K, beta = 257, 65, 3, 0.37
    plan, assess = _case(lowered, oracle_ops, name, D)
    rng = np.random.default_rng(200 + impl)
    cols = P.columns(name, n, rng)
    lp0, ll0 = assess(cols)
    anc = _ancestors(n, rng)
    key = genjax.random.key(1000 + impl, "philox" if impl else "threefry")
    ref = R.move_ref(oracle_ops, assess, key, cols, lp0, ll0, beta, K, SCALES[name], ancestors=anc)
    assert 0 < int(ref[3].sum()) < n * K  # the replay accepts some proposals and rejects some
    for wg in (0, 1, 7):
        x, lp, ll, acc = hip_ops.temper_move(plan, key, _dev(cols), torch.from_numpy(lp0).cuda(), torch.from_numpy(ll0).cuda(), beta, K,
                                             SCALES[name], ancestors=torch.from_numpy(anc).cuda(), max_workgroups=wg)
        case = (name, impl, wg)
        assert np.array_equal(acc.cpu().numpy(), ref[3]), case
        assert all(_equal(a.cpu().numpy(), b) for a, b in zip(x, ref[0])), case
        assert _equal(lp.cpu().numpy(), ref[1]) and _equal(ll.cpu().numpy(), ref[2]), case


def _plated_regression(reg, noise=None):
    xs, ys = torch.tensor(reg.xs, dtype=torch.float32), torch.tensor(reg.ys, dtype=torch.float32)
    return Target(P.bodies()["normal"], (xs, reg.noise if noise is None else noise), ChoiceMap.d({"y": ys})), xs, ys


def test_against_the_unrolled_plan(hip_ops):
    """The README's regression (20 points) as the unrolled plan of temper_ref.models() and as ONE plated site over the same
    f32 data: the latents' lp is bit-equal; every row's term is the same f32 number in both, but the unrolled ll is their
    SEQUENTIAL F32 sum and the plated ll their float64 sum rounded once, so equality is not expected: they agree within
    D ulps of |ll|."""
    D, n = 20, 1000
    reg = R.Regression()
    rng = np.random.default_rng(5)
    cols = [(2.0 * rng.standard_normal(n)).astype(np.float32) for _ in range(2)]
    with use_ops(hip_ops):
        out = []
        for target in (R.models()["regression"], _plated_regression(reg)[0]):
            tr = temper.lower(target, 64)
            plan = hip_ops.temper_plan_create(tr.sites, keep=(tr.keep, tr))
            plan.set_params(tr.params)
            if tr.data:
                plan.set_data(_dev([_f32(t) for t in tr.data]))
            _, lp, ll, _ = hip_ops.temper_move(plan, genjax.random.key(3, "philox"), _dev(cols), None, None, 0.0, 0, None, recompute=True)
            out.append((lp.cpu().numpy(), ll.cpu().numpy()))
    (lp_u, ll_u), (lp_p, ll_p) = out
    assert _equal(lp_u, lp_p)
    ulps = np.abs(ll_p.astype(np.float64) - ll_u.astype(np.float64)) / np.spacing(np.abs(ll_u)).astype(np.float64)
    print(f"|ll_plated - ll_unrolled| in ulps of |ll|: max {ulps.max():.1f}, mean {ulps.mean():.2f}; bit-equal {np.mean(ulps == 0):.2f}")
    assert np.all(np.isfinite(ll_u)) and ulps.max() <= D


def test_no_compilation_for_another_data_set(hip_ops):
    """After one run, a second target with other values and another D compiles nothing; an in-place update of xs between
    two runs of ONE sampler changes the result."""
    key = genjax.random.key(77, "philox")
    with use_ops(hip_ops):
        first = P.target("normal", 40, seed=2)[0]
        TemperedSMC(first, 512, n_moves=1).run(key)
        before = hip_ops.jit_stats()["compiles"]
        target, data = P.target("normal", 333, seed=4)
        alg = TemperedSMC(target, 512, n_moves=1)
        a = alg.run(key)
        assert hip_ops.jit_stats()["compiles"] == before
        b = alg.run(key)
        assert a.log_marginal_likelihood == b.log_marginal_likelihood and torch.equal(a.ll, b.ll)
        data[0].mul_(0.5)  # xs, in place
        c = alg.run(key)
        assert hip_ops.jit_stats()["compiles"] == before
        assert c.log_marginal_likelihood != a.log_marginal_likelihood and not torch.equal(a.ll, c.ll)


@pytest.fixture(scope="module")
def end_to_end(hip_ops):
    model = P.conjugate(500)
    with use_ops(hip_ops):
        alg = TemperedSMC(_plated_regression(model)[0], 8192, n_moves=2, ess_target=0.5)
        key = genjax.random.key(2025, "philox")
        return model, alg, key, alg.run(key), alg.run(key)


def test_end_to_end_conjugate_regression(end_to_end):
    """D = 500, n = 8192, K = 2: log Z and the posterior mean and deviation of (w, b) within FOUR TIMES the spread of the
    float64 restatement (tests/plate_ref.py: measured on the CPU over 24 seeds); two runs from one key are bit-equal."""
    model, alg, key, a, b = end_to_end
    assert a.log_marginal_likelihood == b.log_marginal_likelihood and a.betas == b.betas and a.accept_rate == b.accept_rate
    assert torch.equal(a.lp, b.lp) and torch.equal(a.ll, b.ll) and all(torch.equal(u, v) for u, v in zip(a.columns, b.columns))
    sd = np.sqrt(np.diag(model.post_cov))
    w, bb = a.choices["w"].double(), a.choices["b"].double()
    em = [(w.mean().item() - model.post_mean[0]) / sd[0], (bb.mean().item() - model.post_mean[1]) / sd[1]]
    es = [w.std().item() / sd[0] - 1.0, bb.std().item() / sd[1] - 1.0]
    ez = a.log_marginal_likelihood - model.log_z
    print(f"stages {len(a.betas) - 1}, accept {a.accept_rate}")
    print(f"log Z-hat {a.log_marginal_likelihood:.4f} against {model.log_z:.4f} (error {ez:+.4f}, bound {E2E_FACTOR * SPREAD_LOG_Z:.4f}); "
          f"mean errors / sd {em[0]:+.4f} {em[1]:+.4f}; sd errors {es[0]:+.4f} {es[1]:+.4f}")
    assert a.betas[0] == 0.0 and a.betas[-1] == 1.0 and all(y > x for x, y in zip(a.betas, a.betas[1:]))
    assert abs(ez) <= E2E_FACTOR * SPREAD_LOG_Z
    assert all(abs(e) <= E2E_FACTOR * s for e, s in zip(em, SPREAD_MEAN))
    assert all(abs(e) <= E2E_FACTOR * s for e, s in zip(es, SPREAD_SD))


def test_end_to_end_logistic(hip_ops):
    """The logistic model on 200 rows runs to the end: a finite log Z, beta = 1, accept rates in (0, 1)."""
    target, _ = P.target("logistic", 200, seed=6)
    with use_ops(hip_ops):
        r = TemperedSMC(target, 4096, n_moves=2).run(genjax.random.key(8, "philox"))
        est = TemperedSMC(target, 4096, n_moves=2).log_marginal_likelihood_estimate(genjax.random.key(8, "philox"))
    print(f"logistic, 200 rows: log Z-hat {r.log_marginal_likelihood:.4f}, stages {len(r.betas) - 1}, accept {r.accept_rate}")
    assert np.isfinite(r.log_marginal_likelihood) and r.betas[-1] == 1.0 and all(0.0 < x < 1.0 for x in r.accept_rate)
    assert float(est) == float(np.float32(r.log_marginal_likelihood))
    assert -200 * np.log(2.0) < r.log_marginal_likelihood < 0.0  # better than coin flips, a probability of binary data


def test_launch_counts(hip_ops, oracle_ops, lowered, end_to_end):
    """As an unplated plan: a move call is ONE kernel node of a captured graph, and a run makes one move call per stage (plus
    the K = 0 fill of stage 0) and at most two ladder calls per stage."""
    n = 1000
    plan, assess = _case(lowered, oracle_ops, "normal", 65)
    cols = P.columns("normal", n, np.random.default_rng(1))
    dev = _dev(cols)
    key = genjax.random.key(4, "philox")
    anc = torch.arange(n, dtype=torch.int32).cuda()
    _, lp_d, ll_d, _ = hip_ops.temper_move(plan, key, dev, None, None, 0.5, 0, None, recompute=True)  # (compiled before the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, stream=side):
        out = hip_ops.temper_move(plan, key, dev, lp_d, ll_d, 0.5, 2, (0.1, 0.1), ancestors=anc)
    nodes = _kernel_nodes(g.raw_cuda_graph())
    g.replay()
    torch.cuda.synchronize()
    del g, out
    assert nodes == 1
    model, alg, key, a, _ = end_to_end
    calls = {"move": 0, "ladder": 0}
    move, ladder = hip_ops.temper_move, hip_ops.temper_ess_ladder

    def count(name, fn):
        def wrapped(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)
        return wrapped

    hip_ops.temper_move, hip_ops.temper_ess_ladder = count("move", move), count("ladder", ladder)
    try:
        with use_ops(hip_ops):
            res = alg.run(key)
    finally:
        del hip_ops.temper_move, hip_ops.temper_ess_ladder
    stages = len(res.betas) - 1
    assert res.betas == a.betas and calls["move"] == stages + 1 and stages <= calls["ladder"] <= 2 * stages - 1
