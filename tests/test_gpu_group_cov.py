"""Per-group covariance proposals on the GPU (include/gjx_group_cov.h): the two-launch moments against two-pass float64 numpy,
the block move at diagonal factors against the verified diagonal kernel bit for bit, and a full factor through the header's
f32 arithmetic."""

import numpy as np
import pytest
import torch

import genjax
import group_cov_ref as V
import group_ref as GR
from genjax._amd import abi, prng
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from genjax import ChoiceMap, Target

pytestmark = pytest.mark.gpu

SCALES = (0.3, 0.3)
_bits, _dev, _setup = V.bits, V.dev, V.slope_case


def _equal(a, b):
    """Integer views, tolerance 0."""
    return np.array_equal(_bits(a), _bits(b))


def _key(seed, impl):
    return genjax.random.key(seed, "philox" if impl else "threefry")


def _moments(hip_ops, z, lw, **kw):
    f, s, nd = hip_ops.temper_group_moments(_dev(z), None if lw is None else torch.from_numpy(lw).cuda(), **kw)
    return f.cpu().numpy(), s.cpu().numpy(), int(nd.cpu()[0])


def _full(f, S):
    """Packed [G, S (S + 1) / 2] -> [G, S, S] (row-major: the header's packing)."""
    full = np.zeros((f.shape[0], S, S), dtype=np.float32)
    full[:, np.tril_indices(S)[0], np.tril_indices(S)[1]] = f
    return full


def _within_4_ulps(got, ref):
    """Every entry of the f32 rows `got` within 4 f32 ulps of the largest entry of its row of `ref` (rows: the last axis)."""
    top = np.abs(ref).max(axis=-1, keepdims=True).astype(np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - ref) <= 4.0 * np.spacing(top).astype(np.float64)))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 3000])
@pytest.mark.parametrize("G", [1, 5, 17])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_moments(hip_ops, S, G, n, weighted):
    """Factor and scales against the two-pass float64 reference: the float64 sums differ by about 1e-11 relative (the weights
    are exact but for the f32 exp's own rounding, tests/group_cov_ref.py inputs), so the f32 cast is the visible rounding:
    4 f32 ulps of the row's largest entry.  n: one lane, below and above one 256-wide round, several blocks.  The result does
    not depend on the grid."""
    if n == 3000:
        assert hip_ops.lib.call("gjx_temper_ladder_blocks", n) >= 2
    z, lw = V.inputs(S, G, n, 100 * S + G, weighted)
    f, sc, nd = _moments(hip_ops, z, lw)
    rf, rs = V.moments_ref(z, lw)
    assert f.shape == (G, S * (S + 1) // 2) and sc.shape == (S, G)
    full = _full(f, S)
    assert _within_4_ulps(full, rf), (np.abs(full - rf).max(), np.abs(rf).max())
    assert _within_4_ulps(sc, rs), (np.abs(sc - rs).max(), np.abs(rs).max())
    assert nd == (S * G if n == 1 else 0)
    f3, sc3, nd3 = _moments(hip_ops, z, lw, max_workgroups=3)
    assert np.array_equal(_bits(f), _bits(f3)) and np.array_equal(_bits(sc), _bits(sc3)) and nd3 == nd


def test_moments_exact_cases(hip_ops):
    """A constant column is a fallback row (zeros: the component stays put) and is counted exactly; the rest of that group is
    the factor of the remaining component.  Weights that are all -inf: a zero factor, zero scales, S rows per group."""
    S, G, n = 2, 3, 257
    z, lw = V.inputs(S, G, n, 7, True)
    z[1][1, :] = np.float32(3.25)
    f, sc, nd = _moments(hip_ops, z, lw)
    rf, _ = V.moments_ref([z[0]], lw)  # (S = 1: c = 2.38, the kernel's 2.38 / sqrt(2))
    assert nd == 1 and f[1, 1] == 0.0 and f[1, 2] == 0.0 and sc[1, 1] == 0.0
    assert _within_4_ulps(f[1:2, 0:1], rf[1, :, 0:1] / np.sqrt(2.0))
    assert np.all(f[[0, 2]][:, [0, 2]] > 0)
    f, sc, nd = _moments(hip_ops, z, np.full(n, -np.inf, dtype=np.float32))
    assert nd == S * G and not f.any() and not sc.any()


def test_moments_largest_block(hip_ops):
    """The last shape the launch takes but 37: per = 16000 (64 000 bytes of LDS), 256 blocks, a shorter last block."""
    n = abi.GROUP_MOMENTS_MAX_N - 37
    z, lw = V.inputs(2, 2, n, 5, True)
    f, sc, nd = _moments(hip_ops, z, lw)
    rf, rs = V.moments_ref(z, lw)
    assert nd == 0 and _within_4_ulps(_full(f, 2), rf) and _within_4_ulps(sc, rs)
    with pytest.raises(ValueError, match="out of range"):
        hip_ops.temper_group_moments_workspace(abi.GROUP_MOMENTS_MAX_N + 1, 2, 2)


def test_block_route_end_to_end(hip_ops, monkeypatch):
    """TemperedSMC(proposal="block") on the intercept-and-slope model with x in [2, 3] (D = 200, G = 8, n = 4096, K = 2, PHILOX)
    against the exact Gaussian posterior: log Z, every posterior mean and the variance ratios of a_g, c_g within FOUR TIMES the
    root-mean-square error of the float64 restatement (tests/group_cov_ref.py: 24 seeds on the CPU), the last stage's group
    accept rate at least half the smallest the restatement saw.  A stage calls neither group_scales nor population_scales
    (both raise here); two runs from one key are bit-equal."""
    def refuse(*a, **k):
        raise AssertionError("a torch scale route was called under proposal=\"block\"")

    monkeypatch.setattr(TemperedSMC, "group_scales", staticmethod(refuse))
    monkeypatch.setattr(TemperedSMC, "population_scales", staticmethod(refuse))
    m = V.e2e_model()
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    with use_ops(hip_ops):
        target = Target(GR.body("slope", m.G), (f(m.xs), torch.from_numpy(m.g.astype(np.int64))), ChoiceMap.d({"y": f(m.ys)}))
        alg = TemperedSMC(target, 4096, n_moves=2, ess_target=0.5, proposal="block")
        res, again = alg.run(genjax.random.key(2027, "philox")), alg.run(genjax.random.key(2027, "philox"))
    assert res.log_marginal_likelihood == again.log_marginal_likelihood and torch.equal(res.group_factor, again.group_factor)
    assert all(torch.equal(a, b) for a, b in zip(res.group_columns, again.group_columns))
    stages = len(res.betas) - 1
    assert tuple(res.group_factor.shape) == (m.G, 2, 2) and tuple(res.factor.shape) == (2, 2) and bool((res.group_factor[:, 0, 1] == 0).all())
    assert len(res.n_degenerate) == len(res.n_degenerate_groups) == len(res.accept_rate_groups) == stages and res.n_degenerate_groups[-1] == 0
    col = lambda addr: res.choices[addr].double().cpu().numpy()
    ez, em, vr, rate = V.e2e_errors(m, res.log_marginal_likelihood, col("mu"), col("b"), col("a"), col("c"), res.accept_rate_groups[-1])
    print(f"stages {stages}; log Z error {ez:+.4f} (bound {V.E2E_FACTOR * V.RMS_LOG_Z:.4f}); mean errors / sd {np.round(em, 3).tolist()}; "
          f"variance ratios {np.round(vr, 3).tolist()}; last group accept rate {rate:.4f} (floor {0.5 * V.MIN_LAST_RATE:.4f})")
    assert abs(ez) <= V.E2E_FACTOR * V.RMS_LOG_Z
    assert all(abs(e) <= V.E2E_FACTOR * s for e, s in zip(em, V.RMS_MEAN))
    assert all(abs(r - 1.0) <= V.E2E_FACTOR * s for r, s in zip(vr, V.RMS_VAR_RATIO))
    assert rate >= 0.5 * V.MIN_LAST_RATE


@pytest.mark.parametrize("impl", [0, 1])
def test_diagonal_factor_is_the_grouped_kernel(hip_ops, oracle_ops, impl):
    """slope over the layout with empty groups, n = 300, K = 2, permuted ancestors: diagonal factor_z (and then a diagonal
    factor_x) against gjx_temper_move_grouped with the same scales, every output bit for bit.  No draw and no latent is a
    zero (asserted): the only values at which +0 + z and a zero off-diagonal product could show."""
    n, K, G, S, L = 300, 2, 17, 2, 2
    plan, rng, x, z, lp, ll, anc = _setup(hip_ops, oracle_ops, 31)
    zs, key = rng.uniform(0.2, 0.6, (S, G)).astype(np.float32), _key(9, impl)
    for r in range(K):
        kr = prng.fold_in(key, r)
        keys = [prng.fold_in(kr, 0)] + [prng.fold_in(prng.fold_in(prng.fold_in(kr, 2), g), 0) for g in range(G)]
        assert all(np.all(e != 0) for k in keys for e in V.draws(oracle_ops, k, S, n))  # (L == S: one count serves both)
    args = (plan, key, _dev(x), _dev(z), torch.from_numpy(lp).cuda(), torch.from_numpy(ll).cuda(), 0.6, K)
    a = torch.from_numpy(anc).cuda()
    ref = hip_ops.temper_move_grouped(*args, SCALES, torch.from_numpy(zs).cuda(), ancestors=a)
    fz = torch.from_numpy(np.stack([zs[0], 0 * zs[0], zs[1]], axis=1)).cuda()  # packed diagonal factors [G, 3]
    fx = torch.tensor([SCALES[0], 0.0, SCALES[1]], dtype=torch.float32).cuda()
    assert int(ref[5].sum()) > 0 and int(ref[4].sum()) > 0
    for got in (hip_ops.temper_move_grouped_cov(*args, fz, None, SCALES, ancestors=a), hip_ops.temper_move_grouped_cov(*args, fz, fx, ancestors=a)):
        for c, d in zip(got[0] + got[1], ref[0] + ref[1]):
            assert np.all(c.cpu().numpy() != 0) and _equal(c.cpu().numpy(), d.cpu().numpy())
        assert _equal(got[2].cpu().numpy(), ref[2].cpu().numpy()) and _equal(got[3].cpu().numpy(), ref[3].cpu().numpy())
        assert torch.equal(got[4], ref[4]) and torch.equal(got[5], ref[5])


@pytest.mark.parametrize("impl", [0, 1])
def test_full_factor_moves_through_the_spec(hip_ops, oracle_ops, impl):
    """K = 1, full lower-triangular factors: every output entry is the gathered old value or the replayed f32 proposal, the
    components of a group (and the scalars) move together, n_accept_z counts the groups that moved, and (lp, ll) are a
    recompute launch on the outputs."""
    n, G, S, L = 300, 17, 2, 2
    plan, rng, x, z, lp, ll, anc = _setup(hip_ops, oracle_ops, 32)
    fz = (rng.uniform(0.1, 0.4, (G, 3)) * rng.choice([-1.0, 1.0], (G, 3))).astype(np.float32)
    fx = np.array([0.2, -0.15, 0.25], dtype=np.float32)
    key = _key(13, impl)
    xo, zo, lpo, llo, acc, accz = hip_ops.temper_move_grouped_cov(
        plan, key, _dev(x), _dev(z), torch.from_numpy(lp).cuda(), torch.from_numpy(ll).cuda(), 0.6, 1, torch.from_numpy(fz).cuda(),
        torch.from_numpy(fx).cuda(), ancestors=torch.from_numpy(anc).cuda())
    kr = prng.fold_in(key, 0)

    def moved(out, old, new):  # per particle: did the block move?  Every component is the old or the new value, together
        o = [_bits(c) for c in out]
        stay = np.all([a == _bits(b) for a, b in zip(o, old)], axis=0)
        go = np.all([a == _bits(b) for a, b in zip(o, new)], axis=0)
        assert np.all(stay | go) and not np.any(stay & go)
        return go

    old = [c[anc] for c in x]
    mx = moved([c.cpu().numpy() for c in xo], old, V.propose(old, fx, V.draws(oracle_ops, prng.fold_in(kr, 0), L, n)))
    assert np.array_equal(mx.astype(np.int32), acc.cpu().numpy()) and 0 < mx.sum() < n
    count = np.zeros(n, dtype=np.int32)
    zo_np = [c.cpu().numpy() for c in zo]
    for g in range(G):
        old = [c[g][anc] for c in z]
        eps = V.draws(oracle_ops, prng.fold_in(prng.fold_in(prng.fold_in(kr, 2), g), 0), S, n)
        count += moved([c[g] for c in zo_np], old, V.propose(old, fz[g], eps))
    assert np.array_equal(count, accz.cpu().numpy()) and 0 < count.sum() < n * G
    _, _, lp2, ll2, _, _ = hip_ops.temper_move_grouped_cov(plan, key, xo, zo, None, None, 0.6, 0, None, recompute=True)
    assert _equal(lp2.cpu().numpy(), lpo.cpu().numpy()) and _equal(ll2.cpu().numpy(), llo.cpu().numpy())
