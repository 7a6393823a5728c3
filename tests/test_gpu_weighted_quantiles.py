"""Weighted quantiles and moments of columns on the GPU (include/gjx_quantiles.h, GJX_QUANTILES_WEIGHTED) against numpy on
integer masses, and SMCResult.summary / Trajectories.summary against both."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

import genjax
import paths_ref as P
from genjax._amd.runtime import use_ops
from genjax.inference.smc import BootstrapSMC, StateSummary

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.05, 0.5, 0.5, 0.999, 1.0)
KINDS = ("concentrated", "ties", "signed")
WEIGHTS = ("equal", "spread", "one", "tiny", "dead")
SPLITS = (0, 16, 3)  # max_workgroups: the library's split; 4 particle blocks at n = 4099; two batches (3 columns, then 1)
F = 31  # min(gjx_frac_bits(n), 31) for every n below 2^31


def _data(kind, n, rng):
    """f32 [4, n].  "signed": +-0 and denormals in every column, +-inf in column 0 alone, about 10 % NaNs."""
    if kind == "concentrated":  # one top-12-bit prefix: the wave peel, one slot
        return (1.0 + 0.05 * rng.random((4, n))).astype(np.float32)
    if kind == "ties":
        return rng.integers(0, 4, (4, n)).astype(np.float32)
    v = (1e3 * rng.standard_normal((4, n))).astype(np.float32)
    v[:, (3 * np.arange(5)) % n] = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45], dtype=np.float32)
    v[0, (5 * np.arange(2) + 1) % n] = [np.inf, -np.inf]
    v[rng.random((4, n)) < 0.1] = np.nan
    return v


def _weights(kind, n, rng):
    """f32 [2, n] log-weights."""
    lw = np.zeros((2, n), dtype=np.float32)
    if kind == "spread":
        lw = (3.0 * rng.standard_normal((2, n))).astype(np.float32)
    if kind == "one":
        lw[:] = -np.inf
        lw[[0, 1], rng.integers(0, n, 2)] = [-3.5, 7.25]
    if kind == "tiny":
        lw[:, ::2] = -100.0
    if kind == "dead":
        lw[:] = -np.inf
        lw[:, 1::2] = np.nan
    return lw


def _masses(raw, lw):
    """One weight column -> rint(exp_spec(lw - m) 2^F) as uint64, exp_spec the f32 exp of the specification."""
    ok = ~np.isnan(lw)
    m = lw[ok].max() if ok.any() else np.float32(-np.inf)
    with np.errstate(invalid="ignore"):
        d = np.ascontiguousarray(lw - m, dtype=np.float32)
    e = np.empty_like(d)
    raw.gjo_math(1, d.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_uint64(d.size))
    q = np.rint(e.astype(np.float64) * 2.0**F)
    q[~(lw > -np.inf)] = 0.0  # (NaN and -inf weigh nothing)
    assert q.max() <= 2.0**32 - 1
    return q.astype(np.uint64)


def _check(col, q, probs, quant, stats):
    """One column (f32 [n]), its masses (uint64 [n]) and its outputs (numpy: f32 [Q], f64 [6]) under the header's assertions."""
    ok = ~np.isnan(col)
    x, q = col[ok], q[ok]
    W = int(q.sum())
    assert stats[0] == col.size - x.size
    if W == 0:
        assert np.isnan(quant).all() and np.isnan(stats[1:]).all()
        return
    order = np.argsort(x, kind="stable")
    cum = np.cumsum(q[order], dtype=np.uint64)
    T = np.array([min(max(int(math.ceil(p * float(W))), 1), W) for p in probs], dtype=np.uint64)
    ref = x[order][np.searchsorted(cum, T, side="left")]
    nz = ref != 0  # (numpy's sort does not order -0 and +0: those compare numerically)
    assert np.array_equal(quant, ref) and np.array_equal(quant.view(np.uint32)[nz], ref.view(np.uint32)[nz])
    x, qf = x[q > 0].astype(np.float64), q[q > 0].astype(np.float64)
    assert stats[3] == x.min() and stats[4] == x.max()
    if np.isfinite(x).all():
        m, eps = x.size, 2.0**-52
        mean, ess = (qf * x).sum() / W, float(W) ** 2 / (qf * qf).sum()
        var = (qf * (x - mean) ** 2).sum() / W
        bound = (m + 2) * eps * (qf * np.abs(x)).sum() / W
        print(f"m = {m}: mean error {abs(stats[1] - mean):.3e} (bound {bound:.3e}), variance {abs(stats[2] - var):.3e} "
              f"({(m + 8) * eps * var:.3e}), ess {abs(stats[5] - ess):.3e} ({(m + 4) * eps * ess:.3e})")
        assert abs(stats[1] - mean) <= bound
        assert abs(stats[2] - var) <= (m + 8) * eps * var and abs(stats[5] - ess) <= (m + 4) * eps * ess


def _run(hip_ops, dev, lw, w):
    out = hip_ops.weighted_column_quantiles([dev[:3], dev[3]], lw, PROBS, max_workgroups=w, want_mass=True)
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("n", [1, 2, 255, 257, 4099])
@pytest.mark.parametrize("wkind", WEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
def test_weighted_column_quantiles(hip_ops, oracle_ops, kind, wkind, n):
    """A [3, n] segment (at odd n two of its column bases are not 16-byte aligned) plus a one-column segment, under one
    weight column and under two, at every split."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 100 * WEIGHTS.index(wkind) + n)
    data, lw = _data(kind, n, rng), _weights(wkind, n, rng)
    dev, dlw = torch.from_numpy(data).cuda(), torch.from_numpy(lw).cuda()
    q = np.stack([_masses(oracle_ops.lib._dll, lw[v]) for v in range(2)])
    for V in (1, 2):
        base = None
        for w in SPLITS:
            got = _run(hip_ops, dev, dlw[0] if V == 1 else dlw, w)
            assert np.array_equal(got[2].view(np.uint32), q[:V])
            for c in range(4):
                _check(data[c], q[c % V], PROBS, got[0][c], got[1][c])
                if wkind == "equal":  # sorted(valid)[ceil(p m) - 1], clamped
                    x = np.sort(data[c][~np.isnan(data[c])])
                    want = [x[min(max(math.ceil(p * x.size), 1), x.size) - 1] for p in PROBS] if x.size else [np.nan] * len(PROBS)
                    assert np.array_equal(got[0][c], np.array(want, dtype=np.float32), equal_nan=True)
            again = _run(hip_ops, dev, dlw[0] if V == 1 else dlw, w)
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))
            base = base or got
            assert np.array_equal(got[0].view(np.uint32), base[0].view(np.uint32)) and np.array_equal(got[2], base[2])
            assert np.array_equal(got[1][:, [0, 3, 4]].view(np.uint64), base[1][:, [0, 3, 4]].view(np.uint64))


@pytest.mark.parametrize("kind", ["lgssm", "ssm2"])
def test_summaries(hip_ops, oracle_ops, kind):
    """SMCResult.summary and Trajectories.summary: the library call on the same rows bit for bit, and the numpy reference row
    by row."""
    model, obs = P.model_and_obs(kind, 6)
    n, T, raw = 512, 6, oracle_ops.lib._dll
    with use_ops(hip_ops):
        res = BootstrapSMC(model, obs, n, record_history=True).run(genjax.random.key(5))
        filt, tr, eq = res.summary(), res.trajectories(), res.trajectories(genjax.random.key(6))
        smooth, lin = tr.summary(PROBS), eq.summary()
    cols, paths, K = P.as_cols(res.history), P.as_cols(tr.paths), len(P.as_cols(res.history))
    assert isinstance(filt, StateSummary) and filt.probs == (0.05, 0.5, 0.95) and filt.rule == smooth.rule == "inverted_cdf"
    assert lin.rule == "linear" and all(e is None for e in P.as_cols(lin.ess))
    lwh, lwf = res.log_weight_history.cpu().numpy(), res.log_weights.cpu().numpy()
    for s, segs, lw, probs in ((filt, cols, res.log_weight_history, filt.probs), (smooth, paths, res.log_weights, PROBS)):
        quant, stats = hip_ops.weighted_column_quantiles(list(segs), lw, probs)
        mine = [torch.stack([P.as_cols(a)[k] for a in (s.nan_count, s.mean, s.var, s.min, s.max, s.ess)], dim=1) for k in range(K)]
        assert torch.equal(torch.cat(mine), stats) and torch.equal(torch.cat(P.as_cols(s.quantiles)), quant)
        assert torch.equal(P.as_cols(s.sd)[0], torch.sqrt(stats[:T, 2])) and mine[0].dtype == torch.float64 and mine[0].is_cuda
        for k in range(K):
            for t in range(T):
                q = _masses(raw, lwh[t] if s is filt else lwf)
                _check(segs[k][t].cpu().numpy(), q, probs, P.as_cols(s.quantiles)[k][t].cpu().numpy(), mine[k][t].cpu().numpy())
    _, quant, stats = hip_ops.column_quantiles(list(P.as_cols(eq.paths)), lin.probs)
    assert torch.equal(torch.cat(P.as_cols(lin.quantiles)), quant) and torch.equal(torch.cat(P.as_cols(lin.mean)), stats[:, 1])
    assert torch.equal(torch.cat(P.as_cols(lin.var)), stats[:, 2]) and torch.equal(torch.cat(P.as_cols(lin.nan_count)), stats[:, 0])
