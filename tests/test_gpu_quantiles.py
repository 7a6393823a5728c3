"""Exact quantiles and moments of columns on the GPU (include/gjx_quantiles.h) against numpy on float64 copies of the same
columns, and TemperedSMC.summary against both."""

import numpy as np
import pytest
import torch

import genjax
import group_ref as GR
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PosteriorSummary, TemperedSMC

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.05, 0.5, 0.5, 0.999, 1.0)  # (the repeated 0.5: equal target bins merge)
KINDS = ("concentrated", "ties", "signed", "nans", "constant", "allnan")
BLOCKS = 16  # max_workgroups: 4 columns in one batch, min(ceil(4099 / 1024), 16 / 4) = 4 particle blocks at n = 4099
BATCHES = 3  # max_workgroups: two batches (3 columns, then 1) of one particle block


def _data(kind, n, rng):
    """f32 [4, n].  "signed": +-0 and denormals planted in every column, +-inf in column 0 alone (the other columns keep finite
    moments); "nans": the same with about 10 % NaNs."""
    if kind == "concentrated":  # one top-11-bit prefix: the wave peel, one slot
        return (1.0 + 0.2 * rng.random((4, n))).astype(np.float32)
    if kind == "ties":  # ranks fall inside runs of equal keys
        return rng.integers(0, 4, (4, n)).astype(np.float32)
    if kind == "constant":
        return np.full((4, n), 2.5, dtype=np.float32)
    if kind == "allnan":
        return np.full((4, n), np.nan, dtype=np.float32)
    v = (1e3 * rng.standard_normal((4, n))).astype(np.float32)
    v[:, (3 * np.arange(5)) % n] = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45], dtype=np.float32)
    v[0, (5 * np.arange(2) + 1) % n] = [np.inf, -np.inf]
    if kind == "nans":
        v[rng.random((4, n)) < 0.1] = np.nan
    return v


def _check(col, probs, bracket, quant, stats):
    """One column (f32 [n]) and its outputs (numpy: f32 [Q, 2], f64 [Q], f64 [5]) under the header's assertions."""
    p = np.asarray(probs, dtype=np.float64)
    x = np.sort(col[~np.isnan(col)])
    m = x.size
    assert stats[0] == col.size - m
    if m == 0:
        assert np.isnan(bracket).all() and np.isnan(quant).all() and np.isnan(stats[1:]).all()
        return
    h = (m - 1) * p
    lo = np.floor(h).astype(np.int64)
    ref = np.stack([x[lo], x[np.minimum(lo + 1, m - 1)]], axis=1)
    nz = ref != 0  # (numpy's sort does not order -0 and +0: those compare numerically)
    assert np.array_equal(bracket, ref) and np.array_equal(bracket.view(np.uint32)[nz], ref.view(np.uint32)[nz])
    assert stats[3] == x[0] and stats[4] == x[-1]
    x64 = x.astype(np.float64)
    for j in range(p.size):
        if bracket[j, 0] == bracket[j, 1]:
            assert quant[j] == np.float64(bracket[j, 0])
        if np.isfinite(bracket[j]).all():
            # one rounding each of h, the difference, the product and the sum against numpy's differently associated lerp
            assert abs(quant[j] - np.quantile(x64, p[j], method="linear")) <= 4.0 * np.spacing(np.float64(np.abs(bracket[j]).max()))
    if np.isfinite(x).all():
        mean = x64.mean()
        print(f"m = {m}: mean error {abs(stats[1] - mean):.3e} (bound {m * 2.0**-52 * np.abs(x64).mean():.3e})")
        assert abs(stats[1] - mean) <= m * 2.0**-52 * np.abs(x64).mean()
        if m < 2:
            assert np.isnan(stats[2])
        else:
            var = x64.var(ddof=1)
            assert abs(stats[2] - var) <= (m + 8) * 2.0**-52 * var


def _run(hip_ops, dev, probs, w):
    return [t.cpu().numpy() for t in hip_ops.column_quantiles([dev[:3], dev[3]], probs, max_workgroups=w)]


@pytest.mark.parametrize("w", [0, BLOCKS, BATCHES])
@pytest.mark.parametrize("n", [1, 2, 255, 257, 4099])
@pytest.mark.parametrize("kind", KINDS)
def test_column_quantiles(hip_ops, kind, n, w):
    """A [3, n] segment (at n = 4099, 257 and 255 two of its column bases are not 16-byte aligned) plus a one-column segment.
    n: one entry, two, below and above one 256-wide round of quads, several particle blocks under max_workgroups."""
    data = _data(kind, n, np.random.default_rng(1000 * KINDS.index(kind) + n))
    dev = torch.from_numpy(data).cuda()
    got = _run(hip_ops, dev, PROBS, w)
    for c in range(4):
        _check(data[c], PROBS, got[0][c], got[1][c], got[2][c])
    again = _run(hip_ops, dev, PROBS, w)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again))
    if w:  # the integer outputs do not depend on the split
        base = _run(hip_ops, dev, PROBS, 0)
        assert np.array_equal(got[0].view(np.uint32), base[0].view(np.uint32))
        assert np.array_equal(got[2][:, [0, 3, 4]].view(np.uint64), base[2][:, [0, 3, 4]].view(np.uint64))


@pytest.mark.parametrize("G", [1, 2])
def test_summary(hip_ops, G):
    """TemperedSMC.summary on the random-intercept model: the numpy reference on the columns of `choices`, and
    ops.column_quantiles called directly on the result's columns, bit for bit."""
    with use_ops(hip_ops):
        alg = TemperedSMC(GR.target("intercept", GR.LAYOUTS[G])[0], 512)
        res = alg.run(genjax.random.key(11, "philox"))
        got = alg.summary(res)
        listed = alg.summary([res.choices[a] for a in ("mu", "b", "a")], probs=(0.25,))
    assert isinstance(got, PosteriorSummary) and got.probs == (0.05, 0.5, 0.95) and list(got.mean) == ["mu", "b", "a"]
    bracket, quant, stats = hip_ops.column_quantiles([*res.columns, *res.group_columns], got.probs)
    at = 0
    for addr in ("mu", "b", "a"):
        cols = res.choices[addr].cpu().numpy().reshape(-1, 512)
        k = cols.shape[0]
        want = (G,) if addr == "a" else ()
        assert k == (G if addr == "a" else 1) and got.quantiles[addr].shape == (*want, 3) and got.mean[addr].shape == want
        assert listed.quantiles[addr].shape[-1] == 1 and got.mean[addr].dtype == torch.float64 and got.mean[addr].is_cuda
        assert torch.equal(got.quantiles[addr].reshape(k, 3), quant[at:at + k]) and torch.equal(got.brackets[addr].reshape(k, 3, 2), bracket[at:at + k])
        mine = torch.stack([d[addr].reshape(k) for d in (got.nan_count, got.mean, got.var, got.min, got.max)], dim=1)
        assert torch.equal(mine, stats[at:at + k]) and torch.equal(got.sd[addr].reshape(k), torch.sqrt(stats[at:at + k, 2]))
        for c in range(k):
            _check(cols[c], got.probs, got.brackets[addr].reshape(k, 3, 2)[c].cpu().numpy(), got.quantiles[addr].reshape(k, 3)[c].cpu().numpy(),
                   mine[c].cpu().numpy())
        at += k
