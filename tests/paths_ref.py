"""Shared by the history / trace-back tests (CPU and GPU): the filters of the test grid, the numpy reference of
include/gjx_paths.h, and the check of smoothing means against the exact smoother (backsim_ref.lgssm_rts)."""

import numpy as np
import torch

import genjax
from backsim_ref import lgssm_rts
from genjax import ChoiceMapBuilder as C, gen, normal
from genjax._amd import workloads as W
from genjax._amd.smc_fused import DiscreteHMM, LinearGaussianSSM, StateSpaceModel

T_GRID = 12
KINDS = ["lgssm", "hmm16", "ssm2"]
SIZES = [(1000, 0.0), (5000, 0.0), (3000, 0.5)]  # (n, ess_threshold): 5000 is no multiple of the tile


def model_and_obs(kind: str, T: int = T_GRID):
    if kind == "lgssm":
        return LinearGaussianSSM(), W.lgssm_data(T)
    if kind == "hmm16":
        trans, obs = W.hmm_tables(16)
        return DiscreteHMM(torch.from_numpy(trans), torch.from_numpy(obs), W.HMM["init_state"] % 16), W.hmm_data(T, 16)

    @gen
    def init():
        p = normal(0.0, 1.0) @ "p"
        v = normal(0.0, 0.5) @ "v"
        normal(p, 0.6) @ "y"
        return p, v

    @gen
    def step(c):
        p, v = c
        v2 = normal(0.9 * v - 0.1 * p, 0.3) @ "v"
        p2 = normal(p + 0.5 * v2, 0.2) @ "p"
        normal(p2, 0.6) @ "y"
        return p2, v2

    return StateSpaceModel(init, step), C["y"].set(torch.tensor(W.lgssm_data(T)))


def as_cols(x):
    return list(x) if isinstance(x, tuple) else [x]


def clamp(i, n: int):
    """min((uint32) i, n - 1)"""
    return np.minimum(np.asarray(i).astype(np.int32).view(np.uint32).astype(np.int64), n - 1)


def trace_ref(anc, cols, leaves, n: int):
    """The four lines of include/gjx_paths.h.  anc int32 [T, n]; cols: list of 4-byte [T, n] arrays; leaves int32[m] or
    None.  -> lineage int32 [T, m], paths (list of [T, m], the columns' dtypes, copied as bits), unique int64[T]
    (np.unique: meaningful as the kernel's count only for ordered leaves and monotone tables)."""
    anc = np.asarray(anc)
    T = anc.shape[0]
    lin = np.empty((T, n if leaves is None else len(leaves)), dtype=np.int64)
    lin[T - 1] = clamp(np.arange(n) if leaves is None else leaves, n)
    for t in range(T - 1, 0, -1):
        lin[t - 1] = clamp(anc[t][lin[t]], n)
    paths = [np.stack([np.asarray(c)[t].view(np.int32)[lin[t]] for t in range(T)]).view(np.asarray(c).dtype) for c in cols]
    unique = np.array([len(np.unique(lin[t])) for t in range(T)], dtype=np.int64)
    return lin.astype(np.int32), paths, unique


STAT_N, STAT_R, STAT_T = 200_000, 16, 8


def stat_keys(i: int):
    return genjax.random.key(1000 + i), genjax.random.key(5000 + i)


def check_smoothing_means(means):
    """means: [R, T] per-run smoothing means; the R-run average must lie within 4 standard errors (sample standard
    deviation over the runs / sqrt(R)) of the exact smoother, at every t.  -> the z scores."""
    means = np.asarray(means, dtype=np.float64)
    R = means.shape[0]
    exact = lgssm_rts(W.lgssm_data(STAT_T))[0]  # E[x_t | y_0:T-1]
    se = means.std(axis=0, ddof=1) / np.sqrt(R)
    z = (means.mean(axis=0) - exact) / se
    print("smoothing z scores:", np.round(z, 2), "standard errors:", se)
    assert np.all(np.abs(z) <= 4.0), z
    return z
