"""Shared pieces of the parameterised-filter tests (test_smc_params_cpu.py, test_gpu_smc_params.py): the two models, each
once with declared parameters and once with the same numbers written as Python literals, theta rows, and the reference
every parity test is held to — the project's unchanged path: the LITERAL model on the CPU oracle (plain
gjx_smc_plan_create) under the same key."""

import math

import numpy as np
import torch

from genjax import ChoiceMapBuilder as C
from genjax import gen, gamma, normal
from genjax._amd import prng, workloads as W
from genjax._amd.runtime import use_ops
from genjax._amd.smc_fused import BootstrapSMC, StateSpaceModel

LGSSM_NAMES = ("a", "q", "r")
GAMMA_NAMES = ("m", "s", "k")


def f32s(theta) -> tuple:
    """A theta row as the Python floats a filter runs: rounded to f32 (what a literal model must be written with)."""
    return tuple(float(np.float32(v)) for v in theta)


# ---- (i) the LGSSM user model with theta = (a, q, r) -------------------------------------------------------------------
def lgssm_param_model() -> StateSpaceModel:
    """`a` in a mixed expression (a * x), `q` the direct scale of a latent site, `r` the direct scale of an observed one."""

    @gen
    def init(theta):
        a, q, r = theta
        x = normal(0.0, 1.0) @ "x"
        normal(x, r) @ "y"
        return x

    @gen
    def step(x, theta):
        a, q, r = theta
        x2 = normal(a * x, q) @ "x"
        normal(x2, r) @ "y"
        return x2

    return StateSpaceModel(init, step, params=LGSSM_NAMES)


def lgssm_literal_model(theta) -> StateSpaceModel:
    a, q, r = f32s(theta)

    @gen
    def init():
        x = normal(0.0, 1.0) @ "x"
        normal(x, r) @ "y"
        return x

    @gen
    def step(x):
        x2 = normal(a * x, q) @ "x"
        normal(x2, r) @ "y"
        return x2

    return StateSpaceModel(init, step)


def lgssm_rows(F: int) -> np.ndarray:
    """F distinct theta rows (a, q, r), all inside the support."""
    return np.asarray([(0.5 + 0.025 * f, 0.7 + 0.04 * f, 0.4 + 0.03 * f) for f in range(F)], dtype=np.float32)


# ---- (ii) a two-component carry with a Gamma latent, theta = (m, s, k) ---------------------------------------------------
def gamma_param_model() -> StateSpaceModel:
    """Parameters in the init body (a Normal's loc and scale, a Gamma's rate), host arithmetic on parameters (0.5 * s,
    s * s), a parameter against a traced value (k * x) and a parameter inside a carry expression (g2 * k + 0.1)."""

    @gen
    def init(theta):
        m, s, k = theta
        g = gamma(2.0, k) @ "g"
        x = normal(m, s) @ "x"
        normal(x, 0.5 * s) @ "y"
        return x, g

    @gen
    def step(c, theta):
        m, s, k = theta
        x, g = c
        g2 = gamma(3.0, 3.0 / g) @ "g"
        x2 = normal(k * x, s * s) @ "x"
        normal(x2, 0.5 * s) @ "y"
        return x2, g2 * k + 0.1

    return StateSpaceModel(init, step, params=GAMMA_NAMES)


def gamma_literal_model(theta) -> StateSpaceModel:
    m, s, k = f32s(theta)

    @gen
    def init():
        g = gamma(2.0, k) @ "g"
        x = normal(m, s) @ "x"
        normal(x, 0.5 * s) @ "y"
        return x, g

    @gen
    def step(c):
        x, g = c
        g2 = gamma(3.0, 3.0 / g) @ "g"
        x2 = normal(k * x, s * s) @ "x"
        normal(x2, 0.5 * s) @ "y"
        return x2, g2 * k + 0.1

    return StateSpaceModel(init, step)


def gamma_rows(F: int) -> np.ndarray:
    return np.asarray([(-0.3 + 0.05 * f, 0.8 + 0.03 * f, 0.6 + 0.02 * f) for f in range(F)], dtype=np.float32)


MODELS = {
    "lgssm": (lgssm_param_model, lgssm_literal_model, lgssm_rows),
    "gamma": (gamma_param_model, gamma_literal_model, gamma_rows),
}


def observations(T: int):
    """The project's LGSSM data recipe as the observed sequence of either model."""
    return C["y"].set(torch.as_tensor(W.lgssm_data(T), dtype=torch.float32))


# ---- the reference ---------------------------------------------------------------------------------------------------
def oracle_run(oracle_ops, literal_model: StateSpaceModel, obs, n: int, key, ess_threshold: float = 0.0, record_history=False):
    """The literal model's filter on the CPU oracle, ancestors recorded."""
    with use_ops(oracle_ops):
        return BootstrapSMC(literal_model, obs, n, record_ancestors=True, ess_threshold=ess_threshold,
                            record_history=record_history).run(key)


def columns(x) -> list:
    return list(x) if isinstance(x, tuple) else [x]


def assert_same_run(got, ref, what=""):
    """Tolerance 0: state columns, log-weights, ancestors, the (e, q) pairs, resampled flags, the log-marginal."""
    for k, (g, r) in enumerate(zip(columns(got.particles), columns(ref.particles))):
        assert torch.equal(g.cpu(), r.cpu()), f"{what}: state column {k}"
    assert torch.equal(got.log_weights.cpu(), ref.log_weights.cpu()), f"{what}: log-weights"
    assert torch.equal(got.step_e.cpu(), ref.step_e.cpu()) and torch.equal(got.step_q.cpu(), ref.step_q.cpu()), f"{what}: (e, q)"
    if ref.ancestors is not None and got.ancestors is not None:
        assert torch.equal(got.ancestors.cpu(), ref.ancestors.cpu()), f"{what}: ancestors"
    assert (got.resampled is None) == (ref.resampled is None), what
    if ref.resampled is not None:
        assert torch.equal(got.resampled.cpu(), ref.resampled.cpu()), f"{what}: resampled flags"
    assert got.log_marginal_likelihood == ref.log_marginal_likelihood, f"{what}: log-marginal"


def assert_runs_differ(x, y, what=""):
    """Every output of two filters differs (so a bank that served one row, or one key, to all of them cannot pass)."""
    for k, (g, r) in enumerate(zip(columns(x.particles), columns(y.particles))):
        assert not torch.equal(g.cpu(), r.cpu()), f"{what}: state column {k} coincides"
    assert not torch.equal(x.log_weights.cpu(), y.log_weights.cpu()), f"{what}: log-weights coincide"
    assert not torch.equal(x.step_q.cpu(), y.step_q.cpu()), f"{what}: step sums coincide"
    assert x.log_marginal_likelihood != y.log_marginal_likelihood, f"{what}: log-marginals coincide"
    if x.ancestors is not None and y.ancestors is not None:
        assert not torch.equal(x.ancestors.cpu()[1:], y.ancestors.cpu()[1:]), f"{what}: ancestors coincide"


def keys_for(impl: str, F: int, seed: int = 11):
    base = prng.key(seed, impl)
    return [prng.fold_in(base, f) for f in range(F)]


# ---- PMMH: the exact posterior of a in the LGSSM with q = 1, r = 0.5 --------------------------------------------------
def kalman_log_likelihood(a: float, y: np.ndarray, q: float = 1.0, r: float = 0.5) -> float:
    """float64 log p(y | a) of x_0 ~ N(0, 1), x_t ~ N(a x_{t-1}, q), y_t ~ N(x_t, r)."""
    mean, var, ll = 0.0, 1.0, 0.0
    for t, yt in enumerate(np.asarray(y, dtype=np.float64)):
        if t > 0:
            mean, var = a * mean, a * a * var + q * q
        s = var + r * r
        ll += -0.5 * (math.log(2.0 * math.pi * s) + (yt - mean) ** 2 / s)
        gain = var / s
        mean, var = mean + gain * (yt - mean), (1.0 - gain) * var
    return ll


def exact_posterior_mean_a(y: np.ndarray, points: int = 4001) -> float:
    """E[a | y] under the uniform prior on (-1, 1), by the float64 Kalman likelihood on a grid."""
    grid = np.linspace(-1.0, 1.0, points)
    ll = np.asarray([kalman_log_likelihood(a, y) for a in grid])
    w = np.exp(ll - ll.max())
    w[0] = w[-1] = 0.0  # (the open interval)
    return float((grid * w).sum() / w.sum())


def uniform_log_prior(theta) -> float:
    return 0.0 if -1.0 < float(theta[0]) < 1.0 else -math.inf


def lgssm_a_model() -> StateSpaceModel:
    """The LGSSM with theta = (a,), q = 1, r = 0.5."""

    @gen
    def init(theta):
        x = normal(0.0, 1.0) @ "x"
        normal(x, 0.5) @ "y"
        return x

    @gen
    def step(x, theta):
        (a,) = theta
        x2 = normal(a * x, 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    return StateSpaceModel(init, step, params=("a",))


def chains_criterion(samples: np.ndarray, exact: float, burn: int = 100):
    """-> (|mean over chains - exact|, 5 sd(chain means) / sqrt(C)): the self-normalised criterion of the PMMH tests."""
    means = samples[burn + 1:, :, 0].mean(axis=0)
    C_ = means.size
    return abs(float(means.mean()) - exact), 5.0 * float(means.std(ddof=1)) / math.sqrt(C_)
