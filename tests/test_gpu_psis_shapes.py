"""PSIS-LOO on the GPU where the loops of its kernels run MORE THAN ONCE (include/gjx_psis.h; the checks are those of
tests/test_gpu_psis.py: the tail bit for bit, s, tT and bad exact, B within its derived bound, the fit at a stated multiple of
the reference's own reordering noise, two calls equal bit for bit).  Every case of test_gpu_psis.py walks a chunk of
particles in ONE round of 256 and sorts at most 256 keys (tests/test_psis_cpu.py asserts that); here:

  trips      chunks of more than 256 particles (a lane's float64 sum holds several terms, a lane adds to the histogram and
             appends keys several times per row, a last round with one live lane), a short last chunk, an EMPTY last chunk,
             a row block with a row switched off;
  tails      tail lengths M = 255 .. 4095: the bitonic network over 256 .. 4096 keys with and without padding slots, per-lane
             sums of several terms in the fit, 45 .. 93 candidates; a tail that is the whole row; NaN keys among the sorted;
  keys       rows whose keys share their top 22 bits (select passes 0 and 1 see one bin), a tail that crosses the sign
             boundary of the key, per-particle -inf entries (fewer and more than the tail), a heavy tie block across the cutoff;
  public     TemperedSMC.loo(columns) at n = 20000 (M = 425) against the closed-form leave-one-out.

The geometry each case is named for is asserted in tests/test_psis_cpu.py from psis_ref.chunks / trips / empty_chunks /
sort_size (written from the headers' text), the property of each crafted population on the REFERENCE's terms both there and
here.  The key-space classes set the `normal` model's data to xs = 0 on the crafted rows: the row's term then depends on
the intercept b alone.  A +inf term is NOT reachable through a model of plate_ref and is left out: the Normal and Bernoulli
log-densities are bounded above (fixed or data scale, probabilities), and where a Normal scale or a Gamma value reaches 0 or
+inf the +inf part of the log-density meets a -inf part of the same term, which is NaN — the class test_non_finite_entries and
the `outside` case below cover.  No shape had to shrink: the slowest case (n = 4099, D = 1100: 1100 oracle runs for the
replay) takes about a second, the module under ten (profiles/psis_summary.md has the times and the measured noise)."""

import time

import numpy as np
import pytest
import torch

import plate_ref as P
import pointwise_ref as W
import psis_ref as S
from genjax import ChoiceMap, Target
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PSISLOO, TemperedSMC
from test_gpu_psis import _check, _run, case_data, lower_all, population

pytestmark = pytest.mark.gpu

# ---- the cases (tests/test_psis_cpu.py asserts the geometry named here on psis_ref's restatement of the chunk rule) -------------
# (model, n, D, population) -> W chunks of `per` particles, `trips` rounds of 256 of which the last has `last` live lanes in a
# full chunk, `short`: the particles of the last chunk that is not empty, `empty` chunks, tail length M, P sorted keys
TRIP_CASES = [("normal", 4099, 1100, "centred"), ("two_plate", 6000, 700, "dup"), ("normal", 526000, 3, "centred"),
              ("gamma_rate", 20000, 300, "centred")]
TRIP_GEOMETRY = {
    (4099, 1100): dict(W=8, per=513, trips=3, last=1, short=508, empty=0, M=193, P=256),
    (6000, 700): dict(W=12, per=500, trips=2, last=244, short=500, empty=0, M=233, P=256),
    (526000, 3): dict(W=2048, per=257, trips=2, last=1, short=178, empty=1, M=2176, P=4096),
    (20000, 300): dict(W=28, per=715, trips=3, last=203, short=695, empty=0, M=425, P=512),
}
# the `normal` model, D = 5, centred: (n, M) -> (P, padding slots P - (M + 1), Gn)
TAIL_N, TAIL_D = 4200, 5
TAIL_CASES = {(4200, 255): (256, 0, 45), (4200, 256): (512, 255, 46), (4200, 257): (512, 254, 46), (4200, 1000): (1024, 23, 61),
              (4200, 2047): (2048, 0, 75), (4200, 2048): (4096, 2047, 75), (4200, 4095): (4096, 0, 93), (4096, 4095): (4096, 0, 93)}
# `hetero` with every fourth Gamma latent outside its support, n chosen so that fewer than M + 1 entries of a row are not NaN
OUTSIDE_N, OUTSIDE_M = 1200, 1000
# the key-space classes, each at (n, M) = (4096, 192) — the package's rule — and (6000, 1000)
KEY_KINDS = ("one_bin", "sign", "ninf_few", "ninf_many", "tie")
KEY_SIZES = ((4096, 192), (6000, 1000))
KEY_D = 8
CRAFTED = (0, 2, 3, 5, 6)  # rows with xs = 0 (both row blocks hold some), observed at Y0 + 2.5e-5 * (position in this list)
Y0 = -0.3
NINF = {("ninf_few", 192): 50, ("ninf_many", 192): 300, ("ninf_few", 1000): 50, ("ninf_many", 1000): 1200}
PUBLIC_N, PUBLIC_ROWS, PUBLIC_SEED = 20000, 40, 7000


def trip_columns(case):
    name, n, _, kind = case
    return population(name, n, kind, np.random.default_rng(41))


def tail_columns(n):
    return population("normal", n, "centred", np.random.default_rng(42))


def outside_columns():
    return P.columns("hetero", OUTSIDE_N, np.random.default_rng(43), outside=True)


def key_case(lowered, kind, n, M):
    """-> (latent columns (w, b), data columns in the plan's order) of a key-space class."""
    rng = np.random.default_rng(44)
    data = [np.array(c, dtype=np.float32) for c in case_data(lowered, "normal", KEY_D)]
    order = lowered["normal"][2]  # (positions in (xs, ys))
    xs, ys = data[order.index(0)], data[order.index(1)]
    for q, r in enumerate(CRAFTED):
        xs[r], ys[r] = 0.0, Y0 + 2.5e-5 * q
    w = (0.7 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    if kind == "one_bin":  # within 6e-4 of the observed values: the term is within ~150 f32 ulps of its maximum
        b = Y0 + 5e-4 * rng.uniform(-1.0, 1.0, n)
    elif kind == "sign":  # the term is 0 at |y - b| = 0.166: about 4 % of this population is beyond (fewer than M + 1)
        b = Y0 + 0.08 * rng.standard_normal(n)
    elif kind in ("ninf_few", "ninf_many"):  # ((y - b) / 0.1)^2 overflows f32 at b = 3e19
        b = Y0 + 0.05 * rng.standard_normal(n)
        b[rng.choice(n, NINF[kind, M], replace=False)] = 3e19
    else:  # tie: one particle at 2.4 deviations n // 3 times, fewer than M - 100 of the others beyond it
        b = Y0 + 0.05 * rng.standard_normal(n)
        at = rng.choice(n, n // 3, replace=False)
        b[at], w[at] = Y0 + 0.12, 0.7
    return [w, np.asarray(b, dtype=np.float32)], data


def key_property(kind, t, M):
    """The property a key-space class is named for, asserted on the reference's terms t [KEY_D, n]."""
    k = S.keys(t)
    rows = list(CRAFTED)
    sel = [S.select(t[d], M) for d in range(len(t))]
    if kind == "one_bin":
        one = [d for d in range(len(t)) if len(np.unique(k[d] >> 10)) == 1]
        assert len(one) >= 4 and all(len(np.unique(k[d])) < t.shape[1] // 4 for d in one), one
    elif kind == "sign":
        hit = [d for d in rows if sel[d][0][0] < 0.0 < sel[d][0][M - 1] and (S.keys(sel[d][0][M:])[0] >> 21) != (S.keys(sel[d][0][:1])[0] >> 21)]
        assert hit, kind
    elif kind in ("ninf_few", "ninf_many"):
        n_inf = NINF[kind, M]
        assert np.all(np.isneginf(t).sum(axis=1) == n_inf) and np.all((~np.isfinite(t)).sum(axis=1) == n_inf)
        assert n_inf < M if kind == "ninf_few" else n_inf > M + 1
        assert all(np.isneginf(tail[M]) == (kind == "ninf_many") for tail, _ in sel)
    else:
        assert all(M - sel[d][1] >= 100 and (k[d] == S.keys(sel[d][0][M:])[0]).sum() >= t.shape[1] // 3 for d in rows), kind
        assert all((k[d] <= S.keys(sel[d][0][M:])[0]).sum() > M + 1 for d in rows)  # (the block goes on past the cutoff)


@pytest.fixture(scope="module")
def lowered(hip_ops):
    return lower_all(hip_ops)


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    print(f"[time] {request.node.name}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("case", TRIP_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_trips(hip_ops, oracle_ops, lowered, case):
    name, n, D, kind = case
    out, tail, t, M = _run(hip_ops, oracle_ops, lowered, name, D, trip_columns(case))
    assert np.isfinite(t).all() and M == TRIP_GEOMETRY[n, D]["M"]
    ref = _check(out, tail, t, M, case, S.TOL_LARGE)
    if kind == "dup":  # (the cutoff is tied on some row)
        k = S.keys(t)
        assert any((k[d] == S.keys(ref["tail"][d, M:])[0]).sum() > 1 for d in range(D)), case


@pytest.mark.parametrize("case", sorted(TAIL_CASES), ids=lambda c: f"n{c[0]}-M{c[1]}")
def test_tail_lengths(hip_ops, oracle_ops, lowered, case):
    n, M = case
    out, tail, t, _ = _run(hip_ops, oracle_ops, lowered, "normal", TAIL_D, tail_columns(n), M=M)
    ref = _check(out, tail, t, M, case, S.TOL_LARGE)
    assert np.isfinite(ref["khat"]).any() and np.array_equal(np.isfinite(out[1]), np.isfinite(ref["khat"])), case
    if n - M == 1:  # the tail is the whole row: the body is the maximum alone, whatever is tied with it (G - ties = 1)
        assert np.array_equal(np.sort(t, axis=1), tail) and np.all(ref["B"] == 1.0)


def test_tail_with_nan_keys(hip_ops, oracle_ops, lowered):
    """Fewer than M + 1 entries of a row are numbers: the sorted tail ends in NaN keys (next to the 23 padding slots)."""
    out, tail, t, M = _run(hip_ops, oracle_ops, lowered, "hetero", TAIL_D, outside_columns(), M=OUTSIDE_M)
    ref = _check(out, tail, t, M, "outside", S.TOL_LARGE)
    assert np.all(np.isnan(ref["tail"][:, M])) and np.all(np.isnan(ref["tail"]).sum(axis=1) > 1) and np.all(ref["bad"] > 0)
    assert np.isnan(out[0]).all() and np.all(np.isposinf(out[1])) and np.isnan(out[4]).all()


@pytest.mark.parametrize("size", KEY_SIZES, ids=lambda s: f"n{s[0]}-M{s[1]}")
@pytest.mark.parametrize("kind", KEY_KINDS)
def test_key_space(hip_ops, oracle_ops, lowered, kind, size):
    n, M = size
    cols, data = key_case(lowered, kind, n, M)
    out, tail, t, _ = _run(hip_ops, oracle_ops, lowered, "normal", KEY_D, cols, data, M=M)
    key_property(kind, t, M)
    ref = _check(out, tail, t, M, (kind, n, M), S.TOL_LARGE)
    if kind.startswith("ninf"):
        assert np.all(out[6] == NINF[kind, M]) and np.all(np.isposinf(out[1])) and np.isnan(out[0]).all() and np.isnan(out[2]).all()
        assert np.all(np.isneginf(out[3])) and np.array_equal(np.isneginf(out[4]), np.full(KEY_D, kind == "ninf_many"))
    else:
        assert np.all(ref["bad"] == 0) and np.isfinite(out[0]).all()


def test_public_call_at_a_production_tail(hip_ops, oracle_ops, lowered):
    """TemperedSMC.loo(columns) on the conjugate regression with 40 rows under 20000 draws from its exact posterior (M = 425,
    two rounds of sorting per lane, a chunk per 256 particles): the table is the one `_check` holds to the reference on the
    replayed terms, and sum_d elpd_loo_d is within four times the reference's own spread of the closed form."""
    model = P.conjugate(PUBLIC_ROWS)
    n = PUBLIC_N
    cols = W.posterior_columns(model, n, PUBLIC_SEED)
    xs, ys = torch.tensor(model.xs, dtype=torch.float32), torch.tensor(model.ys, dtype=torch.float32)
    given = [xs.numpy(), ys.numpy()]
    data = [given[k] for k in lowered["normal"][2]]
    out, tail, t, M = _run(hip_ops, oracle_ops, lowered, "normal", PUBLIC_ROWS, cols, data)
    ref = _check(out, tail, t, M, "public", S.TOL_LARGE)
    assert ref["khat"].max() <= 0.7 and np.all(ref["bad"] == 0)
    with use_ops(hip_ops):
        alg = TemperedSMC(Target(P.bodies()["normal"], (xs, model.noise), ChoiceMap.d({"y": ys})), 64)
        loo = alg.loo([torch.from_numpy(c).cuda() for c in cols])
    assert isinstance(loo, PSISLOO) and loo.tail_len == S.tail_len(n) == M == 425 and loo.n == n
    for q, v in ((0, loo.elpd_loo), (1, loo.khat), (2, loo.sigma), (6, loo.bad)):  # (the order of every sum is a function of (n, D, M))
        assert v.shape == (PUBLIC_ROWS,) and np.array_equal(v.cpu().numpy().view(np.int64), out[q].view(np.int64)), q
    exact = S.closed_form_loo(model).sum()
    bound = S.CLOSED_FORM_FACTOR * S.SPREAD_ELPD_SUM_20000
    print(f"elpd {loo.elpd:.5f} against {exact:.5f} (error {loo.elpd - exact:+.5f}, bound {bound:.5f}); largest khat {float(loo.khat.max()):.3f}")
    assert abs(loo.elpd - exact) <= bound and loo.n_high == 0 and loo.khat_threshold == 0.7
