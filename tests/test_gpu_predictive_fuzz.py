"""The predictive kernels with SEVERAL plated sites on the GPU (include/gjx_predictive.h), against laws that share nothing with
the lowering (tests/temper_fuzz.py predictive_laws).

The fixed `interleaved` body — four plated sites (Normal, Gamma, flip, Beta), latents declared between them, a plate's value read
as data — and random bodies run through gjx_temper_predictive at the very seeds, keys, sizes and bodies whose replay
tests/test_predictive_fuzz_cpu.py has held to the laws of the bodies' own source text: every stored draw of every site is
bit-equal to that replay (the out[(s * 5 + k) * D + d] and draws[(s * m + i / k) * D + d] layouts, the W x S x D workspace and its
fold, the per-site accumulators, pair-row Beta draws and lanes that run samplers of different kinds), the [S, 5, D] table meets
predictive_ref.check, two calls give equal bits, and wherever a site has 16 384 draws or more the KERNEL'S OWN draws pass the
laws, keyed by address.  Then the stride with S = 4, latents outside their support, and the public call: addresses in table
order, each address's draws under that address's own law, held-out rows without a second compilation, and `args=`."""

import time

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import predictive_ref as Q
import temper_fuzz as F
from genjax._amd import temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import PosteriorPredictive, TemperedSMC

pytestmark = pytest.mark.gpu

IMPLS = ("threefry", "philox")
BODIES = {"threefry": 2, "philox": 8}  # per seed: see test_random_bodies


def _dev(cols):
    return [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).cuda() for c in cols]


def _lower(hip_ops, src, args, obs):
    """-> (tracer, plan): lowered on the HIP backend from device tensors; the plan knows no length (data is set per case)."""
    with use_ops(hip_ops):
        tracer = temper.lower(F.target_of(src, args, obs, device="cuda"), 64)
        plan = hip_ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
    if tracer.params:
        plan.set_params(tracer.params)
    return tracer, plan


def _call(hip_ops, plan, key, cols, stride):
    out, draws = hip_ops.temper_predictive(plan, key, _dev(cols), stride)
    torch.cuda.synchronize()
    return out, draws


def _pin(hip_ops, plan, replay, key, cols, y, case, twice=True):
    """One population against the replay's draws y [S, D, n] at stride 1: every draw of every site, every count, the moments,
    and a second call's bits -> the kernel's draws, float32 numpy [S, n, D]."""
    n, D, S = len(cols[0]), replay.D, replay.S
    out, draws = _call(hip_ops, plan, key, cols, 1)
    assert out.shape == (S, 5, D) and out.dtype == torch.float64 and draws.shape == (S, n, D) and draws.dtype == torch.float32, case
    if twice:
        again, draws2 = _call(hip_ops, plan, key, cols, 1)
        assert torch.equal(out.view(torch.int64), again.view(torch.int64)) and torch.equal(draws.view(torch.int32), draws2.view(torch.int32)), case
    got = draws.cpu().numpy()
    for s, a in enumerate(replay.addrs):
        assert Q.same_bits(got[s], y[s].T), (case, a)
    Q.check(out.cpu().numpy(), y, replay.observed(), case)
    return got


def _set(plan, tracer, D):
    data = F.data_of(tracer, D)
    plan.set_data(_dev(data))
    return data


@pytest.fixture(scope="module")
def interleaved(hip_ops):
    args, obs = F.interleaved_inputs()
    tracer, plan = _lower(hip_ops, F.INTERLEAVED, args, obs)
    assert [m["addr"] for m in tracer.meta] == [s[0] for s in F.INTERLEAVED_SITES] and plan.n_plated == 4
    return dict(args=args, obs=obs, tracer=tracer, plan=plan)


@pytest.fixture(scope="module")
def compiled(hip_ops, interleaved):
    """The S = 4 kernel of each generator, compiled by a first launch on two rows; the seconds are printed (under THREEFRY the
    four samplers with a cipher block each take the compiler far longer than any launch below: 12 s on an MI355X machine against
    1 s under PHILOX, paid once per session in the setup of the first test that asks for it)."""
    c, took = interleaved, {}
    _set(c["plan"], c["tracer"], 2)
    cols = F.columns_of(c["tracer"], F.interleaved_latents(2, 5))
    for impl in IMPLS:
        t0 = time.time()
        _call(hip_ops, c["plan"], genjax.random.key(F.PRED_KEY, impl), cols, 0)
        took[impl] = time.time() - t0
    print("first predictive launch of the interleaved body, compilation included:", {k: f"{v:.2f} s" for k, v in took.items()})
    return took


def _case(c, oracle_ops, what, n, D, key):
    """Data of D rows set on the plan -> (replay, its draws y [4, D, n], latents, columns, (args, obs) of those rows)."""
    data = _set(c["plan"], c["tracer"], D)
    latents = F.interleaved_latents(what, n)
    cols = F.columns_of(c["tracer"], latents)
    replay = Q.Replay(oracle_ops, c["tracer"], data, key.impl)
    assert replay.addrs == ["y1", "y2", "y3", "y4"]
    return replay, replay.draws(key, cols), latents, cols, F.head_rows(c["args"], c["obs"], D)


def _laws(src, latents, inputs, addrs, got, context):
    """The KERNEL's draws [S, n, D] against the source text's laws, by address."""
    return F.check_predictive(src, latents, inputs[1], inputs[0], F.draws_by_address(addrs, got), context)


# ---- the interleaved body ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
def test_interleaved_grid(hip_ops, oracle_ops, interleaved, compiled, impl):
    """D in (1, 2, 3, 127, 129, 513) x n in (1, 5, 257) at stride 1: one replay of 257 particles per D — particle i's draws are a
    function of (key, i, x_i), so the smaller populations are its prefixes.  Below 16 384 draws per site the DKW bound is too
    loose to mean anything: bit equality with a replay whose larger case passed the laws is the check there."""
    c, key, worst, lawful = interleaved, genjax.random.key(F.PRED_KEY, impl), {"ks": 0.0, "z": 0.0}, 0
    for D in F.PRED_DS:
        replay, y, latents, cols, inputs = _case(c, oracle_ops, D, max(F.PRED_NS), D, key)
        for n in F.PRED_NS:
            got = _pin(hip_ops, c["plan"], replay, key, [x[:n].copy() for x in cols], y[:, :, :n], ("interleaved", impl, D, n))
            if n * D >= F.LAW_MIN_DRAWS:
                w = _laws(F.INTERLEAVED, {k: v[:n] for k, v in latents.items()}, inputs, replay.addrs, got, f"interleaved {impl} D {D} n {n}")
                worst, lawful = {k: max(worst[k], w[k]) for k in worst}, lawful + 1
    assert lawful == 3  # D = 127, 129, 513 at n = 257
    print(f"interleaved grid, {impl}: worst Kolmogorov distance / bound {worst['ks']:.3f}, |z| / bound {worst['z']:.3f}")


@pytest.mark.parametrize("impl", IMPLS)
def test_interleaved_several_chunks(hip_ops, oracle_ops, interleaved, compiled, impl):
    n, D = F.PRED_BIG
    key = genjax.random.key(F.PRED_KEY + 1, impl)
    assert int(hip_ops.lib.call("gjx_predictive_chunks", n, D)) == 4
    replay, y, latents, cols, inputs = _case(interleaved, oracle_ops, "big", n, D, key)
    got = _pin(hip_ops, interleaved["plan"], replay, key, cols, y, ("interleaved", impl, D, n))
    w = _laws(F.INTERLEAVED, latents, inputs, replay.addrs, got, f"interleaved {impl} big")
    print(f"interleaved {n} x {D}, {impl}: worst Kolmogorov distance / bound {w['ks']:.3f}, |z| / bound {w['z']:.3f}")


def test_interleaved_stride(hip_ops, interleaved, compiled):
    """n = 1000, D = 129, stride 7 with S = 4: the stored draws are every seventh particle's of every site, and the table does
    not depend on the stride."""
    n, D = F.PRED_BIG
    k = 7
    c, key = interleaved, genjax.random.key(F.PRED_KEY + 1, "philox")
    _set(c["plan"], c["tracer"], D)
    cols = F.columns_of(c["tracer"], F.interleaved_latents("big", n))
    full, every = _call(hip_ops, c["plan"], key, cols, 1)
    out, draws = _call(hip_ops, c["plan"], key, cols, k)
    none, nothing = _call(hip_ops, c["plan"], key, cols, 0)
    assert every.shape == (4, n, D) and draws.shape == (4, 143, D) and nothing is None
    for s in range(4):
        assert torch.equal(draws[s].view(torch.int32), every[s, ::k].contiguous().view(torch.int32)), s
    assert torch.equal(out.view(torch.int64), full.view(torch.int64)) and torch.equal(none.view(torch.int64), full.view(torch.int64))


@pytest.mark.parametrize("impl", IMPLS)
def test_interleaved_outside_support(hip_ops, oracle_ops, interleaved, compiled, impl):
    """Every fourth Gamma / Beta latent value outside its support: bit equality with the replay, NaN included, the NaN counts the
    replay's, and the laws on the particles inside."""
    n, D = F.PRED_OUTSIDE
    key = genjax.random.key(F.PRED_KEY + 2, impl)
    replay, y, latents, cols, inputs = _case(interleaved, oracle_ops, "outside", n, D, key)
    ok = F.inside(F.INTERLEAVED_SITES, latents)
    assert (~ok).sum() >= n // 4 and not np.isnan(y[:, :, ok]).any()
    got = _pin(hip_ops, interleaved["plan"], replay, key, cols, y, ("outside", impl))
    out = _call(hip_ops, interleaved["plan"], key, cols, 0)[0].cpu().numpy()
    assert np.array_equal(out[:, 4], np.isnan(y).sum(axis=2)) and np.array_equal(np.isnan(got), np.isnan(np.transpose(y, (0, 2, 1))))
    w = _laws(F.INTERLEAVED, latents, inputs, replay.addrs, got, f"outside {impl}")
    print(f"outside support, {impl}: NaN draws {int(np.isnan(got).sum())}; worst Kolmogorov distance / bound {w['ks']:.3f}, |z| / bound {w['z']:.3f}")


# ---- random bodies -----------------------------------------------------------------------------------------------------------
def _cheap(sites):
    """No plated Gamma or Beta site.  Under THREEFRY each such site is a rejection loop with a cipher block of its own in flight,
    and the compiler takes 10 to 30 s over a body that holds one (measured offline, profiles/predictive_fuzz_summary.md): no such
    body fits a test.  The THREEFRY stream keeps the Normal / flip bodies — the many-site layouts, workspace and accumulators —
    and the multi-word samplers under THREEFRY run in the interleaved body, compiled once per session."""
    return all(kind in ("normal", "flip") for _, role, kind in sites if role == "plated")


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("seed", F.PRED_SEEDS)
def test_random_bodies(hip_ops, oracle_ops, seed, impl):
    """The first BODIES[impl] bodies of the seed's stream that tests/test_predictive_fuzz_cpu.py keeps (a plated site, laws that
    cover 0.9 of the entries; under THREEFRY also `_cheap`) and that lower, at n = 257 and D in (65, 2): bit equality with the
    replay and predictive_ref.check at both, the laws on the kernel's own draws at D = 65.  Each body costs one compilation of
    its predictive kernel per generator.
    Measured on an MI355X machine with four bodies per test (profiles/predictive_fuzz_summary.md): a body's first predictive
    launch, compilation included and the replay not, takes 0.19 to 0.98 s under PHILOX, a whole test of four 1.3 to 2.2 s:
    EIGHT bodies per test (3.3 to 5.2 s when run so).  Under THREEFRY it takes 0.31 to 0.52 s for a body of Normal sites but
    4.2 to 5.2 s for one with a flip site, and whole tests of four took 1.8 to 11.2 s, over the 10 s a test may take: TWO bodies
    per test (0.9 to 5.7 s when run so); the four seeds make eight THREEFRY bodies.  The times of a run are printed."""
    n, sizes = F.PRED_RANDOM
    done, worst, t_first, t0_test = 0, {"ks": 0.0, "z": 0.0}, [], time.time()
    for i, src, sites, args, obs, latents, reasons in F.predictive_stream(seed):
        if reasons or done == BODIES[impl] or (impl == "threefry" and not _cheap(sites)):
            continue
        try:
            tracer, plan = _lower(hip_ops, src, args, obs)
        except PlanUnsupported:
            continue
        key = genjax.random.key(F.PRED_KEY + 100 + i, impl)
        cols = F.columns_of(tracer, latents)
        for D in sizes:
            case = f"seed {seed} body {i} {impl} D {D}\n{src}\nargs {args[3:]}"
            replay = Q.Replay(oracle_ops, tracer, _set(plan, tracer, D), key.impl)
            assert replay.addrs == [name for name, role, _ in sites if role == "plated"]
            y = replay.draws(key, cols)
            if D == sizes[0]:
                t0 = time.time()
                _call(hip_ops, plan, key, cols, 0)  # (the first launch of the body under this generator: its compilation)
                t_first.append((i, replay.S, time.time() - t0))
            got = _pin(hip_ops, plan, replay, key, cols, y, case, twice=D == sizes[0])
            if D == sizes[0]:
                w = _laws(src, latents, F.head_rows(args, obs, D), replay.addrs, got, case)
                worst = {k: max(worst[k], w[k]) for k in worst}
        done += 1
    print(f"seed {seed} {impl}: {done} bodies in {time.time() - t0_test:.2f} s; worst Kolmogorov distance / bound {worst['ks']:.3f}, |z| / bound "
          f"{worst['z']:.3f}; first predictive launch per body (index, plated sites, seconds, compilation included): "
          + ", ".join(f"({i}, {S}, {t:.2f})" for i, S, t in t_first))
    assert done == BODIES[impl]


# ---- the public call ---------------------------------------------------------------------------------------------------------
def _against_replay(pp, replay, key, cols, latents, inputs, k, case):
    """Every address's stored draws: the replay's site OF THAT ADDRESS bit for bit, and that address's own law."""
    y = replay.draws(key, cols)
    assert pp.addresses == ["y1", "y2", "y3", "y4"] == replay.addrs, case
    got = {}
    for s, a in enumerate(replay.addrs):
        got[a] = pp.draws[a].cpu().numpy()
        assert Q.same_bits(got[a], y[s].T[::k]), (case, a)
    ref = Q.summarize(y, replay.observed())
    for s, a in enumerate(replay.addrs):
        assert np.array_equal(pp.below[a].cpu().numpy(), ref[s, 2]) and np.array_equal(pp.nan_count[a].cpu().numpy(), ref[s, 4]), (case, a)
    return F.check_predictive(F.INTERLEAVED, {name: v[::k] for name, v in latents.items()}, inputs[1], inputs[0], got, str(case))


def test_public_api_interleaved(hip_ops, oracle_ops, compiled):
    """alg.predictive(cols, key, draw_stride=4) at n = 300 on 65 fitted rows, then target= of 33 other rows: no new compilation,
    and the same checks against a replay of the held-out lowering."""
    n, D, H = F.PRED_API
    k = 4
    key = genjax.random.key(F.PRED_KEY + 3, "philox")
    fitted = F.head_rows(*F.interleaved_inputs(), D)
    held = F.heldout_inputs()
    latents = F.interleaved_latents("api", n)
    with use_ops(hip_ops):
        target = F.target_of(F.INTERLEAVED, *fitted, device="cuda")
        alg = TemperedSMC(target, n)
        tracer = temper.lower(target, 64)
        cols = F.columns_of(tracer, latents)
        pp = alg.predictive(_dev(cols), key, draw_stride=k)
        before = hip_ops.jit_stats()["compiles"]
        other = F.target_of(F.INTERLEAVED, *held, device="cuda")
        pph = alg.predictive(_dev(cols), key, target=other, draw_stride=k)
        assert hip_ops.jit_stats()["compiles"] == before
        tracer_h = temper.lower(other, 64)
    assert isinstance(pp, PosteriorPredictive) and pp.n == n and pp.draws["y1"].shape == (75, D) and pph.draws["y4"].shape == (75, H)
    _against_replay(pp, Q.Replay(oracle_ops, tracer, F.data_of(tracer), key.impl), key, cols, latents, fitted, k, "fitted rows")
    _against_replay(pph, Q.Replay(oracle_ops, tracer_h, F.data_of(tracer_h), key.impl), key, cols, latents, held, k, "held-out rows")


def test_args_predicts_where_no_plate_feeds_a_site(hip_ops):
    """two_plate and plate_ref.MODELS under args= (nothing observed): the draws and moments of the target= call on the same
    inputs; the interleaved body, whose y4 reads y1's value, is refused (tests/test_predictive_fuzz_cpu.py)."""
    n, k = 300, 4
    key = genjax.random.key(F.PRED_KEY + 4, "philox")
    rng = np.random.default_rng(36)
    xs, zs, y1, y2 = P.two_plate_data(40, seed=2)
    hx, hz, h1, h2 = P.two_plate_data(33, seed=7)
    with use_ops(hip_ops):
        cases = [("two_plate", F.target_of(P.TWO_PLATE, (xs, zs), {"y1": y1, "y2": y2}, device="cuda"),
                  F.target_of(P.TWO_PLATE, (hx, hz), {"y1": h1, "y2": h2}, device="cuda"), 2)]
        cases += [(name, P.target(name, 40, seed=2)[0], P.target(name, 33, seed=7)[0], len(P.columns(name, 1, rng))) for name in P.MODELS]
        for name, train, held, L in cases:
            cols = _dev([(0.3 * rng.standard_normal(n)).astype(np.float32) if name != "hetero" or l == 0 else rng.gamma(2.0, 0.5, n).astype(np.float32)
                         for l in range(L)])
            alg = TemperedSMC(train, n)
            pp = alg.predictive(cols, key, target=held, draw_stride=k)
            new = alg.predictive(cols, key, args=held.args, draw_stride=k)
            assert new.pit is None and new.addresses == pp.addresses and len(pp.addresses) == (2 if name == "two_plate" else 1), name
            for a in pp.addresses:
                assert torch.equal(new.draws[a].view(torch.int32), pp.draws[a].view(torch.int32)), (name, a)
                assert torch.equal(new.mean[a], pp.mean[a]) and torch.equal(new.nan_count[a], pp.nan_count[a]), (name, a)
    with use_ops(hip_ops):
        args, obs = F.head_rows(*F.interleaved_inputs(), 40)
        alg = TemperedSMC(F.target_of(F.INTERLEAVED, args, obs, device="cuda"), n)
        new = tuple(torch.from_numpy(a[:33].copy()).cuda() if isinstance(a, np.ndarray) else a for a in args)
        with pytest.raises(PlanUnsupported, match=r"'y4' reads the value of the plated site at address 'y1'"):
            alg.predictive(_dev([np.full(n, 0.5, dtype=np.float32)] * 4), key, args=new)
