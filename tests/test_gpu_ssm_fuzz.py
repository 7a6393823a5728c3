"""The state-space kernels held to float64 on the GPU (tests/ssm_fuzz.py): random `init` / `step` bodies and the fixed `MIXED`
body through the fused bootstrap step, the parameter bank, the guided step, the conditional step and backward simulation.
Every recorded run is replayed in float64 from the bodies' own source text, which shares nothing with the lowering: the
log-weights of every step, every carry component that is not a latent draw, and the law of every latent draw given its parents.

Shapes, with tile = ops.tile: n in {1, tile + 1, 2 tile + 476} — a lone particle, one past a tile, a ragged third tile — and
T = 4.  Log-weights and expression components are checked at all three, laws at the largest only, pooled over the steps and
over 3 keys (N >= 5000 per site).  The shares of bodies that do not lower or are dropped for conditioning are asserted on 200
bodies by tests/test_ssm_fuzz_cpu.py; here a test takes the first body of its stream that lowers and is conditioned."""

import time

import numpy as np
import pytest
import torch

import backmove_ref as M
import backsim_ref as B
import genjax
import ssm_fuzz as S
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax._amd.smc_plan import build_transition_table
from genjax.inference.smc import BootstrapSMC, GuidedSMC

pytestmark = pytest.mark.gpu

T = 4
SEEDS = (51, 52, 53, 54)
BODIES = 8          # per seed: one test each (a body costs one compilation of its step kernels, see _generator)
KEYS = 3            # runs pooled for a law check
IMPL = ("threefry", "philox")
ATTEMPTS = 4        # bodies a test may walk past (unlowered, or dropped for conditioning) before it fails


def _generator(body):
    """Every fourth body runs under threefry, the others under philox.  Measured on an MI355X machine: the one compilation of a
    body's kernels — every launch after it takes milliseconds — costs 1.2 to 4 s under philox, and under threefry 2 s plus
    about 3 s per latent Gamma site and 6 s per latent Beta site (29 s for two Beta and one Gamma).  That compilation is the
    test's time, so the threefry bodies are drawn `cheap` (ssm_fuzz.random_ssm: Normal latents, at most one Gamma); the lowering
    does not depend on the generator, and the threefry Gamma and Beta samplers are held by the distribution and parity suites."""
    return IMPL[0] if body % 4 == 3 else IMPL[1]


def _bodies(seed, body, make):
    """The first body of the stream (seed, body) on which `make(rng, attempt)` returns True; it returns a reason (a string)
    for a body it walks past and lets PlanUnsupported through."""
    rng, refused = np.random.default_rng([seed, body]), []
    for attempt in range(ATTEMPTS):
        try:
            out = make(rng, attempt)
        except PlanUnsupported as e:
            out = f"unlowered: {e}"
        if out is True:
            return refused
        refused.append(out)
    raise AssertionError(f"no body of {ATTEMPTS} could be compared: {refused}")


def _sizes(ops):
    return 1, ops.tile + 1, 2 * ops.tile + 476


def _smc(src, d, obs, n, ess=0.0, history=True, like=None, theta=None, proposals=None):
    """The filter of a body; `like`: a filter of the same body that has run — its compiled plan is shared."""
    model, chm = S.build_model(*src, params=d["params"]), S.observations_of(obs)
    if proposals is not None:
        sp, ip = S.build_proposals(proposals)
        smc = GuidedSMC(model, chm, n, sp, ip, ess_threshold=ess, record_history=history, params=theta)
    else:
        smc = BootstrapSMC(model, chm, n, ess_threshold=ess, record_history=history, params=theta)
    if like is not None:
        assert like._plan is not None
        smc._plan = like._plan
    return smc


def _ctx(src, proposals=None, **kw):
    p = proposals or {}
    return "\n".join([f"{k} {v}" for k, v in kw.items()] + list(src) + [p.get("step") or "", p.get("init") or ""])


class _Stats:
    def __init__(self):
        self.worst, self.first, self.small = {}, [], 0

    def add(self, s):
        self.worst.update({k: max(v, self.worst.get(k, 0.0)) for k, v in s.items()})

    def __str__(self):
        w = self.worst
        return (f"worst err / tol: log-weights {w.get('lw', 0):.3f}, expression components {w.get('expr', 0):.3f}; largest Kolmogorov "
                f"distance {w.get('ks_abs', 0):.4f} ({w.get('ks', 0):.3f} of its bound), largest |z| {w.get('z_abs', 0):.2f} (bound {S.Z_BOUND}); "
                f"first run of a body (compilation included) {min(self.first, default=0):.2f} .. {max(self.first, default=0):.2f} s")


def _bootstrap_body(hip_ops, src, d, obs, impl, seed, stats, theta=None):
    """The bootstrap checks of one body -> False when a reference at n > 1 is not conditioned (nothing is counted then)."""
    ns = _sizes(hip_ops)
    ctx = _ctx(src, seed=seed, impl=impl)
    keys = [genjax.random.key(100 * seed + k, impl) for k in range(KEYS)]
    t0 = time.time()
    big = _smc(src, d, obs, ns[2], theta=theta)
    runs = [big.run(k) for k in keys]
    torch.cuda.synchronize()
    stats.first.append(time.time() - t0)
    refs = [S.Reference(r, *src, obs, theta=theta) for r in runs]
    todo = [(r, ref, True) for r, ref in zip(runs, refs)]
    for n in ns:
        for ess in (0.0, 0.5):
            if n == ns[2] and ess == 0.0:
                continue
            r = _smc(src, d, obs, n, ess, like=big, theta=theta).run(keys[0])
            if ess and n > 1:
                assert r.resampled is not None and r.resampled.numel() == T
            if n == ns[1]:  # the whole-run call returns the estimate of the stepwise run, as run_with_history promises
                plain = _smc(src, d, obs, n, ess, history=False, like=big, theta=theta).run(keys[0])
                assert plain.history is None and plain.log_marginal_likelihood == r.log_marginal_likelihood, ctx
                assert torch.equal(plain.log_weights, r.log_weights), ctx
            todo.append((r, S.Reference(r, *src, obs, theta=theta), False))
    if not all(ref.kept for r, ref, _ in todo if r.log_weights.numel() > 1):
        return False
    samples = []
    for r, ref, law in todo:
        if not ref.kept:  # (a lone particle: a single entry decides the conditioning)
            stats.small += 1
            continue
        stats.add(S.check_run(r, ref=ref, laws=False, context=ctx))
        if law:
            samples.append(S.law_samples(ref))
    stats.add(S.check_laws(samples, ctx))
    return True


@pytest.mark.parametrize("body", range(BODIES))
@pytest.mark.parametrize("seed", SEEDS)
def test_random_bodies(hip_ops, seed, body):
    """8 bodies x 4 seeds (one per test; every other body flat; both generators): the bootstrap filter with history at ess 0
    and 0.5 at the three sizes, and once without history — `log_marginal_likelihood` and the final log-weights equal the
    history run's."""
    stats, impl = _Stats(), _generator(body)

    def make(rng, attempt):
        src = S.random_ssm(rng, flat=body % 2 == 1, cheap=impl == IMPL[0])
        obs = S.random_observations(rng, src[2]["obs"], T)
        return _bootstrap_body(hip_ops, src[:2], src[2], obs, impl, 16 * seed + body, stats) or "dropped for conditioning"

    with use_ops(hip_ops):
        refused = _bodies(seed, body, make)
    print(f"seed {seed} body {body} {impl}: {stats}; lone-particle runs not conditioned {stats.small}", *refused, sep="\n  ")


def test_mixed(hip_ops):
    """Nested callees two deep with an observed site at a nested address, an integer-valued flip column, an observation and
    a constant as carry components: the bootstrap checks, under both generators."""
    rng = np.random.default_rng(7)
    obs = {("h", "o"): rng.standard_normal(T).astype(np.float32), ("z",): rng.standard_normal(T).astype(np.float32)}
    d = dict(params=False)
    stats = _Stats()
    with use_ops(hip_ops):
        for impl in IMPL:
            assert _bootstrap_body(hip_ops, S.MIXED, d, obs, impl, 7, stats)
        r = _smc(S.MIXED, d, obs, 257).run(genjax.random.key(1, "philox"))
    assert all(h.dtype == torch.float32 for h in r.history) and set(np.unique(r.history[1].cpu().numpy())) <= {0.0, 1.0}
    print(f"mixed: {stats}")


# ---- parameterised bodies ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", range(3))
@pytest.mark.parametrize("seed", (61, 62))
def test_parameterised_bodies(hip_ops, seed, body):
    """A body that takes theta: `run(key, params=row)` for 3 rows through ONE compiled plan — nothing is compiled after the
    first row — each row checked against replay64 at its f32 theta (laws pooled over the rows); then a bank,
    `run_many(keys, params=rows)` with F = 16 at n = tile + 1: filter f's final log-weights and estimate are bit-equal to the
    single run of row f, and rows 0 .. 2 of those to a history run that replay64 checks."""
    ns, stats, impl = _sizes(hip_ops), _Stats(), _generator(body + 1)

    def make(rng, attempt):
        src = S.random_ssm(rng, flat=body % 2 == 1, params=True, cheap=impl == IMPL[0])
        obs = S.random_observations(rng, src[2]["obs"], T)
        rows = np.stack([S.random_theta(rng) for _ in range(16)])
        ctx = _ctx(src[:2], seed=seed, impl=impl)
        keys = [genjax.random.key(1000 * seed + 100 * body + f, impl) for f in range(16)]
        t0 = time.time()
        big = _smc(src[:2], src[2], obs, ns[2])
        runs = [big.run(keys[0], params=rows[0])]
        torch.cuda.synchronize()
        stats.first.append(time.time() - t0)
        compiles = hip_ops.jit_stats()["compiles"]
        runs += [big.run(keys[f], params=rows[f]) for f in (1, 2)]
        assert hip_ops.jit_stats()["compiles"] == compiles, "a new row must not compile anything\n" + ctx
        refs = [S.Reference(r, *src[:2], obs, theta=rows[f]) for f, r in enumerate(runs)]
        hist = _smc(src[:2], src[2], obs, ns[1], like=big)
        small = [hist.run(keys[f], params=rows[f]) for f in range(3)]
        srefs = [S.Reference(r, *src[:2], obs, theta=rows[f]) for f, r in enumerate(small)]
        bank = _smc(src[:2], src[2], obs, ns[1], history=False, like=big)
        many = bank.run_many(keys, params=rows)
        ones = [bank.run(keys[f], params=rows[f]) for f in range(16)]
        if not all(r.kept for r in refs + srefs):
            return "dropped for conditioning"
        for r, ref in zip(runs + small, refs + srefs):
            stats.add(S.check_run(r, ref=ref, laws=False, context=ctx))
        stats.add(S.check_laws([S.law_samples(ref) for ref in refs], ctx))
        for f in range(16):
            assert torch.equal(many[f].log_weights, ones[f].log_weights), (f, ctx)
            assert many[f].log_marginal_likelihood == ones[f].log_marginal_likelihood, (f, ctx)
            if f < 3:
                assert torch.equal(ones[f].log_weights, small[f].log_weights), (f, ctx)
                assert ones[f].log_marginal_likelihood == small[f].log_marginal_likelihood, (f, ctx)
        return True

    with use_ops(hip_ops):
        refused = _bodies(seed, body, make)
    print(f"seed {seed} body {body} {impl}: parameterised: {stats}", *refused, sep="\n  ")


# ---- guided bodies ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", range(4))
@pytest.mark.parametrize("seed", (71, 72))
def test_guided_bodies(hip_ops, seed, body):
    """A flat body under GuidedSMC with random proposals (body 3 of a seed: parameterised): the log-weights are
    log p(proposed latents) + log p(observations) - log q(proposed latents); a proposed latent follows the PROPOSAL's law given
    the carry and y, an unproposed one the model's."""
    ns, stats, impl, params = _sizes(hip_ops), _Stats(), _generator(body + 2), body == 3
    count = {}

    def make(rng, attempt):
        src = S.random_ssm(rng, flat=True, params=params, cheap=impl == IMPL[0])
        prop = S.random_proposal(rng, src[2])
        obs = S.random_observations(rng, src[2]["obs"], T)
        theta = S.random_theta(rng) if params else None
        ctx = _ctx(src[:2], prop, seed=seed, impl=impl, theta=theta)
        keys = [genjax.random.key(1000 * seed + 100 * body + k, impl) for k in range(KEYS)]
        t0 = time.time()
        big = _smc(src[:2], src[2], obs, ns[2], theta=theta, proposals=prop)
        runs = [big.run(k) for k in keys]
        torch.cuda.synchronize()
        stats.first.append(time.time() - t0)
        runs.append(_smc(src[:2], src[2], obs, ns[1], 0.5, like=big, theta=theta, proposals=prop).run(keys[0]))
        runs.append(_smc(src[:2], src[2], obs, 1, like=big, theta=theta, proposals=prop).run(keys[0]))
        refs = [S.Reference(r, *src[:2], obs, theta=theta, proposals=prop) for r in runs]
        if not all(r.kept for r in refs[:-1]):
            return "dropped for conditioning"
        for r, ref in zip(runs, refs):
            if ref.kept:
                stats.add(S.check_run(r, ref=ref, laws=False, context=ctx))
        stats.add(S.check_laws([S.law_samples(ref) for ref in refs[:KEYS]], ctx))
        flags = refs[0].r64.proposed
        assert {a[0] for a, f in flags.items() if f[1]} == set(prop["step_sites"]), ctx
        assert {a[0] for a, f in flags.items() if f[0]} == set(prop["init_sites"]), ctx
        count["proposed"], count["free"] = sum(f[1] for f in flags.values()), sum(not f[1] for f in flags.values())
        return True

    with use_ops(hip_ops):
        refused = _bodies(seed, body, make)
    print(f"seed {seed} body {body} {impl}: guided: {stats}; latents proposed {count['proposed']}, left to the model {count['free']}", *refused, sep="\n  ")
    assert count["proposed"] > 0


# ---- the conditional step --------------------------------------------------------------------------------------------------------
def _genealogy(r, leaf):
    """The path of final particle `leaf` through a recorded run, one contiguous f32 [T] tensor per carry component."""
    hist = r.history if isinstance(r.history, tuple) else (r.history,)
    anc = r.ancestors.cpu().numpy()
    idx, rows = leaf, []
    for t in range(anc.shape[0] - 1, -1, -1):
        rows.append(idx)
        idx = int(anc[t][idx])
    rows = torch.as_tensor(rows[::-1], device=hist[0].device)
    return tuple(h.gather(1, rows[:, None])[:, 0].contiguous() for h in hist)


@pytest.mark.parametrize("body", range(3))
@pytest.mark.parametrize("seed", (81, 82))
def test_conditional_step(hip_ops, seed, body):
    """A flat body, `run(key, retained=path)` with a path of an earlier run of the same filter: slot n - 1 of every step holds
    the path bit for bit and is its own ancestor; every log-weight, the retained slot's included, matches replay64; the laws
    hold over slots 0 .. n - 2."""
    ns, stats, impl = _sizes(hip_ops), _Stats(), _generator(body + 3)

    def make(rng, attempt):
        src = S.random_ssm(rng, flat=True, cheap=impl == IMPL[0])
        obs = S.random_observations(rng, src[2]["obs"], T)
        ctx = _ctx(src[:2], seed=seed, impl=impl)
        keys = [genjax.random.key(1000 * seed + 100 * body + k, impl) for k in range(KEYS + 1)]
        t0 = time.time()
        big = _smc(src[:2], src[2], obs, ns[2])
        first = big.run(keys[KEYS])
        torch.cuda.synchronize()
        stats.first.append(time.time() - t0)
        path = _genealogy(first, 5)
        runs = [(big.run(k, retained=path), path) for k in keys[:KEYS]]
        small = _smc(src[:2], src[2], obs, ns[1], like=big)
        spath = _genealogy(small.run(keys[KEYS]), ns[1] - 1)
        runs.append((small.run(keys[0], retained=spath), spath))
        refs = [S.Reference(r, *src[:2], obs) for r, _ in runs]
        if not all(r.kept for r in refs):
            return "dropped for conditioning"
        for (r, p), ref in zip(runs, refs):
            n = r.log_weights.numel()
            hist = r.history if isinstance(r.history, tuple) else (r.history,)
            for h, c in zip(hist, p):
                assert torch.equal(h[:, n - 1].view(torch.int32), c.view(torch.int32)), ctx
            assert bool((r.ancestors[:, n - 1] == n - 1).all()), ctx
            stats.add(S.check_run(r, ref=ref, laws=False, context=ctx))
        stats.add(S.check_laws([S.law_samples(ref, free=slice(0, ns[2] - 1)) for ref in refs[:KEYS]], ctx))
        return True

    with use_ops(hip_ops):
        refused = _bodies(seed, body, make)
    print(f"seed {seed} body {body} {impl}: conditional step: {stats}", *refused, sep="\n  ")


# ---- backward simulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", range(2))
def test_backward_simulation(hip_ops, oracle_ops, body):
    """2 flat random bodies (one per test), n = 257, T = 3, m = 64: the lineage and the paths of `backward_simulate` equal
    backsim_ref.backsim_ref's, and those of the MCMC route (`n_moves=3`) backmove_ref.backmove_ref's — both references take the
    transition table lowered on the oracle, which tests/test_ssm_fuzz_cpu.py holds to float64."""
    n, Tb, m, K = 257, 3, 64, 3

    def make(rng, attempt):
        src = S.random_ssm(rng, flat=True)
        obs = S.random_observations(rng, src[2]["obs"], Tb)
        addrs = [(n_,) for n_, _ in src[2]["obs"]]
        with use_ops(oracle_ops):
            table = build_transition_table(S.build_model(*src[:2]), addrs)
        rows = np.stack([obs[n_] for n_, _ in src[2]["obs"]], axis=1)
        ctx = _ctx(src[:2], body=body)
        key, key2 = genjax.random.key(3 + body, "philox"), genjax.random.key(13 + body, "philox")
        with use_ops(hip_ops):
            alg = _smc(src[:2], src[2], obs, n)
            res = alg.run(key)
            sm = alg.backward_simulate(res, key2, n_paths=m)
            mv = alg.backward_simulate(res, key2, n_paths=m, n_moves=K)
        torch.cuda.synchronize()
        hist = [c.cpu() for c in (res.history if isinstance(res.history, tuple) else (res.history,))]
        lw, anc = res.log_weight_history.cpu(), res.ancestors.cpu()
        lin, paths = B.backsim_ref(oracle_ops, table, key2, hist, lw, rows, m)
        stats = {}
        mlin, mpaths = M.backmove_ref(oracle_ops, table, key2, hist, lw, anc, rows, m, K, stats)
        for got, (rl, rp), what in ((sm, (lin, paths), "backward simulation"), (mv, (mlin, mpaths), "backward moves")):
            gp = got.paths if isinstance(got.paths, tuple) else (got.paths,)
            assert torch.equal(got.lineage.cpu(), rl), f"{what}: {int((got.lineage.cpu() != rl).sum())} lineage entries differ\n{ctx}"
            for a, b in zip(gp, rp):
                assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)), f"{what}\n{ctx}"
        print(f"body {body}: {len(table.sites)} sites in the transition table; the move reference accepted {stats['accepted']} of {m * K * (Tb - 1)}")
        return True

    _bodies(91, body, make)
