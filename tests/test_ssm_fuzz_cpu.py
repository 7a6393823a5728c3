"""The state-space lowering held to float64 without a GPU (tests/ssm_fuzz.py): random `init` / `step` bodies and the fixed
`MIXED` body are lowered and run on the oracle backend with their history recorded, and every step's log-weights, every carry
component that is not a latent draw and every latent's law given its parents are compared with the float64 replay of the
bodies' own source text; five mutations of the lowered tables must each FAIL that comparison on every body of a fixed set of
ten; the transition tables of backward simulation are held to the same replay; and every derived slot of a parameterised
body's `ParamSpace` equals the float64 value of its own host arithmetic."""

import numpy as np
import pytest
import torch

import backsim_ref as B
import genjax
import ssm_fuzz as S
from genjax._amd import abi, prng
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax._amd.smc_fused import BootstrapSMC
from genjax._amd.smc_plan import build_smc_plan, build_transition_table
from offline import ops  # noqa: F401
from temper_fuzz import FLOOR_FACTOR, misses

SEEDS = (31, 32, 33, 34)
PER_SEED = 50
MAX_DROPPED, MAX_UNLOWERED = 0.10, 0.15  # shares of the generated cases (the tempered fuzz's)
N, T = 3000, 4
IMPL = ("threefry", "philox")


def _run(oracle_ops, src, obs, key, ess=0.0, n=N, plan=None):
    """-> the SMCResult with history of the bootstrap filter of `src` on the oracle.  `plan`: run this plan instead of the
    one the filter lowers (the mutation tests)."""
    with use_ops(oracle_ops):
        smc = BootstrapSMC(S.build_model(*src), S.observations_of(obs), n, ess_threshold=ess, record_history=True)
        if plan is not None:
            smc._bind(oracle_ops)
            smc._plan = (plan, smc._plan[1])
        return smc.run(key), smc


def _ctx(src, **kw):
    return "\n".join([f"{k} {v}" for k, v in kw.items()] + list(src))


def test_random_bodies(oracle_ops):
    """200 random bodies (4 seeds x 50; every other one flat; both generators; n = 3000, T = 4, ess 0 and 0.5): the recorded
    log-weights of every step, the expression components and the latent laws against replay64.  At most 10 % of the cases may
    be dropped for conditioning and at most 15 % may fail to lower; both kinds of row occur among the adaptive runs."""
    compared, unlowered, dropped = 0, [], []
    worst = {}
    rows = {"resampled": 0, "accumulated": 0}
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        for i in range(PER_SEED):
            src = S.random_ssm(rng, flat=i % 2 == 1)
            obs = S.random_observations(rng, src[2]["obs"], T)
            ess, impl = (0.0, 0.5)[(i // 2) % 2], IMPL[(i // 4) % 2]
            try:
                r, _ = _run(oracle_ops, src[:2], obs, genjax.random.key(1000 * seed + i, impl), ess)
            except PlanUnsupported as e:
                unlowered.append(f"seed {seed} case {i}: {e}")
                continue
            ref = S.Reference(r, *src[:2], obs)
            if not ref.kept:
                dropped.append(f"seed {seed} case {i}: {'; '.join(ref.reasons)}")
                continue
            if ess:
                assert r.resampled is not None
                rows["resampled"] += int(r.resampled[1:].sum())
                rows["accumulated"] += int((r.resampled[1:] == 0).sum())
            stats = S.check_run(r, ref=ref, context=_ctx(src[:2], seed=seed, case=i, ess=ess, impl=impl))
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in stats.items()}
            compared += 1
    total = len(SEEDS) * PER_SEED
    print(f"compared {compared}, unlowered {len(unlowered)} ({len(unlowered) / total:.3f}, cap {MAX_UNLOWERED}), dropped {len(dropped)} "
          f"({len(dropped) / total:.3f}, cap {MAX_DROPPED}); worst err / tol: log-weights {worst['lw']:.3f}, expression components "
          f"{worst['expr']:.3f}; largest Kolmogorov distance {worst['ks_abs']:.4f} ({worst['ks']:.3f} of its bound), largest |z| "
          f"{worst['z_abs']:.2f} (bound {S.Z_BOUND}); adaptive rows {rows}")
    for r in unlowered + dropped:
        print("  ", r)
    assert len(unlowered) <= MAX_UNLOWERED * total and len(dropped) <= MAX_DROPPED * total
    assert compared + len(unlowered) + len(dropped) == total
    assert rows["resampled"] > 0 and rows["accumulated"] > 0, rows


def test_parameterised_bodies_lower(ops):  # noqa: F811
    """The same caps for bodies that take theta (their launches need the GPU; the lowering does not): of 100, at most 15 % may
    fail to lower."""
    rng = np.random.default_rng(41)
    unlowered = []
    for i in range(100):
        src = S.random_ssm(rng, flat=i % 2 == 1, params=True)
        try:
            with use_ops(ops):
                build_smc_plan(S.build_model(*src[:2], params=True), [(n_,) for n_, _ in src[2]["obs"]], S.random_theta(rng))
        except PlanUnsupported as e:
            unlowered.append(f"case {i}: {e}")
    print(f"parameterised bodies: unlowered {len(unlowered)} of 100 (cap {MAX_UNLOWERED})", *unlowered, sep="\n  ")
    assert len(unlowered) <= MAX_UNLOWERED * 100


# ---- the fixed body ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ess,impl", [(0.0, "threefry"), (0.5, "philox")])
def test_mixed(oracle_ops, ess, impl):
    """Nested callees two deep (a latent returned through both into the carry, an observed site at ("h", "o")), an integer-valued
    flip column, an observation and a constant as carry components."""
    rng = np.random.default_rng(7)
    obs = {("h", "o"): rng.standard_normal(T).astype(np.float32), ("z",): rng.standard_normal(T).astype(np.float32)}
    r, smc = _run(oracle_ops, S.MIXED, obs, genjax.random.key(5, impl), ess)
    assert [a for a, _ in S.observations_of(obs).leaves()] == list(S.MIXED_OBS)
    # (a generated plan keeps every carry column in f32: the integer-valued flip is the column of its values 0.0 / 1.0)
    assert smc._plan[0]._nested and all(h.dtype == torch.float32 for h in r.history)
    assert set(np.unique(r.history[1].numpy())) == {0.0, 1.0} and np.all(r.history[3].numpy() == 1.5)
    ref = S.Reference(r, *S.MIXED, obs)
    assert ref.kept, ref.reasons
    assert ref.r64.latent_components[1] == {("k",): 1, ("h", "in", "w"): 0} and sorted(ref.r64.comps) == [2, 3]
    stats = S.check_run(r, ref=ref)
    print(f"mixed, ess {ess}, {impl}: {stats}")


# ---- mutations of the lowered tables -----------------------------------------------------------------------------------------
def _prog(a):
    return [(o.op, o.ref, o.value) for o in (abi.ExprOp * a.ref).from_address(a.table)]


def _copy(a):
    return abi.Arg.from_buffer_copy(a)


class _Tables:
    """A mutable copy of a lowered plan's tables (the product's are not touched)."""

    def __init__(self, plan):
        self.init = [abi.Site.from_buffer_copy(s) for s in plan._tables[0]]
        self.step = [abi.Site.from_buffer_copy(s) for s in plan._tables[1]]
        self.init_state, self.next_state = [_copy(a) for a in plan._state_args[0]], [_copy(a) for a in plan._state_args[1]]
        self.n_state, self.n_obs, self.keep, self._plan = plan.n_state, plan.n_obs, [], plan

    def create(self, oracle_ops):
        p = oracle_ops.smc_plan_create(self.init, self.step, self.init_state, self.next_state, self.n_obs)
        p._keep = (self.keep, self._plan)
        return p

    def step_args(self, observed=None):
        """(holder, key) of every argument of the step: the sites' (`observed`: of the observed / the latent ones only), then
        the carry's."""
        out = []
        for s in self.step:
            if observed is None or bool(s.observed) == observed:
                out += [(s.arg, k) for k in range(1 if s.dist == abi.DIST_BERNOULLI else 2)]
        return out

    def carry_args(self):
        return [(self.next_state, k) for k in range(self.n_state)]


def _move_state(t, where):
    """The first state reference among `where` to the next component -> whether there was one."""
    for holder, k in where:
        a = holder[k]
        if a.kind == abi.ARG_STATE:
            holder[k] = abi.Arg(a.kind, (a.ref + 1) % t.n_state, a.scale, a.offset, None)
            return True
        if a.kind == abi.ARG_EXPR and any(op == abi.EXPR_STATE for op, _, _ in _prog(a)):
            prog, done = [], False
            for op, ref, v in _prog(a):
                if op == abi.EXPR_STATE and not done:
                    ref, done = (ref + 1) % t.n_state, True
                prog.append((op, ref, v))
            holder[k] = abi.expr_arg(prog, t.keep)
            return True
    return False


def _mutate(plan, which):
    """-> the mutated _Tables, or None when the body does not hold the feature."""
    t = _Tables(plan)
    if which == "state_reference":      # a state reference of an observed site or of a carry program moves to the next component
        ok = t.n_state > 1 and _move_state(t, t.step_args(observed=True) + t.carry_args())
    elif which == "obs_columns":        # observation columns 0 and 1 change places wherever they are read
        sw = {0: 1, 1: 0}
        ok = t.n_obs > 1
        for sites, state in ((t.init, t.init_state), (t.step, t.next_state)):
            holders = [(s.arg, k) for s in sites for k in range(2)] + [(state, k) for k in range(t.n_state)]
            for s in sites:
                if s.observed and s.obs.kind == abi.ARG_OBS:
                    s.obs = abi.Arg(abi.ARG_OBS, sw.get(s.obs.ref, s.obs.ref), s.obs.scale, s.obs.offset, None)
            for holder, k in holders:
                a = holder[k]
                if a.kind == abi.ARG_OBS:
                    holder[k] = abi.Arg(a.kind, sw.get(a.ref, a.ref), a.scale, a.offset, None)
                elif a.kind == abi.ARG_EXPR:
                    holder[k] = abi.expr_arg([(op, sw.get(ref, ref) if op == abi.EXPR_OBS else ref, v) for op, ref, v in _prog(a)], t.keep)
    elif which == "reverse_sub":        # x - y becomes y - x in a carry program: the exact negation of the difference
        ok = False
        for holder, k in t.carry_args():
            a = holder[k]
            if not ok and a.kind == abi.ARG_EXPR and abi.EXPR_SUB in [op for op, _, _ in _prog(a)]:
                p = _prog(a)
                j = [op for op, _, _ in p].index(abi.EXPR_SUB)
                holder[k] = abi.expr_arg(p[:j + 1] + [(abi.EXPR_NEG, 0, 0.0)] + p[j + 1:], t.keep)
                ok = True
    elif which == "second_argument":    # a latent's second argument, a plain reference, reads another site (or another
        # component of the carry).  (Inside a program the same slip can be invisible: with `clamp((0.9 + c3) * (0.9 + c3) + 1.2,
        # max=2.0)` for a scale, reading c0 for the first c3 leaves the clamp saturated on nearly every particle.)
        ok = False
        for q, s in enumerate(t.step):
            a = s.arg[1]
            if ok or s.observed or s.dist == abi.DIST_BERNOULLI:
                continue
            if a.kind == abi.ARG_SITE and q > 1:
                others = [j for j in range(q) if j != a.ref]
                s.arg[1] = abi.Arg(a.kind, others[0], a.scale, a.offset, None)
                ok = True
            elif a.kind == abi.ARG_STATE and t.n_state > 1:
                ok = _move_state(t, [(s.arg, 1)])
    elif which == "affine_sign":        # the sign of an affine `scale` of an observed site's argument
        ok = False
        for holder, k in t.step_args(observed=True):
            a = holder[k]
            if not ok and a.kind in (abi.ARG_STATE, abi.ARG_SITE, abi.ARG_OBS) and a.scale != 0.0:
                holder[k] = abi.Arg(a.kind, a.ref, -a.scale, a.offset, None)
                ok = True
    else:
        raise ValueError(which)
    return t if ok else None


MUTATIONS = ("state_reference", "obs_columns", "reverse_sub", "second_argument", "affine_sign")
MUTATION_SEED, MUTATION_BODIES = 500, 10


@pytest.fixture(scope="module")
def mutation_cases(oracle_ops):
    """The bodies of one fixed stream (seed 500; lowered, well conditioned) with their lowered plans, shared by the
    mutations: each takes the first ten that hold its feature."""
    rng = np.random.default_rng(MUTATION_SEED)
    cases = []
    for i in range(200):
        src = S.random_ssm(rng, flat=i % 3 == 2)
        obs = S.random_observations(rng, src[2]["obs"], T)
        key = genjax.random.key(i, IMPL[i % 2])
        try:
            r, smc = _run(oracle_ops, src[:2], obs, key)
        except PlanUnsupported:
            continue
        ref = S.Reference(r, *src[:2], obs)
        if ref.kept:
            S.check_run(r, ref=ref)  # (the unmutated plan passes)
            cases.append((src, obs, key, smc._plan[0]))
    return cases


@pytest.mark.parametrize("which", MUTATIONS)
def test_mutations_fail_the_float64_check(oracle_ops, mutation_cases, which):
    """The mistakes the check exists for, made in a copy of the lowered tables and run on the oracle: `check_run` fails on
    every one of the first ten bodies that hold the mutated feature."""
    done, caught_by = 0, {}
    for src, obs, key, plan in mutation_cases:
        t = _mutate(plan, which)
        if t is None:
            continue
        r, _ = _run(oracle_ops, src[:2], obs, key, plan=t.create(oracle_ops))
        with pytest.raises(AssertionError, match="miss the float64 reference|law of") as e:
            S.check_run(r, *src[:2], obs, context=_ctx(src[:2], mutation=which))
        what = str(e.value).split(":")[0].split(" ")[0]
        caught_by[what] = caught_by.get(what, 0) + 1
        done += 1
        if done == MUTATION_BODIES:
            break
    print(f"{which}: caught on {done} of {done} bodies, by {caught_by}")
    assert done == MUTATION_BODIES


# ---- transition tables ---------------------------------------------------------------------------------------------------------
def _state_column(rng, kind, m):
    return {"normal": lambda: rng.standard_normal(m), "gamma": lambda: rng.gamma(2.0, 0.5, m) + 0.05,
            "beta": lambda: rng.uniform(0.05, 0.95, m)}[kind]().astype(np.float32)


def test_transition_tables(oracle_ops):
    """Every flat random body that lowers (100 generated): the log-weight column of backsim_ref.transition_importance_plan over
    a random old-state column of 257 rows, for 8 random (next state, observation) rows, against the float64 log-densities of
    the step's latent sites plus its observed sites that READ THE OLD STATE in the source text (one that depends on the new
    state alone is dropped by the builder by design).  Bodies with a component that is not a latent draw are refused."""
    rng = np.random.default_rng(61)
    n, compared, unlowered, dropped, refused, worst = 257, 0, 0, 0, 0, 0.0
    kb = prng.split_lazy(prng.key(0, "philox"), n)
    for i in range(100):
        src = S.random_ssm(rng, flat=i % 4 != 3)
        d = src[2]
        addrs = [(n_,) for n_, _ in d["obs"]]
        with use_ops(oracle_ops):
            model = S.build_model(*src[:2])
            if any(w != "latent" for w, _ in d["comps"]):
                with pytest.raises(PlanUnsupported, match="carry component"):
                    build_transition_table(model, addrs)
                refused += 1
                continue
            try:
                table = build_transition_table(model, addrs)
            except PlanUnsupported:
                unlowered += 1
                continue
            plan = B.transition_importance_plan(oracle_ops, table)
        kinds = [dict(d["lat"])[name] for _, name in d["comps"]]
        old = [_state_column(rng, k, n) for k in kinds]
        ns = S.namespace(*src[:2])
        for _ in range(8):
            nxt = [_state_column(rng, k, 1)[0] for k in kinds]
            row = {(n_,): v[0] for n_, v in S.random_observations(rng, d["obs"], 1).items()}
            plan.set_params(np.asarray(nxt + list(row.values()), dtype=np.float32))
            with use_ops(oracle_ops):
                got = oracle_ops.importance_run(plan, kb, n, [torch.from_numpy(c) for c in old], [], want_score=False, want_max_partials=False)[2].numpy()
            values = {(name,): float(nxt[c]) for c, (_, name) in enumerate(d["comps"])}
            sums = {}
            for dtype in (torch.float64, torch.float32):
                carry = tuple(torch.from_numpy(c.astype(np.float64)).to(dtype) for c in old)
                run = S.Run(ns, "step", (carry[0] if len(carry) == 1 else carry,), values, row, dtype)
                kept = [s for s in run.sites if s["latent"] or d["reads_old"][s["addr"][0]]]
                sums[dtype] = sum(s["lp"] + torch.zeros(n, dtype=dtype) for s in kept).numpy().astype(np.float64)
                if dtype == torch.float64:
                    spec = sum(np.broadcast_to(s["tol"], (n,)) for s in kept)
            r64, r32 = sums[torch.float64], sums[torch.float32]
            fin = np.isfinite(r64) & np.isfinite(r32)
            tol = spec + FLOOR_FACTOR * (float(np.abs(r32 - r64)[fin].max()) if fin.any() else 0.0)
            if fin.mean() < S.MIN_FINITE or tol[fin].max() > S.COND_REL * max(1.0, float(np.median(np.abs(r64[fin])))):
                dropped += 1
                continue
            bad = misses(got, r64, tol)
            assert not bad.any(), (f"{int(bad.sum())} of {n} transition sums miss the float64 reference: got {got[bad][:3]}, "
                                   f"reference {r64[bad][:3]}, tol {tol[bad][:3]}\n" + _ctx(src[:2], case=i, next=nxt, obs=row))
            worst = max(worst, float((np.abs(got - r64)[fin] / tol[fin]).max()))
            compared += 1
    flat = 100 - refused
    print(f"transition tables: {compared} (body, row) pairs compared, {dropped} dropped for conditioning, {unlowered} of {flat} flat bodies "
          f"unlowered, {refused} bodies refused as they must be; worst err / tol {worst:.3f}")
    assert unlowered <= MAX_UNLOWERED * flat and dropped <= MAX_DROPPED * 8 * flat and compared > 0


def test_transition_tables_refuse_what_has_no_density(oracle_ops):
    """A nested call (MIXED) and a latent returned twice."""
    twice = ("def init():\n    x0 = normal(0.0, 1.0) @ 'x0'\n    normal(x0, 0.5) @ 'y0'\n    return (x0, x0)\n",
             "def step(carry):\n    c0, c1 = carry\n    x0 = normal(0.9 * c0, 1.0) @ 'x0'\n    normal(x0, 0.5) @ 'y0'\n    return (x0, x0)\n")
    with use_ops(oracle_ops):
        with pytest.raises(PlanUnsupported, match="nested `@gen` call"):
            build_transition_table(S.build_model(*S.MIXED), list(S.MIXED_OBS))
        with pytest.raises(PlanUnsupported, match="returned twice"):
            build_transition_table(S.build_model(*twice), [("y0",)])


# ---- the slots of a parameterised body -------------------------------------------------------------------------------------
def test_param_space_rows(ops):  # noqa: F811
    """Parameterised random bodies (40 generated), `plan._space.rows(thetas)` over 16 random thetas: slots 0 .. P-1 are theta
    rounded to f32, and every derived slot's column over the 16 rows is, bit for bit, the f32 rounding of the float64 value of
    a piece of host arithmetic the SOURCE TEXT hands to a site argument or a traced value at those thetas (ssm_fuzz.theta_uses)
    — and every such piece has a slot.  Which slot an argument reads is covered where the launches run, on the GPU."""
    rng = np.random.default_rng(71)
    checked = derived = 0
    for i in range(40):
        src = S.random_ssm(rng, flat=i % 2 == 1, params=True)
        addrs = [(n_,) for n_, _ in src[2]["obs"]]
        thetas = np.stack([S.random_theta(rng) for _ in range(16)])
        try:
            with use_ops(ops):
                plan, _ = build_smc_plan(S.build_model(*src[:2], params=True), addrs, thetas[0])
        except PlanUnsupported:
            continue
        rows = plan._space.rows(thetas)
        P = len(S.THETA)
        assert rows.dtype == np.float32 and rows.shape == (16, plan._space.n_slots) and np.array_equal(rows[:, :P], thetas)
        uses = np.asarray([S.theta_uses(*src[:2], addrs, th) for th in thetas], dtype=np.float64).reshape(16, -1).astype(np.float32)
        want = {uses[:, k].tobytes() for k in range(uses.shape[1])}
        have = {rows[:, k].tobytes() for k in range(rows.shape[1])}
        ctx = _ctx(src[:2], case=i)
        for k in range(P, rows.shape[1]):
            assert rows[:, k].tobytes() in want, f"slot {k} holds {rows[:3, k]}: no host arithmetic of the source gives that\n{ctx}"
        assert want <= have, f"{len(want - have)} derived values of the source text have no slot\n{ctx}"
        checked, derived = checked + 1, derived + rows.shape[1] - P
    print(f"ParamSpace: {checked} bodies, {derived} derived slots")
    assert checked >= 30 and derived >= 30
