"""The predictive replay held to the law of the body's own source text, without a GPU (tests/temper_fuzz.py predictive_laws).

tests/predictive_ref.py's Replay builds its shadow table from the TRACER's site table, so a lowering mistake is in the
predictive kernel and in the replay alike.  Here the replay's draws of the fixed `interleaved` body (four plated sites: Normal,
Gamma, flip, Beta; latents declared between them; a plate's value read as data) and of random bodies are compared, per plated
address, with the law that the float64 evaluation of the SOURCE TEXT gives each (particle, row) — at the very seeds, keys,
sizes and bodies tests/test_gpu_predictive_fuzz.py runs the kernel at, which holds the kernel bit for bit to this replay.
Five mutations of the shadow table must each FAIL the laws; the generated kernels of these many-site bodies compile for
gfx950; and `predictive(args=...)` refuses a body in which a plated site's value, which nothing observes there, feeds a later
site."""

import numpy as np
import pytest
import torch

import genjax
import plate_ref as P
import predictive_ref as Q
import temper_fuzz as F
from genjax._amd import abi, temper
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax.inference.smc import TemperedSMC
from offline import kernel_notes, ops  # noqa: F401  (ops: a fixture)

IMPLS = ("threefry", "philox")
MAX_DROPPED, MAX_UNLOWERED = 0.10, 0.15  # shares of the generated bodies (tests/test_temper_fuzz_cpu.py's caps)
COMPILED_BODIES = 2                      # random bodies compiled offline per generator, next to the interleaved one


def _laws(src, latents, obs, args, replay, y, context=""):
    """The replay's draws y [S, D, n] against the source text's laws, by address -> ssm_fuzz.check_laws' worst ratios."""
    return F.check_predictive(src, latents, obs, args, F.draws_by_address(replay.addrs, np.transpose(y, (0, 2, 1))), context)


def _worse(a, b):
    return {k: max(a.get(k, 0.0), v) for k, v in b.items()}


@pytest.fixture(scope="module")
def interleaved(oracle_ops):
    args, obs = F.interleaved_inputs()
    with use_ops(oracle_ops):
        tracer = temper.lower(F.target_of(F.INTERLEAVED, args, obs), 64)
    assert [m["addr"] for m in tracer.meta] == [s[0] for s in F.INTERLEAVED_SITES]
    return dict(args=args, obs=obs, tracer=tracer)


def _interleaved_draws(oracle_ops, c, what, n, D, key, tracer=None, inputs=None):
    """-> (replay, y [4, D, n], latents, (args, obs) of the D rows)."""
    tracer = tracer or c["tracer"]
    args, obs = F.head_rows(*(inputs or (c["args"], c["obs"])), D)
    latents = F.interleaved_latents(what, n)
    replay = Q.Replay(oracle_ops, tracer, F.data_of(tracer, D), key.impl)
    assert replay.addrs == ["y1", "y2", "y3", "y4"] and replay.S == 4
    return replay, replay.draws(key, F.columns_of(tracer, latents)), latents, (args, obs)


# ---- the replay against the law ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
def test_interleaved_replay_has_the_laws(oracle_ops, interleaved, impl):
    """The grid of the GPU suite: per D one population of 257 (the smaller ones are its prefixes), and the 1000 x 129 case.  Every
    draw is finite, and wherever n * D >= 16384 the four sites pass their laws."""
    worst, key = {}, genjax.random.key(F.PRED_KEY, impl)
    for D in F.PRED_DS:
        replay, y, latents, (args, obs) = _interleaved_draws(oracle_ops, interleaved, D, max(F.PRED_NS), D, key)
        assert y.shape == (4, D, max(F.PRED_NS)) and np.isfinite(y).all(), D
        if y[0].size >= F.LAW_MIN_DRAWS:
            worst = _worse(worst, _laws(F.INTERLEAVED, latents, obs, args, replay, y, f"interleaved D {D} {impl}"))
    n, D = F.PRED_BIG
    replay, y, latents, (args, obs) = _interleaved_draws(oracle_ops, interleaved, "big", n, D, genjax.random.key(F.PRED_KEY + 1, impl))
    assert np.isfinite(y).all()
    worst = _worse(worst, _laws(F.INTERLEAVED, latents, obs, args, replay, y, f"interleaved big {impl}"))
    print(f"interleaved replay, {impl}: worst Kolmogorov distance / bound {worst['ks']:.3f}, |z| / bound {worst['z']:.3f}")


def test_interleaved_outside_support(oracle_ops, interleaved):
    """Every fourth Gamma / Beta latent outside its support: the laws hold on the particles inside, and a NaN draw, if the
    oracle's samplers make one of an argument outside its domain, belongs to a particle outside."""
    n, D = F.PRED_OUTSIDE
    for impl in IMPLS:
        replay, y, latents, (args, obs) = _interleaved_draws(oracle_ops, interleaved, "outside", n, D, genjax.random.key(F.PRED_KEY + 2, impl))
        ok = F.inside(F.INTERLEAVED_SITES, latents)
        assert (~ok).sum() >= n // 4 and not np.isnan(y[:, :, ok]).any()
        w = _laws(F.INTERLEAVED, latents, obs, args, replay, y, f"outside {impl}")
        print(f"outside support, {impl}: {int(ok.sum())} of {n} particles inside; NaN draws {int(np.isnan(y).sum())}; worst ratios {w['ks']:.3f} {w['z']:.3f}")


def test_interleaved_api_cases(oracle_ops, interleaved):
    """The public-API cases of the GPU suite (n = 300, stride 4): the fitted rows, and a lowering of 33 held-out rows."""
    n, D, H = F.PRED_API
    key = genjax.random.key(F.PRED_KEY + 3, "philox")
    replay, y, latents, (args, obs) = _interleaved_draws(oracle_ops, interleaved, "api", n, D, key)
    cut = {k: v[::4] for k, v in latents.items()}
    _laws(F.INTERLEAVED, cut, obs, args, replay, y[:, :, ::4], "api, fitted rows")
    held = F.heldout_inputs()
    with use_ops(oracle_ops):
        tracer = temper.lower(F.target_of(F.INTERLEAVED, *held), 64)
    replay, y, latents, (args, obs) = _interleaved_draws(oracle_ops, interleaved, "api", n, H, key, tracer=tracer, inputs=held)
    _laws(F.INTERLEAVED, cut, obs, args, replay, y[:, :, ::4], "api, held-out rows")


@pytest.mark.parametrize("impl", IMPLS)
def test_random_bodies(oracle_ops, impl):
    """PRED_PER_SEED bodies of each of the four seeds' streams: every body with a plated site whose laws cover 0.9 of its entries
    and that lowers is replayed at n = 257, D = 65 and passes the laws of its source text, address by address; the replay at
    D = 2 is finite.  At most 10 % of the generated bodies may be dropped for coverage and 15 % may fail to lower."""
    n, (D, D2) = F.PRED_RANDOM
    total, kept, flat, dropped, unlowered, worst, s_hist = 0, 0, 0, [], [], {"ks": 0.0, "z": 0.0}, {}
    with use_ops(oracle_ops):
        for seed in F.PRED_SEEDS:
            for i, src, sites, args, obs, latents, reasons in F.predictive_stream(seed):
                total += 1
                if reasons == ["no plated site"]:
                    flat += 1
                    continue
                if reasons:
                    dropped.append(f"seed {seed} body {i}: {'; '.join(reasons)}")
                    continue
                try:
                    tracer = temper.lower(F.target_of(src, args, obs), 64)
                except PlanUnsupported as e:
                    unlowered.append(f"seed {seed} body {i}: {e}")
                    continue
                key = genjax.random.key(F.PRED_KEY + 100 + i, impl)
                cols = F.columns_of(tracer, latents)
                replay = Q.Replay(oracle_ops, tracer, F.data_of(tracer, D), key.impl)
                assert replay.addrs == [name for name, role, _ in sites if role == "plated"]
                y = replay.draws(key, cols)
                assert np.isfinite(y).all() and np.isfinite(Q.Replay(oracle_ops, tracer, F.data_of(tracer, D2), key.impl).draws(key, cols)).all()
                worst = _worse(worst, _laws(src, latents, obs, args, replay, y, f"seed {seed} body {i} {impl}\n{src}\nargs {args[3:]}"))
                s_hist[replay.S] = s_hist.get(replay.S, 0) + 1
                kept += 1
    print(f"{impl}: generated {total}, without a plated site {flat}, dropped {len(dropped)} (cap {MAX_DROPPED}), unlowered {len(unlowered)} "
          f"(cap {MAX_UNLOWERED}), compared {kept} (plated sites per body: {dict(sorted(s_hist.items()))}); worst Kolmogorov distance / bound "
          f"{worst['ks']:.3f}, |z| / bound {worst['z']:.3f}")
    for r in dropped + unlowered:
        print("  ", r)
    assert total == len(F.PRED_SEEDS) * F.PRED_PER_SEED == kept + flat + len(dropped) + len(unlowered)
    assert len(dropped) <= MAX_DROPPED * total and len(unlowered) <= MAX_UNLOWERED * total
    assert max(s_hist) >= 4 and kept >= 0.6 * total


# ---- mutations of the shadow table ------------------------------------------------------------------------------------------
def _prog(a):
    return [(o.op, o.ref, o.value) for o in (abi.ExprOp * a.ref).from_address(a.table)]


def _n_args(s):
    return 1 if s.dist == abi.DIST_BERNOULLI else 2


def _map_inputs(replay, fn, sites=None):
    """Every input-column reference of `sites` (all of them), plain or inside a program, through fn(column) -> the number changed."""
    changed = 0
    for s in replay.sites if sites is None else sites:
        for k in range(_n_args(s)):
            a = s.arg[k]
            if a.kind == abi.ARG_INPUT:
                new = fn(a.ref)
                changed, a.ref = changed + (new != a.ref), new
            elif a.kind == abi.ARG_EXPR:
                prog = _prog(a)
                new = [(op, fn(ref) if op == abi.EXPR_INPUT else ref, v) for op, ref, v in prog]
                if new != prog:
                    changed, s.arg[k] = changed + 1, abi.expr_arg(new, replay.keep)
    return changed


def _inputs_of(s):
    return [r for k in range(_n_args(s)) for r in ([s.arg[k].ref] if s.arg[k].kind == abi.ARG_INPUT else
                                                    [ref for op, ref, _ in _prog(s.arg[k]) if op == abi.EXPR_INPUT] if s.arg[k].kind == abi.ARG_EXPR else [])]


def _same_arg(a, b):
    if a.kind != b.kind:
        return False
    if a.kind == abi.ARG_EXPR:
        return _prog(a) == _prog(b)
    return (a.ref, a.scale, a.offset) == (b.ref, b.scale, b.offset)


def _mutate(oracle_ops, replay, which, args):
    """Mutates the shadow table of `replay` in place and rebuilds its plan -> True, or False when the body does not hold the
    feature.  (The product is not touched: the replay holds copies.)"""
    C, L = len(replay.data), replay.L
    hit = False
    if which == "swap_columns":         # (a) two DATA operands change places wherever they are read: xs and zs where the table
        # holds both (the interleaved body), else the first two data columns the sites read (a random body mostly reads columns
        # the body computed from its arguments before they met a traced value)
        col = [next((i for i, c in enumerate(replay.data) if np.array_equal(c, args[k][:replay.D])), None) for k in (0, 1)]
        if col[0] is None or col[1] is None:
            read = list(dict.fromkeys(r for s in replay.sites for r in _inputs_of(s) if r < C))
            col = read[:2] if len(read) >= 2 else None
        if col:
            sw = {col[0]: col[1], col[1]: col[0]}
            hit = _map_inputs(replay, lambda r: sw.get(r, r)) > 0
    elif which == "wrong_latent":       # (b) every reference to the first latent the sites read goes to the neighbouring input
        lat = [r for s in replay.sites for r in _inputs_of(s) if r >= C]  # column C + l +- 1 (a renumbering that is off by one)
        if lat:
            l = lat[0] - C
            to = C + l + 1 if l + 1 < L else C + l - 1
            hit = _map_inputs(replay, lambda r: to if r == lat[0] else r) > 0
    elif which == "affine_sign":        # (c) scale * column + offset becomes -scale * column + offset
        for s in replay.sites:
            for k in range(_n_args(s)):
                if not hit and s.arg[k].kind == abi.ARG_INPUT and s.arg[k].scale != 0.0:
                    s.arg[k].scale, hit = -s.arg[k].scale, True
    elif which == "swap_args":          # (d) the two arguments of the first two-argument site that reads a column and whose
        for s in replay.sites:          # arguments differ (two literals may lie as close as the body's arithmetic puts them)
            if _n_args(s) == 2 and _inputs_of(s) and not _same_arg(s.arg[0], s.arg[1]):
                a0, a1 = abi.Arg.from_buffer_copy(s.arg[0]), abi.Arg.from_buffer_copy(s.arg[1])
                s.arg[0], s.arg[1], hit = a1, a0, True
                break
    elif which == "other_observed":     # (e) the last site with a data operand reads ANOTHER plated site's observed column there
        for q in range(replay.S - 1, -1, -1):
            s = replay.sites[q]
            dat = [r for r in _inputs_of(s) if r < C]
            to = next((c for p, c in enumerate(replay.obs_col) if p != q and dat and c != dat[0]), None)
            if to is not None:
                hit = _map_inputs(replay, lambda r: to if r == dat[0] else r, [s]) > 0
                break
    else:
        raise ValueError(which)
    if hit:
        replay.plan = oracle_ops.plan_create(replay.sites)
        if replay.params:
            replay.plan.set_params(replay.params)
    return hit


MUTATIONS = ("swap_columns", "wrong_latent", "affine_sign", "swap_args", "other_observed")
MUTATION_SEED, MUTATION_BODIES = 500, 10


def _replay(oracle_ops, tracer, D, impl):
    r = Q.Replay(oracle_ops, tracer, F.data_of(tracer, D), impl)
    r.params = tracer.params
    return r


@pytest.mark.parametrize("which", MUTATIONS)
def test_mutations_fail_the_laws_interleaved(oracle_ops, interleaved, which):
    """The 257 x 129 case of the grid under PHILOX: the unmutated replay passes (test_interleaved_replay_has_the_laws), every
    mutated one fails."""
    n, D = max(F.PRED_NS), 129
    key = genjax.random.key(F.PRED_KEY, "philox")
    args, obs = F.head_rows(interleaved["args"], interleaved["obs"], D)
    latents = F.interleaved_latents(D, n)
    replay = _replay(oracle_ops, interleaved["tracer"], D, key.impl)
    assert _mutate(oracle_ops, replay, which, args)
    y = replay.draws(key, F.columns_of(interleaved["tracer"], latents))
    with pytest.raises(AssertionError, match="law of") as e:
        _laws(F.INTERLEAVED, latents, obs, args, replay, y)
    print(which, "->", str(e.value).splitlines()[0])


@pytest.fixture(scope="module")
def mutation_cases(oracle_ops):
    """Bodies of the stream MUTATION_SEED that the suite compares (a plated site, covered, lowers), with their unmutated replays
    checked: each mutation takes the first ten that hold its feature."""
    out = []
    n, (D, _) = F.PRED_RANDOM
    with use_ops(oracle_ops):
        for i, src, sites, args, obs, latents, reasons in F.predictive_stream(MUTATION_SEED, 60):
            if reasons:
                continue
            try:
                tracer = temper.lower(F.target_of(src, args, obs), 64)
            except PlanUnsupported:
                continue
            key = genjax.random.key(F.PRED_KEY + 200 + i, "philox")
            replay = _replay(oracle_ops, tracer, D, key.impl)
            y0 = replay.draws(key, F.columns_of(tracer, latents))
            _laws(src, latents, obs, args, replay, y0, src)  # (the unmutated replay passes)
            out.append((i, src, args, obs, latents, tracer, key, y0))
    return out


@pytest.mark.parametrize("which", MUTATIONS)
def test_mutations_fail_the_laws_random(oracle_ops, mutation_cases, which):
    """Each mutation fails the laws on every one of the first ten random bodies that hold the mutated feature.  (A mutated table
    whose draws are the unmutated one's bit for bit — two columns exchanged across a commutative operation — is no mutation.)"""
    n, (D, _) = F.PRED_RANDOM
    done = 0
    for i, src, args, obs, latents, tracer, key, y0 in mutation_cases:
        replay = _replay(oracle_ops, tracer, D, key.impl)
        if not _mutate(oracle_ops, replay, which, args):
            continue
        y = replay.draws(key, F.columns_of(tracer, latents))
        if Q.same_bits(y, y0):
            continue
        with pytest.raises(AssertionError, match="law of"):
            _laws(src, latents, obs, args, replay, y, f"{which} on body {i}\n{src}")
            print(f"{which} passed the laws on body {i}\n{src}\nargs {args[3:]}")
        done += 1
        if done == MUTATION_BODIES:
            break
    assert done == MUTATION_BODIES


# ---- offline compilation ------------------------------------------------------------------------------------------------------
def _compile(plan, tmp_path, name, impl):
    assert plan.predictive_compile_check(impl) == 0, (name, impl)
    k = kernel_notes(plan.predictive_source(impl), tmp_path, f"predictive_{name}_{impl}")["gjx_predictive_kernel"]
    print(f"predictive kernel, {name}, generator {impl}: {k}")  # (profiles/predictive_fuzz_summary.md records these)
    return k


@pytest.mark.parametrize("impl", [0, 1])
def test_many_site_kernels_compile(ops, tmp_path, impl):  # noqa: F811
    """The generated predictive kernel of the interleaved body (S = 4) and of the first random bodies of the first seed's stream
    compiles for gfx950; the registers and scratch of each are printed.  No register limit is asserted: nothing derives one for
    an arbitrary number of sites."""
    with use_ops(ops):
        tracer = temper.lower(F.target_of(F.INTERLEAVED, *F.interleaved_inputs()), 64)
        plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
        src = plan.predictive_source(impl)
        assert "PredictiveAcc qA[4], qB[4];" in src
        _compile(plan, tmp_path, "interleaved", impl)
        done = 0
        for i, src, sites, args, obs, latents, reasons in F.predictive_stream(F.PRED_SEEDS[0]):
            if reasons or done == COMPILED_BODIES:
                continue
            try:
                tracer = temper.lower(F.target_of(src, args, obs), 64)
            except PlanUnsupported:
                continue
            plan = ops.temper_plan_create(tracer.sites, keep=(tracer.keep, tracer))
            S = sum(role == "plated" for _, role, _ in sites)
            assert f"PredictiveAcc qA[{S}], qB[{S}];" in plan.predictive_source(impl)
            _compile(plan, tmp_path, f"seed{F.PRED_SEEDS[0]}_body{i}_S{S}", impl)
            done += 1
    assert done == COMPILED_BODIES


# ---- args=: nothing observed ---------------------------------------------------------------------------------------------------
def test_args_refuses_a_plate_that_feeds_a_later_site(ops):  # noqa: F811
    """`interleaved`: y4 = beta(u * ps + 0.5, 1.0 + y1 * y1) reads y1's VALUE.  Under args= nothing is observed at y1, so the
    call is refused with both addresses in the message, before anything is launched (no device is there to launch on)."""
    args, obs = F.head_rows(*F.interleaved_inputs(), 20)
    cols = [torch.zeros(8) + 0.5 for _ in range(4)]
    key = genjax.random.key(0, "philox")
    with use_ops(ops):
        alg = TemperedSMC(F.target_of(F.INTERLEAVED, args, obs), 64)
        new = tuple(torch.from_numpy(a[:7].copy()) if isinstance(a, np.ndarray) else a for a in args)
        with pytest.raises(PlanUnsupported, match=r"'y4' reads the value of the plated site at address 'y1'"):
            alg.predictive(cols, key, args=new)
        with pytest.raises(PlanUnsupported, match=r"'y4'.*'y1'"):
            alg._unobserved_target(alg._state(), new)

    # a value that reaches the later site DIRECTLY (the observed column itself, no column computed from it)
    direct = '''def model(xs, zs, ps, s, t):
    a = normal(0.0, 1.5) @ "a"
    y1 = normal(a * xs, s) @ "y1"
    normal(a * zs, 0.5) @ "y2"
    normal(y1, 0.3) @ "y3"
'''
    d_obs = {"y1": obs["y1"], "y2": obs["y1"] + np.float32(1.0), "y3": obs["y1"] - np.float32(1.0)}
    with use_ops(ops):
        alg = TemperedSMC(F.target_of(direct, args, d_obs), 64)
        with pytest.raises(PlanUnsupported, match=r"'y3' reads the value of the plated site at address 'y1'"):
            alg.predictive(cols[:1], key, args=new)


def test_args_still_lowers_bodies_without_such_a_dependency(ops):  # noqa: F811
    """two_plate and plate_ref.MODELS: no plated site reads another's value — the unobserved target is built as before, every
    plated address constrained to zeros of the new length (the GPU suite compares its draws with the target= call's)."""
    xs, zs, y1, y2 = P.two_plate_data(20)
    with use_ops(ops):
        alg = TemperedSMC(F.target_of(P.TWO_PLATE, (xs, zs), {"y1": y1, "y2": y2}), 64)
        new = (torch.from_numpy(xs[:7].copy()), torch.from_numpy(zs[:7].copy()))
        t = alg._unobserved_target(alg._state(), new)
        assert torch.equal(t.constraint["y1"], torch.zeros(7)) and torch.equal(t.constraint["y2"], torch.zeros(7))
        assert temper.lower(t, 64).data_rows == 7
        for name in P.MODELS:
            target, _ = P.target(name, 20)
            held, _ = P.target(name, 7, seed=7)
            alg = TemperedSMC(target, 64)
            t = alg._unobserved_target(alg._state(), held.args)
            assert torch.equal(t.constraint["y"], torch.zeros(7)) and temper.lower(t, 64).data_rows == 7, name
