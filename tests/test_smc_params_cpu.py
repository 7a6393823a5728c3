"""Parameterised state-space models (include/gjx_smc_params.h), everything that needs no GPU: the lowering and its slot
rows, the generated source (no value of theta in it, compiled for gfx950 by the library's own helper, its register and
scratch budget against the baked-constant kernel of the same model), every stated error code and message, the header's
symbols, and ParticleMH driven by an exact Kalman likelihood."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import guided_ref as G
import smc_params_ref as R
from genjax import categorical, gen, normal
from genjax._amd import abi, prng, workloads as W
from genjax._amd.abi import GjxError
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax._amd.smc_plan import ParamSpace, build_guided_plan, build_smc_plan
from genjax.inference.smc import BootstrapSMC, GuidedSMC, ParticleMH, StateSpaceModel
from offline import ROOT, header_symbols, kernel_notes, ops  # noqa: F401

Y = [("y",)]
SYMBOLS = {"gjx_smc_params_version", "gjx_smc_plan_create_params", "gjx_smc_plan_set_params"}
INVALID, UNSUPPORTED = -1, -2


def _plan(ops, model, theta):
    with use_ops(ops):
        return build_smc_plan(model, Y, theta)[0]


# ---- the header and its bindings ---------------------------------------------------------------------------------------
def test_the_header_is_exported_by_the_hip_library_only(ops, oracle_ops):
    h = abi.PLAN_HEADERS["smc_params"]
    assert h in abi.all_optional_headers()
    syms = header_symbols(h.header)
    assert h.header == "gjx_smc_params.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.prototypes is abi.SMC_PARAMS_PROTOTYPES and h.version == abi.SMC_PARAMS_ABI_VERSION
    assert h.unavailable is abi.SmcParamsUnavailable
    assert not (syms & header_symbols("gjx.h")) and not (syms & set(abi.PROTOTYPES))
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_smc_params and ops.lib.has["smc_params"] and not oracle_ops.lib.has_smc_params
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_smc_params_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == abi.SMC_PARAMS_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", h.header)).read()
    assert f"GJX_SMC_PARAMS_VERSION_MAJOR {major.value}" in hdr and f"GJX_SMC_PARAMS_VERSION_MINOR {minor.value}" in hdr
    assert f"GJX_SMC_PARAMS_MAX_ROWS {abi.SMC_PARAMS_MAX_ROWS}" in hdr
    # the tables the earlier headers' suites pin are as they were
    assert list(abi.OPTIONAL_HEADERS) == ["paths", "guided", "backsim"] and list(abi.EXTENSION_HEADERS) == ["backmove"]


def test_the_oracle_says_the_header_is_missing(oracle_ops):
    with use_ops(oracle_ops):
        with pytest.raises(abi.SmcParamsUnavailable, match="gjx_smc_plan_create_params") as e:
            build_smc_plan(R.lgssm_param_model(), Y, (0.9, 1.0, 0.5))
    assert e.value.code == UNSUPPORTED and isinstance(e.value, GjxError)


# ---- the lowering ------------------------------------------------------------------------------------------------------
def test_slot_layout_lgssm(ops):
    theta = R.lgssm_rows(1)[0]
    plan = _plan(ops, R.lgssm_param_model(), theta)
    sp = plan._space
    assert plan.n_params == sp.n_slots == 3 and sp.names == R.LGSSM_NAMES  # theta alone: nothing is derived
    ti, ts = plan._tables
    # init: x latent with constants; y observed with scale = slot 2 (r)
    assert (ti[1].arg[1].kind, ti[1].arg[1].ref, ti[1].arg[1].scale, ti[1].arg[1].offset) == (abi.ARG_PARAM, 2, 1.0, 0.0)
    # step: loc a * x is a program with a parameter leaf, scale q is slot 1, the observed scale r is slot 2
    assert ts[0].arg[0].kind == abi.ARG_EXPR and (ts[0].arg[1].kind, ts[0].arg[1].ref) == (abi.ARG_PARAM, 1)
    assert (ts[1].arg[1].kind, ts[1].arg[1].ref) == (abi.ARG_PARAM, 2)
    src = plan.source(1)
    assert "(prm.p[0] * st_0)" in src and "prm.p[1]" in src and "prm.p[2]" in src
    assert "prm.d[2]" in src and "prm.d[3]" in src  # the observed site's 1 / r and log normaliser, derived per row


def test_derived_slots_in_first_use_order(ops):
    theta = R.gamma_rows(1)[0]
    m, s, k = R.f32s(theta)
    plan = _plan(ops, R.gamma_param_model(), theta)
    sp = plan._space
    # slots 0..2 are theta; then init's 0.5 * s, then step's s * s and 0.5 * s, each where a site first takes it
    assert sp.n_slots == plan.n_params == 6
    want = np.asarray([m, s, k, 0.5 * s, s * s, 0.5 * s], dtype=np.float32)
    assert np.array_equal(np.asarray(sp.values, dtype=np.float32), want)
    ti, ts = plan._tables
    assert (ti[0].arg[1].kind, ti[0].arg[1].ref) == (abi.ARG_PARAM, 2)  # gamma(2, k)
    assert [(a.kind, a.ref) for a in (ti[1].arg[0], ti[1].arg[1])] == [(abi.ARG_PARAM, 0), (abi.ARG_PARAM, 1)]
    assert (ti[2].arg[1].kind, ti[2].arg[1].ref) == (abi.ARG_PARAM, 3)
    assert (ts[1].arg[1].kind, ts[1].arg[1].ref) == (abi.ARG_PARAM, 4) and (ts[2].arg[1].kind, ts[2].arg[1].ref) == (abi.ARG_PARAM, 5)
    init_state, next_state = plan._state_args
    assert next_state[1].kind == abi.ARG_EXPR  # g2 * k + 0.1: a parameter inside a carry expression
    assert "prm.p[2]" in plan.source(0).split("out.s[1] =")[1].split("\n")[0]


@pytest.mark.parametrize("name", list(R.MODELS))
def test_a_row_from_the_derivations_equals_a_fresh_trace(ops, name):
    make, _, rows = R.MODELS[name]
    th = rows(5)
    plan = _plan(ops, make(), th[0])
    for f in range(1, 5):
        fresh = _plan(ops, make(), th[f])
        want = np.asarray(fresh._space.values, dtype=np.float32)
        got = plan._space.row(th[f])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, f)
        assert fresh.source(1) == plan.source(1)  # the structure does not depend on where the bodies were traced
    assert np.array_equal(plan._space.rows(th)[3], plan._space.row(th[3]))


def test_param_space_rounds_theta_to_f32():
    sp = ParamSpace(("a",), [0.1])
    assert sp.values == [float(np.float32(0.1))] and sp.row([0.1])[0] == np.float32(0.1)
    with pytest.raises(ValueError, match="declares 1 parameters"):
        sp.row([0.1, 0.2])


# ---- the generated source ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.MODELS))
@pytest.mark.parametrize("impl", [0, 1])
def test_compile_check(ops, name, impl):
    make, _, rows = R.MODELS[name]
    assert _plan(ops, make(), rows(1)[0]).compile_check(impl) == 0


@pytest.mark.parametrize("name", list(R.MODELS))
def test_the_source_holds_no_value_of_theta(ops, name):
    make, literal, rows = R.MODELS[name]
    th = rows(3)
    plan = _plan(ops, make(), th[0])
    before = [plan.source(impl) for impl in (0, 1)]
    plan.set_params(plan._space.rows(th[1:]))
    assert [plan.source(impl) for impl in (0, 1)] == before
    lits = {f"0x{int(np.float32(v).view(np.uint32)):08x}u" for f in range(3) for v in plan._space.row(th[f])}
    lits -= {"0x3f000000u", "0x3f800000u", "0x00000000u"}  # (0.5, 1 and 0 are the bodies' own literals)
    with use_ops(ops):
        baked = build_smc_plan(literal(th[0]), Y)[0].source(1)
    assert any(l in baked for l in lits)  # the literal model does carry them ...
    for src in before:
        assert "prm_rows" in src and "GenStepPrm" in src and "GenInitPrm" in src
        for l in lits:  # ... the parameterised one carries none
            assert l not in src, l


def test_a_plain_plan_keeps_its_source(ops):
    """A model without parameters generates what it generated before: no parameter table in its kernels' signatures."""
    with use_ops(ops):
        src = build_smc_plan(StateSpaceModel(*G.lgssm_model(0.5)), Y)[0].source(1)
    assert "prm" not in src
    assert "void gjx_smc_step_kernel(ResampleArgs A, PlanPolicyArgs PA, PlanTables T) {" in src


@pytest.mark.parametrize("impl", [0, 1])
def test_register_and_scratch_budget(ops, tmp_path, impl):
    """The LGSSM user model: the parameterised step kernel against the baked-constant kernel of the same model from the same
    build — no scratch, and at most one allocation granule (8) more VGPRs: parameters arrive by scalar loads and live in
    SGPRs; an SGPR operand can need a copy where a literal did not, never more."""
    with use_ops(ops):
        baked = build_smc_plan(StateSpaceModel(*G.lgssm_model(0.5)), Y)[0]
    param = _plan(ops, R.lgssm_param_model(), (G.A, G.Q, 0.5))
    nb = kernel_notes(baked.source(impl), tmp_path, f"baked{impl}")
    np_ = kernel_notes(param.source(impl), tmp_path, f"param{impl}")
    for kernel in ("gjx_smc_step_kernel", "gjx_smc_step_kernel_adaptive", "gjx_smc_init_kernel"):
        print(impl, kernel, "baked", nb[kernel], "parameterised", np_[kernel])
        assert np_[kernel]["private_segment_fixed_size"] == 0, kernel
    assert np_["gjx_smc_step_kernel"]["vgpr_count"] <= nb["gjx_smc_step_kernel"]["vgpr_count"] + 8


# ---- error codes -------------------------------------------------------------------------------------------------------
def _cfg(ops, n=1000, T=3, F=1):
    sk, rk = W.smc_key_schedule(prng.key(0, "philox"), T)
    if F > 1:
        sk, rk = np.stack([sk] * F), np.stack([rk] * F)
    return ops.smc_config(1, n, 0, n, sk, rk)


def _run(ops, plan, cfg):
    """gjx_smc_run_plan over dummy non-null addresses: the refusals below are decided on the host, before any launch."""
    d = C.c_void_p(0x1000)
    cols = (C.c_void_p * plan.n_state)(*[0x1000] * plan.n_state)
    obs = (C.c_float * (cfg.n_steps * max(plan.n_obs, 1)))()
    return ops.lib._gjx_smc_run_plan(C.byref(cfg), plan.handle, obs, d, d, cols, d, None, d, 1 << 20, None)


def test_run_before_set_params_and_row_counts(ops):
    plan = _plan(ops, R.lgssm_param_model(), (0.9, 1.0, 0.5))
    assert _run(ops, plan, _cfg(ops)) == INVALID  # no rows yet
    plan.set_params(plan._space.rows(R.lgssm_rows(3)))
    assert _run(ops, plan, _cfg(ops, F=4)) == INVALID  # three rows, four filters
    assert _run(ops, plan, _cfg(ops, F=1)) == INVALID  # three rows, one filter
    plan.set_params(plan._space.rows(R.lgssm_rows(4)))
    assert _run(ops, plan, _cfg(ops, F=3)) == INVALID


def test_the_table_walking_route_is_refused(ops, monkeypatch):
    plan = _plan(ops, R.lgssm_param_model(), (0.9, 1.0, 0.5))
    plan.set_params(plan._space.row((0.9, 1.0, 0.5)))
    monkeypatch.setenv("GJX_PLAN_JIT", "0")
    assert _run(ops, plan, _cfg(ops)) == UNSUPPORTED


def test_peers_and_the_sharded_driver_are_refused(ops):
    plan = _plan(ops, R.lgssm_param_model(), (0.9, 1.0, 0.5))
    plan.set_params(plan._space.row((0.9, 1.0, 0.5)))
    cfg = _cfg(ops)
    peers = abi.SmcPeers()
    cfg.peers = C.pointer(peers)
    assert _run(ops, plan, cfg) == UNSUPPORTED
    g, comm = C.c_void_p(), C.c_void_p()
    ops.lib.call("gjx_comm_group_create", 1, C.byref(g))
    ops.lib.call("gjx_comm_init_local", g, 0, C.byref(comm))
    try:
        assert ops.lib._gjx_smc_sharded_run_plan(comm, None, plan.handle, None, None, None) == UNSUPPORTED
    finally:
        ops.lib.call("gjx_comm_destroy", comm)
        ops.lib.call("gjx_comm_group_destroy", g)


def test_creator_and_setter_refusals(ops):
    with use_ops(ops):
        plain = build_smc_plan(StateSpaceModel(*G.lgssm_model(0.5)), Y)[0]
    row = (C.c_float * 3)(0.9, 1.0, 0.5)
    assert ops.lib._gjx_smc_plan_set_params(plain.handle, row, 1) == INVALID  # not a parameterised plan
    plan = _plan(ops, R.lgssm_param_model(), (0.9, 1.0, 0.5))
    for n_rows in (0, -1, abi.SMC_PARAMS_MAX_ROWS + 1):
        assert ops.lib._gjx_smc_plan_set_params(plan.handle, row, n_rows) == INVALID
    assert ops.lib._gjx_smc_plan_set_params(plan.handle, None, 1) == INVALID
    with pytest.raises(ValueError, match="rows of 3 values"):
        plan.set_params([0.9, 1.0])
    ti, ts = plan._tables
    init_state, next_state = plan._state_args
    for n_params in (0, 2, abi.MAX_PARAMS + 1):  # none; slot 2 is referenced; too many
        with pytest.raises(GjxError, match="GJX_ERR_INVALID|-1"):
            ops.smc_plan_create(ti, ts, init_state, next_state, 1, n_params=n_params) if n_params else \
                ops.lib.call("gjx_smc_plan_create_params", None, None, 0, None, 0, 0, C.byref(C.c_void_p()))
    with pytest.raises(GjxError):  # the creators of gjx.h keep refusing parameters in SMC tables
        ops.smc_plan_create(ti, ts, init_state, next_state, 1)


# ---- refusals of the Python layer ---------------------------------------------------------------------------------------
def _structure_model(body):
    @gen
    def init(theta):
        x = normal(0.0, 1.0) @ "x"
        normal(x, 0.5) @ "y"
        return x

    return StateSpaceModel(init, gen(body), params=("a", "b"))


def test_parameters_as_structure_are_refused_by_name(ops):
    def compares(x, theta):
        a, b = theta
        x2 = normal(x if a > 0 else -x, 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    def floats(x, theta):
        a, b = theta
        x2 = normal(float(b) * x, 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    def indexes(x, theta):
        a, b = theta
        x2 = normal([0.5, 0.9][b] * x, 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    def integer_argument(x, theta):
        a, b = theta
        categorical(logits=a) @ "z"
        x2 = normal(x, 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    def derived(x, theta):
        a, b = theta
        x2 = normal(x, 1.0 if (2.0 * b) < 1.0 else 2.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    for body, name in ((compares, "a"), (floats, "b"), (indexes, "b"), (integer_argument, "a"), (derived, "b")):
        with use_ops(ops):
            with pytest.raises(PlanUnsupported, match=f"model parameter '{name}' used as structure"):
                build_smc_plan(_structure_model(body), Y, (0.5, 1.0))


def test_params_arguments_are_checked(ops):
    obs = R.observations(4)
    with pytest.raises(ValueError, match="declares parameters"):
        BootstrapSMC(StateSpaceModel(*G.lgssm_model(0.5)), obs, 100, params=(0.9,))
    with pytest.raises(ValueError, match="declares 3 parameters"):
        BootstrapSMC(R.lgssm_param_model(), obs, 100, params=(0.9, 1.0))
    smc = BootstrapSMC(R.lgssm_param_model(), obs, 100)
    with use_ops(ops):
        with pytest.raises(ValueError, match="pass params="):
            smc.run(prng.key(0, "philox"))
        with pytest.raises(ValueError, match="one row per key"):
            smc.run_many([prng.key(0, "philox")] * 3, params=R.lgssm_rows(2))
    with pytest.raises(ValueError, match="distinct parameter names"):
        StateSpaceModel(*G.lgssm_model(0.5), params=("a", "a"))
    assert StateSpaceModel(*G.lgssm_model(0.5)).params == ()


def test_smoothing_and_sharding_refuse_a_parameterised_model(ops):
    from genjax._amd.dist import ShardedSMC
    from genjax._amd.smc_plan import build_transition_table

    obs = R.observations(4)
    smc = BootstrapSMC(R.lgssm_param_model(), obs, 100, record_history=True, params=(0.9, 1.0, 0.5))
    with pytest.raises(PlanUnsupported, match="build the model at a fixed θ to smooth"):
        smc.backward_simulate(None, prng.key(0, "philox"), 10)
    with use_ops(ops):
        with pytest.raises(PlanUnsupported, match="build the model at a fixed θ to smooth"):
            build_transition_table(R.lgssm_param_model(), Y)
    plan = _plan(ops, R.lgssm_param_model(), (0.9, 1.0, 0.5))
    with pytest.raises(PlanUnsupported, match="ShardedSMC: a parameterised plan"):
        ShardedSMC(ops, "plan", 1, 0, 1024, 4, 0, 1, plan=plan, obs=np.zeros((4, 1), np.float32), comm=object())


def test_guided_proposals_take_theta(ops):
    @gen
    def track_q(carry, y, theta):
        a, q, r = theta
        normal(0.5 * (a * carry) + 0.5 * y, q) @ "x"

    @gen
    def start_q(y, theta):
        a, q, r = theta
        normal(0.5 * y, 2.0 * r) @ "x"

    with use_ops(ops):
        plan, n_state = build_guided_plan(R.lgssm_param_model(), Y, track_q, start_q, theta=(0.9, 1.0, 0.5))
    assert n_state == 1 and plan.n_params == 4  # theta and 2 r
    assert G.modes(plan._tables[0]) == [abi.SITE_PROPOSED, abi.SITE_GUIDED, 1]
    assert G.modes(plan._tables[1]) == [abi.SITE_PROPOSED, abi.SITE_GUIDED, 1]
    for impl in (0, 1):
        assert plan.compile_check(impl) == 0
    assert GuidedSMC(R.lgssm_param_model(), R.observations(4), 100, track_q, start_q, params=(0.9, 1.0, 0.5))._parameterised


# ---- ParticleMH with an exact likelihood ------------------------------------------------------------------------------
def _kalman_rows(y):
    def ll(rows):
        return np.asarray([R.kalman_log_likelihood(float(a), y) for a in rows[:, 0]])

    return ll


def test_particle_mh_with_the_exact_likelihood_meets_the_criterion():
    y = W.lgssm_data(50)
    exact = R.exact_posterior_mean_a(y)
    assert abs(exact - 0.4729) < 5e-4
    seen = []

    def ll(rows):
        seen.append(np.array(rows))
        return _kalman_rows(y)(rows)

    for seed in range(10):
        pm = ParticleMH(None, R.uniform_log_prior, 0.15, n_chains=8, log_likelihood=ll)
        samples, lls, acc = pm.run(prng.key(seed, "philox"), [0.5], 400)
        assert samples.shape == (401, 8, 1) and lls.shape == (401, 8) and acc.shape == (400, 8) and acc.dtype == bool
        err, bound = R.chains_criterion(samples, exact)
        print(f"seed {seed}: |mean - exact| = {err:.4f}, bound = {bound:.4f}, acceptance = {acc.mean():.2f}")
        assert err <= bound, (seed, err, bound)
        assert np.all(np.abs(samples) < 1.0) and np.array_equal(samples, samples.astype(np.float32).astype(np.float64))
    rows = np.concatenate(seen)
    assert rows.dtype == np.float32 and np.all(np.abs(rows) < 1.0)  # no proposal outside the support reached the callable


def test_particle_mh_rejects_out_of_support_proposals_without_running_them():
    calls = []

    def ll(rows):
        calls.append(np.array(rows))
        return np.zeros(len(rows))

    # a wide random walk from the edge of the support: many proposals fall outside
    pm = ParticleMH(None, R.uniform_log_prior, 2.0, n_chains=4, log_likelihood=ll)
    samples, lls, acc = pm.run(prng.key(3, "threefry"), [0.9], 50)
    rng = np.random.default_rng([prng.key(3, "threefry").k0, prng.key(3, "threefry").k1])
    theta = np.full((4, 1), np.float32(0.9), dtype=np.float32)
    outside = 0
    for i in range(1, 51):
        z, u = rng.standard_normal((4, 1)), rng.random(4)
        prop = (theta.astype(np.float64) + 2.0 * z).astype(np.float32)
        live = np.abs(prop[:, 0]) < 1.0
        outside += int((~live).sum())
        assert np.array_equal(calls[i], np.where(live[:, None], prop, theta))  # a dead row runs the chain's current theta
        a = live & (np.log(u) < 0.0)  # flat likelihood, flat prior: every live proposal is accepted
        assert np.array_equal(acc[i - 1], a)
        theta = np.where(a[:, None], prop, theta)
        assert np.array_equal(samples[i], theta.astype(np.float64))
    assert outside > 20 and len(calls) == 51 and all(np.all(np.abs(c) < 1.0) for c in calls)
    with pytest.raises(ValueError, match="n_chains"):
        ParticleMH(None, R.uniform_log_prior, 0.1, n_chains=17, log_likelihood=ll)
    with pytest.raises(TypeError, match="params"):
        ParticleMH(BootstrapSMC(StateSpaceModel(*G.lgssm_model(0.5)), R.observations(3), 10), R.uniform_log_prior, 0.1)
