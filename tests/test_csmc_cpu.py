"""The conditional particle filter without a GPU: the scheme itself (a float64 restatement held to the exact smoother),
include/gjx_csmc.h as one more header (libgjx_hip.so exports it, the oracle does not), what `run(retained=...)`,
`ParticleGibbs` and the C entry points refuse, that asking for the conditional source leaves the unconditional one byte
for byte as it was, and the conditional kernels compiled for gfx950 offline (libgjx_hip.so loaded without a device, as
test_plan_specialization.py does)."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import genjax
import backsim_ref as B
import csmc_ref as R
import guided_ref as G
import smc_params_ref as SP
from genjax import ChoiceMapBuilder as Cm, gen, normal
from genjax._amd import abi
from genjax._amd.abi import GjxError
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax._amd.smc_plan import build_guided_plan, build_smc_plan, check_conditional
from genjax.inference.smc import (BootstrapSMC, DiscreteHMM, GuidedSMC, LinearGaussianSSM, ParticleGibbs, StateSpaceModel)
from offline import ROOT, header_symbols, kernel_notes, ops  # noqa: F401

Y = [("y",)]
INVALID, UNSUPPORTED = -1, -2
SYMBOLS = {"gjx_csmc_version", "gjx_smc_plan_step_conditional", "gjx_csmc_plan_source", "gjx_csmc_plan_compile_check"}


# ---- the scheme --------------------------------------------------------------------------------------------------------
def test_the_restated_sampler_meets_the_exact_smoother():
    """n - 1 teeth plus the forced slot, a leaf by the weights, trace-back — in float64 numpy, at the sizes the device runs."""
    y, mean, var = R.lgssm_truth(R.T_INV)
    paths = R.pg_restatement(y, R.N_INV, R.CHAINS, R.SWEEPS, seed=1)
    R.assert_invariant(paths, mean, var, "restatement")
    # the variant the design refuses (n teeth, the last slot overwritten), same sizes: figures only (profiles/csmc_summary.md)
    wrong = R.pg_restatement(y, R.N_INV, R.CHAINS, R.SWEEPS, seed=1, wrong=True)
    for t, (err, bound, cap) in enumerate(R.invariance(wrong, mean, var)):
        print(f"overwritten n-tooth comb t={t}: |mean - RTS| = {err:.4f}  bound = {bound:.4f}  cap = {cap:.4f}")


def test_the_criterion_rejects_the_overwritten_comb_where_it_can():
    """At the invariance sizes (n = 8) the refused scheme is a few hundredths of a posterior sd off and passes; at n = 2 it
    is 0.15 sd off.  There the same criterion, with its cap, accepts the specified scheme and rejects the refused one: a guard
    of the n - 1-tooth construction next to the bit-exact ancestor pins."""
    y, mean, var = R.lgssm_truth(R.T_INV)
    sizes = (R.N_SHARP, R.CHAINS_SHARP, R.SWEEPS_SHARP)
    R.assert_invariant(R.pg_restatement(y, *sizes, seed=1), mean, var, "n = 2, specified", R.BURN_SHARP)
    inv = R.invariance(R.pg_restatement(y, *sizes, seed=1, wrong=True), mean, var, R.BURN_SHARP)
    for t, (err, bound, cap) in enumerate(inv):
        print(f"n = 2, overwritten n-tooth comb t={t}: |mean - RTS| = {err:.4f}  bound = {bound:.4f}  cap = {cap:.4f}")
    assert all(bound <= cap for _, bound, cap in inv)  # (the bound is meaningful: the rejection is not an artefact of a wide one)
    assert max(err / bound for err, bound, _ in inv) > 2.0, "the criterion no longer tells the refused comb from the specified one"


# ---- the header and its bindings ---------------------------------------------------------------------------------------
def test_the_header_is_exported_by_the_hip_library_only(ops, oracle_ops):
    h = abi.PLAN_HEADERS["csmc"]
    assert h in abi.all_optional_headers()
    syms = header_symbols(h.header)
    assert h.header == "gjx_csmc.h" and syms == set(h.prototypes) == SYMBOLS and h.version_fn in syms
    assert h.unavailable is abi.CsmcUnavailable and h.version == abi.CSMC_ABI_VERSION == (0, 1)
    assert not (syms & header_symbols("gjx.h")) and not (syms & set(abi.PROTOTYPES))
    for other in abi.all_optional_headers():
        if other is not h:
            assert not (syms & header_symbols(other.header)) and not (syms & set(other.prototypes))
    for name in syms:
        assert hasattr(ops.lib._dll, name) and not hasattr(oracle_ops.lib._dll, name), name
    assert ops.lib.has_csmc and not oracle_ops.lib.has_csmc
    major, minor = C.c_int(-1), C.c_int(-1)
    ops.lib.call("gjx_csmc_version", C.byref(major), C.byref(minor))
    hdr = open(os.path.join(ROOT, "include", h.header)).read()
    assert f"GJX_CSMC_VERSION_MAJOR {major.value}" in hdr and f"GJX_CSMC_VERSION_MINOR {minor.value}" in hdr
    # the tables the earlier headers' suites pin are as they were
    assert list(abi.OPTIONAL_HEADERS) == ["paths", "guided", "backsim"] and list(abi.EXTENSION_HEADERS) == ["backmove"]


def test_the_oracle_says_the_header_is_missing(oracle_ops):
    y, _, _ = R.lgssm_truth(4)
    smc = BootstrapSMC(StateSpaceModel(*B.lgssm_model()), Cm["y"].set(torch.tensor(y)), 8, record_history=True)
    with use_ops(oracle_ops):
        with pytest.raises(abi.CsmcUnavailable, match="gjx_smc_plan_step_conditional") as e:
            smc.run(genjax.random.key(1), retained=torch.zeros(4))
    assert e.value.code == UNSUPPORTED and isinstance(e.value, GjxError)


# ---- lowering and refusals ---------------------------------------------------------------------------------------------
def _obs(T=4):
    return Cm["y"].set(torch.tensor(R.lgssm_truth(T)[0]))


def _nested_model():
    @gen
    def inner(m):
        return normal(m, 1.0) @ "x"

    @gen
    def init():
        x = inner(0.0) @ "sub"
        normal(x, 0.5) @ "y"
        return x

    @gen
    def step(x):
        x2 = inner(0.9 * x) @ "sub"
        normal(x2, 0.5) @ "y"
        return x2

    return StateSpaceModel(init, step)


def _spare_latent_model():
    """A latent site ("e") that is not returned in the carry."""

    @gen
    def init():
        x = normal(0.0, 1.0) @ "x"
        normal(x, 0.5) @ "y"
        return x

    @gen
    def step(x):
        e = normal(0.0, 0.3) @ "e"
        x2 = normal(0.9 * x + e, 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    return StateSpaceModel(init, step)


def test_the_model_condition(ops):
    def refuse(model, match, n_state=1):
        smc = BootstrapSMC(model, _obs(), 8, record_history=True)
        with use_ops(ops):
            with pytest.raises(PlanUnsupported, match=match):
                smc.run(genjax.random.key(0), retained=tuple(torch.zeros(4) for _ in range(n_state)) if n_state > 1 else torch.zeros(4))

    refuse(_spare_latent_model(), "latent site 0 of `step` is not returned in the carry")
    refuse(StateSpaceModel(*B.track_model()), "carry component 0 of `step` is not one of the body's sampled sites", 2)
    refuse(_nested_model(), "nested `@gen` calls")
    # an unpaired latent of a guided model is fine as long as it is carried (guided_ref.mixed_model) ...
    mi, ms, mtq = G.mixed_model()
    with use_ops(ops):
        check_conditional(build_guided_plan(StateSpaceModel(mi, ms), Y, mtq)[0])
        check_conditional(build_smc_plan(StateSpaceModel(*B.two_component_model()), Y)[0])

    # ... and not when it is left out of the carry
    @gen
    def init_x():
        x = normal(0.0, 1.0) @ "x"
        z = normal(0.0, 0.3) @ "z"
        normal(x + z, 0.2) @ "y"
        return x

    @gen
    def step_x(x):
        z2 = normal(0.0, 0.3) @ "z"
        x2 = normal(0.9 * x, 1.0) @ "x"
        normal(x2 + z2, 0.2) @ "y"
        return x2

    @gen
    def tq(x, y):
        normal(0.3 * x + 0.7 * y, 0.25) @ "x"

    smc = GuidedSMC(StateSpaceModel(init_x, step_x), _obs(), 8, step_proposal=tq, record_history=True)
    with use_ops(ops):
        with pytest.raises(PlanUnsupported, match="latent site 1 of `init` is not returned in the carry"):
            smc.run(genjax.random.key(0), retained=torch.zeros(4))


def test_what_run_refuses(ops):
    model, obs, key, path = StateSpaceModel(*B.lgssm_model()), _obs(), genjax.random.key(0), torch.zeros(4)
    with use_ops(ops):
        with pytest.raises(ValueError, match="ess_threshold must be 0"):
            BootstrapSMC(model, obs, 8, record_history=True, ess_threshold=0.5).run(key, retained=path)
        with pytest.raises(ValueError, match="record_history=True"):
            BootstrapSMC(model, obs, 8).run(key, retained=path)
        y = R.lgssm_truth(4)[0]
        with pytest.raises(ValueError, match="LinearGaussianSSM is a fixed model: write it as a StateSpaceModel"):
            BootstrapSMC(LinearGaussianSSM(), y, 8, record_history=True).run(key, retained=path)
        hmm = DiscreteHMM(torch.zeros(3, 3), torch.zeros(3, 3))
        with pytest.raises(ValueError, match="DiscreteHMM is a fixed model: write it as a StateSpaceModel"):
            BootstrapSMC(hmm, np.zeros(4, dtype=np.int32), 8, record_history=True).run(key, retained=path)
        with pytest.raises(ValueError, match="run_many.*one at a time"):
            BootstrapSMC(model, obs, 8, record_history=True).run_many([key, key], retained=path)
        smc = BootstrapSMC(model, obs, 8, record_history=True)
        with pytest.raises(ValueError, match=r"T = 4 values.*got shape \(5,\)"):
            smc.run(key, retained=torch.zeros(5))
        with pytest.raises(ValueError, match=r"got shape \(2, 2\)"):
            smc.run(key, retained=torch.zeros(2, 2))
        with pytest.raises(ValueError, match="1 component.*got 2 path column"):
            smc.run(key, retained=(path, path))
        with pytest.raises(ValueError, match="at least 2 particles"):
            BootstrapSMC(model, obs, 1, record_history=True).run(key, retained=path)


def test_what_particle_gibbs_refuses():
    model, obs = StateSpaceModel(*B.lgssm_model()), _obs()
    with pytest.raises(ValueError, match="record_history=True"):
        ParticleGibbs(BootstrapSMC(model, obs, 8))
    with pytest.raises(ValueError, match="'trace' or 'backward'"):
        ParticleGibbs(BootstrapSMC(model, obs, 8, record_history=True), refresh="forward")
    with pytest.raises(ValueError, match="ess_threshold must be 0"):
        ParticleGibbs(BootstrapSMC(model, obs, 8, record_history=True, ess_threshold=0.5))
    with pytest.raises(TypeError, match="write it as a StateSpaceModel"):
        ParticleGibbs(BootstrapSMC(LinearGaussianSSM(), R.lgssm_truth(4)[0], 8, record_history=True))
    par = BootstrapSMC(SP.lgssm_param_model(), obs, 8, record_history=True, params=(0.9, 1.0, 0.5))
    with pytest.raises(PlanUnsupported, match="refresh='backward'.*parameters.*use refresh='trace'"):
        ParticleGibbs(par, refresh="backward")
    ParticleGibbs(par, refresh="trace", param_update=lambda key, path, theta: theta)
    with pytest.raises(ValueError, match="declares parameters"):
        ParticleGibbs(BootstrapSMC(model, obs, 8, record_history=True), param_update=lambda key, path, theta: theta)


# ---- source and compile --------------------------------------------------------------------------------------------------
def _plans(ops):
    tq, sq, _ = G.lgssm_optimal(0.05)
    ti, ts, ttq, tsq = G.two_latent_model()
    gi, gs, gtq, gsq = G.gamma_scale_model()
    mi, ms, mtq = G.mixed_model()
    with use_ops(ops):
        return dict(lgssm=build_smc_plan(StateSpaceModel(*B.lgssm_model()), Y)[0],
                    lgssm_guided=build_guided_plan(StateSpaceModel(*G.lgssm_model(0.05)), Y, tq, sq)[0],
                    two_latent=build_guided_plan(StateSpaceModel(ti, ts), Y, ttq, tsq)[0],
                    gamma=build_guided_plan(StateSpaceModel(gi, gs), Y, gtq, gsq)[0],
                    mixed=build_guided_plan(StateSpaceModel(mi, ms), Y, mtq)[0],
                    lgssm_params=build_smc_plan(SP.lgssm_param_model(), Y, (0.9, 1.0, 0.5))[0])


@pytest.mark.parametrize("impl", [0, 1])
def test_the_unconditional_source_is_untouched_and_the_conditional_one_compiles(ops, impl):
    for name, plan in _plans(ops).items():
        before = plan.source(impl)
        cond = plan.csmc_source(impl)
        assert plan.source(impl) == before, name  # (asking for the conditional source first changes nothing)
        assert "conditional" not in before and "CsmcRet" not in before and "rsel" not in before, name
        assert "gjx_smc_step_kernel_conditional" in cond and "gjx_smc_init_kernel_conditional" in cond, name
        assert 'void gjx_smc_step_kernel(' not in cond and "gjx_smc_step_kernel_adaptive" not in cond, name
        assert "resample_body<" + str(impl) + ", GenPolicy, false, false, true>" in cond, name
        # the override is a select after the draw, one per sampled site and slot of the walk
        assert cond.count(" = rsel") >= 2 and "if (rsel" in cond, name
        assert plan.csmc_compile_check(impl) == 0, name
        assert plan.compile_check(impl) == 0, name
    # the policy of the conditional source is GenPolicy plus the selects: dropping them gives the unconditional lines
    plan = _plans(ops)["lgssm"]
    a, b = plan.source(impl), plan.csmc_source(impl)
    assert a.count("std_normal(") + a.count("bm_pair(") > 0
    assert b.count("philox4x32(") == a.count("philox4x32(") and b.count("Stream<0>(") == a.count("Stream<0>(")  # no draw renumbered


@pytest.mark.parametrize("impl", [0, 1])
def test_conditional_kernels_have_no_scratch(ops, tmp_path, impl):
    """Register counts of the kernels of both generators, conditional next to unconditional (figures: profiles/csmc_summary.md)."""
    plans = _plans(ops)
    for name in ("lgssm", "lgssm_guided", "lgssm_params"):
        cond = kernel_notes(plans[name].csmc_source(impl), tmp_path, name + "_cond")
        plain = kernel_notes(plans[name].source(impl), tmp_path, name + "_plain")
        for k in ("gjx_smc_step_kernel", "gjx_smc_init_kernel"):
            print(f"{name} impl {impl} {k}: unconditional {plain[k]}  conditional {cond[k + '_conditional']}")
            assert cond[k + "_conditional"]["private_segment_fixed_size"] == 0
            assert plain[k]["private_segment_fixed_size"] == 0
        assert set(cond) == {"gjx_smc_step_kernel_conditional", "gjx_smc_init_kernel_conditional"}


# ---- the C entry points' refusals --------------------------------------------------------------------------------------------
def _call_step(ops, plan, cfg, t=0, path=None, n_state=1):
    keep = np.zeros(8, dtype=np.float32)
    p = abi.CsmcPath()
    for k in range(n_state):
        p.path[k] = keep.ctypes.data  # (never read: every call below is refused before a launch)
    out = abi.SmcPop()
    return ops.lib._gjx_smc_plan_step_conditional(C.byref(cfg), plan.handle, t, keep.ctypes.data_as(C.c_void_p), None, C.byref(out),
                                                  None, None, None, C.byref(p) if path is None else path, None)


def test_the_c_entry_points_refuse(ops, monkeypatch):
    plans = _plans(ops)
    plan = plans["lgssm"]
    sk = np.zeros((2, 2), dtype=np.uint32)
    good = lambda: ops.smc_config(1, 2048, 0, 2048, sk, sk)  # noqa: E731
    # GJX_ERR_INVALID
    assert _call_step(ops, plan, ops.smc_config(1, 1, 0, 1, sk, sk)) == INVALID  # n_total < 2
    assert _call_step(ops, plan, good(), n_state=0) == INVALID  # a NULL path component
    assert ops.lib._gjx_smc_plan_step_conditional(C.byref(good()), plan.handle, 0, None, None, C.byref(abi.SmcPop()), None, None, None,
                                                  None, None) == INVALID  # no path at all
    with use_ops(ops):
        track = build_smc_plan(StateSpaceModel(*B.track_model()), Y)[0]
        spare = build_smc_plan(_spare_latent_model(), Y)[0]
        nested = build_smc_plan(_nested_model(), Y)[0]
    assert _call_step(ops, track, good(), n_state=2) == INVALID  # the model condition: a carry expression
    assert _call_step(ops, spare, good()) == INVALID  # ... a latent site outside the carry
    for bad in (track, spare):
        assert ops.lib._gjx_csmc_plan_compile_check(bad.handle, 1) == INVALID
        assert ops.lib._gjx_csmc_plan_source(bad.handle, 1, None, 0, None) == INVALID
    assert ops.lib._gjx_csmc_plan_compile_check(plan.handle, 2) == INVALID
    # GJX_ERR_UNSUPPORTED
    assert _call_step(ops, nested, good()) == UNSUPPORTED  # scopes
    assert ops.lib._gjx_csmc_plan_compile_check(nested.handle, 1) == UNSUPPORTED
    cfg = good()
    cfg.ess_threshold = 0.5
    assert _call_step(ops, plan, cfg) == UNSUPPORTED
    cfg = good()
    cfg.n_filters = 2
    assert _call_step(ops, plan, cfg) == UNSUPPORTED
    assert _call_step(ops, plan, ops.smc_config(1, 2048, 1024, 1024, sk, sk)) == UNSUPPORTED  # a shard
    assert _call_step(ops, plan, ops.smc_config(1, 2048, 0, 1024, sk, sk)) == UNSUPPORTED
    cfg = good()
    peers = abi.SmcPeers()
    cfg.peers = C.pointer(peers)
    assert _call_step(ops, plan, cfg) == UNSUPPORTED
    monkeypatch.setenv("GJX_PLAN_JIT", "0")
    assert _call_step(ops, plan, good()) == UNSUPPORTED
