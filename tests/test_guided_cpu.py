"""Guided particle filters without a GPU: the lowering of `GuidedSMC` (one site table per body, the proposal's sites in
front), what it refuses, include/gjx_guided.h as a third header (libgjx_hip.so exports it, the oracle does not), the
creators' validation, and the generated kernels compiled for gfx950 offline (libgjx_hip.so loaded without a device, as
test_plan_specialization.py does)."""

import ctypes as C
import re

import pytest
import torch

import genjax
import guided_ref as G
from genjax import ChoiceMapBuilder as Cm, flip, gen, normal
from genjax._amd import abi
from genjax._amd.abi import GjxError
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax._amd.smc_plan import build_guided_plan, build_smc_plan
from genjax.inference.smc import GuidedSMC, StateSpaceModel
from offline import kernel_notes, ops  # noqa: F401

R = 0.05
Y = [("y",)]


def _lgssm_guided(ops, with_init=True):
    init, step = G.lgssm_model(R)
    tq, sq, _ = G.lgssm_optimal(R)
    with use_ops(ops):
        return build_guided_plan(StateSpaceModel(init, step), Y, tq, sq if with_init else None)[0]


# ---- the header (that it is exported by the HIP library only: test_paths_abi.py, with the other optional headers) ---------
def test_oracle_bound_ops_refuse_guided_filters(oracle_ops):
    init, step = G.lgssm_model(R)
    tq, sq, _ = G.lgssm_optimal(R)
    y, _ = G.lgssm_setting(R, 5)
    alg = GuidedSMC(StateSpaceModel(init, step), Cm["y"].set(torch.tensor(y)), 256, step_proposal=tq, init_proposal=sq)
    with use_ops(oracle_ops):
        with pytest.raises(abi.GuidedUnavailable, match="gjx_smc_plan_create_guided") as e:
            alg.run(genjax.random.key(1))
    assert isinstance(e.value, GjxError) and e.value.code == -2
    with pytest.raises(abi.GuidedUnavailable):  # ... and the low-level route hands the oracle no table it would misread
        oracle_ops.smc_plan_create([], [], [], [], 0, guided=True)
    with pytest.raises(abi.GuidedUnavailable, match="gjx_smc_plan_source"):
        oracle_ops.lib.call("gjx_smc_plan_source", None, 0, None, 0, None)


# ---- lowering ----------------------------------------------------------------------------------------------------------
def test_lowering_of_a_one_latent_model(ops):
    plan = _lgssm_guided(ops)
    for table, state in zip(plan._tables, plan._state_args):
        assert G.modes(table) == [abi.SITE_PROPOSED, abi.SITE_GUIDED, 1]  # the proposal's site first, then the model body
        q, x, y = table
        assert (x.obs.kind, x.obs.ref, x.obs.scale, x.obs.offset) == (abi.ARG_SITE, 0, 1.0, 0.0)
        assert (y.obs.kind, y.obs.ref) == (abi.ARG_OBS, 0)
        # the value the model body sees is the PARTNER's: the observed site's location and the carry read site 0
        assert (y.arg[0].kind, y.arg[0].ref) == (abi.ARG_SITE, 0) and (state[0].kind, state[0].ref) == (abi.ARG_SITE, 0)
        assert all(s.out_col == -1 for s in table)
    step = plan._tables[1]
    assert step[0].arg[0].kind == abi.ARG_EXPR  # c1 * carry + c2 * y: a program over the carry and the observation
    assert (step[1].arg[0].kind, step[1].arg[0].ref) == (abi.ARG_STATE, 0)
    # without an init proposal step 0 is the bootstrap step 0
    boot_init = _lgssm_guided(ops, with_init=False)._tables[0]
    assert G.modes(boot_init) == [0, 1]


def test_lowering_of_a_two_latent_model_with_a_two_component_carry(ops):
    init, step, tq, sq = G.two_latent_model()
    with use_ops(ops):
        plan, n_state = build_guided_plan(StateSpaceModel(init, step), Y, tq, sq)
    assert n_state == 2
    ti, ts = plan._tables
    P, Gd = abi.SITE_PROPOSED, abi.SITE_GUIDED
    assert G.modes(ti) == [P, P, Gd, Gd, 1] and G.modes(ts) == [P, P, Gd, Gd, 1]
    # init: proposal (p, v), model (p, v); step: proposal (v, p), model (v, p) — partners by ADDRESS
    assert [s.obs.ref for s in ti[2:4]] == [0, 1] and [s.obs.ref for s in ts[2:4]] == [0, 1]
    # the model's `p + 0.5 * v2` reads the proposed v (site 0), the observation reads the proposed p (site 1)
    assert (ts[4].arg[0].kind, ts[4].arg[0].ref) == (abi.ARG_SITE, 1)
    init_state, next_state = plan._state_args
    assert [(a.kind, a.ref) for a in init_state] == [(abi.ARG_SITE, 0), (abi.ARG_SITE, 1)]
    assert [(a.kind, a.ref) for a in next_state] == [(abi.ARG_SITE, 1), (abi.ARG_SITE, 0)]  # (p2, v2)
    # one guided, one prior-drawn latent: the unpaired site stays latent, at its own position in the model body
    init, step, tq = G.mixed_model()
    with use_ops(ops):
        plan, _ = build_guided_plan(StateSpaceModel(init, step), Y, tq)
    assert G.modes(plan._tables[0]) == [0, 0, 1] and G.modes(plan._tables[1]) == [P, 0, Gd, 1]
    assert plan._tables[1][2].obs.ref == 0


def test_observations_reach_a_proposal_as_a_tuple_in_leaf_order(ops):
    @gen
    def init():
        x = normal(0.0, 1.0) @ "x"
        normal(x, 0.5) @ "u"
        normal(x, 0.7) @ "w"
        return x

    @gen
    def step(x):
        x2 = normal(0.9 * x, 1.0) @ "x"
        normal(x2, 0.5) @ "u"
        normal(x2, 0.7) @ "w"
        return x2

    @gen
    def tq(carry, y):
        u, w = y
        normal(0.2 * carry + 0.5 * u + 0.3 * w, 0.4) @ "x"

    with use_ops(ops):
        plan, _ = build_guided_plan(StateSpaceModel(init, step), [("u",), ("w",)], tq)
    prog = C.cast(plan._tables[1][0].arg[0].table, C.POINTER(abi.ExprOp))
    ops_ = [(prog[k].op, prog[k].ref) for k in range(plan._tables[1][0].arg[0].ref)]
    assert [r for o, r in ops_ if o == abi.EXPR_OBS] == [0, 1] and plan.n_obs == 2
    plan.ops.lib.call("gjx_smc_plan_compile_check", plan.handle, 1)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_what_the_lowering_refuses_names_the_address(ops):
    init, step = G.lgssm_model(R)
    model = StateSpaceModel(init, step)

    def refuse(match, tq, sq=None, m=model):
        with use_ops(ops):
            with pytest.raises(PlanUnsupported, match=match):
                build_guided_plan(m, Y, tq, sq)

    @gen
    def no_partner(carry, y):
        normal(carry, 1.0) @ "x"
        normal(0.0, 1.0) @ "ghost"

    refuse("'ghost'.*no partner", no_partner)

    @gen
    def on_observed(carry, y):
        normal(carry, 1.0) @ "x"
        normal(carry, 1.0) @ "y"

    refuse("OBSERVED address 'y'", on_observed)

    @gen
    def int_for_float(carry, y):
        flip(0.5) @ "x"

    refuse("'x'.*integer-valued.*float-valued", int_for_float)

    @gen
    def inner(m):
        return normal(m, 1.0) @ "x"

    @gen
    def nested(carry, y):
        inner(carry) @ "sub"

    refuse("nested `@gen` call at address 'sub' inside a proposal", nested)

    # a partner inside a callee: the model draws ("sub", "x") in a nested call, the proposal names that address
    @gen
    def init_c():
        x = inner(0.0) @ "sub"
        normal(x, R) @ "y"
        return x

    @gen
    def step_c(x):
        x2 = inner(0.9 * x) @ "sub"
        normal(x2, R) @ "y"
        return x2

    @gen
    def into_callee(carry, y):
        normal(carry, 1.0) @ ("sub", "x")

    refuse(r"\('sub', 'x'\).*inside the callee at 'sub'", into_callee, m=StateSpaceModel(init, step_c))
    # (a callee in a body that has no proposal of its own is refused as well: guided plans have flat bodies)
    refuse("nested `@gen` call at address 'sub' in a body of a guided model", into_callee, m=StateSpaceModel(init_c, step_c))
    # the init proposal is held to the same rules
    tq, _, _ = G.lgssm_optimal(R)

    @gen
    def init_ghost(y):
        normal(0.0, 1.0) @ "nowhere"

    refuse("init proposal's site 'nowhere'", tq, init_ghost)


# ---- the creators ------------------------------------------------------------------------------------------------------
def _site(dist, a0, a1=None, observed=0, obs=None):
    s = abi.Site()
    s.dist, s.observed, s.out_col = dist, observed, -1
    s.arg[0] = a0
    if a1 is not None:
        s.arg[1] = a1
    if obs is not None:
        s.obs = obs
    return s


def _c(v):
    return abi.Arg(abi.ARG_CONST, 0, 0.0, v, None)


def _ref(k, scale=1.0, offset=0.0):
    return abi.Arg(abi.ARG_SITE, k, scale, offset, None)


def test_old_creators_reject_the_new_modes(ops):
    N = abi.DIST_NORMAL
    for mode in (abi.SITE_PROPOSED, abi.SITE_GUIDED, 4):
        odd = [_site(N, _c(0.0), _c(1.0)), _site(N, _c(0.0), _c(1.0), observed=mode, obs=_ref(0) if mode == 3 else _c(0.5))]
        with pytest.raises(GjxError, match="GJX_ERR_INVALID"):
            ops.plan_create(odd)
        with pytest.raises(GjxError, match="gjx_plan_create_scoped.*GJX_ERR_INVALID"):
            ops.plan_create(odd, scopes=[(0, 1, 2)])
        ok = [_site(N, _c(0.0), _c(1.0))]
        for init, step in ((odd, ok), (ok, odd)):
            with pytest.raises(GjxError, match="gjx_smc_plan_create failed: GJX_ERR_INVALID"):
                ops.smc_plan_create(init, step, [_ref(0)], [_ref(0)], 0)
            with pytest.raises(GjxError, match="gjx_smc_plan_create_scoped.*GJX_ERR_INVALID"):
                ops.smc_plan_create(init, step, [_ref(0)], [_ref(0)], 0, init_scopes=[(0, 0, 1)])
        with pytest.raises(GjxError, match="gjx_scan_plan_create failed: GJX_ERR_INVALID"):
            ops.scan_plan_create(odd, [_ref(0)], 0)
        with pytest.raises(GjxError, match="gjx_scan_plan_create_scoped.*GJX_ERR_INVALID"):
            ops.scan_plan_create(odd, [_ref(0)], 0, scopes=[(0, 0, 1)])
    # (what they accepted before they still accept)
    ops.smc_plan_create(ok, [ok[0], _site(N, _ref(0), _c(1.0), observed=1, obs=_c(0.5))], [_ref(0)], [_ref(0)], 0)


def test_guided_creator_validates_the_pairing(ops):
    N, B = abi.DIST_NORMAL, abi.DIST_BERNOULLI
    P, Gd = abi.SITE_PROPOSED, abi.SITE_GUIDED
    plain = [_site(N, _c(0.0), _c(1.0))]
    q = _site(N, _c(0.0), _c(2.0), observed=P)
    x = _site(N, _c(0.0), _c(1.0), observed=Gd, obs=_ref(0))

    def create(step):
        return ops.smc_plan_create(plain, step, [_ref(0)], [_ref(0)], 0, guided=True)

    create([q, x])  # a valid pair
    create(plain)   # ... and a table without the new modes is a bootstrap plan
    bad = {
        "a proposed site nobody refers to": [q, plain[0]],
        "two guided sites on one proposal": [q, x, x],
        "a guided site that refers to a latent site": [plain[0], x],
        "a guided site that refers to itself / a later site": [q, _site(N, _c(0.0), _c(1.0), observed=Gd, obs=_ref(1))],
        "a scaled reference": [q, _site(N, _c(0.0), _c(1.0), observed=Gd, obs=_ref(0, 2.0))],
        "a shifted reference": [q, _site(N, _c(0.0), _c(1.0), observed=Gd, obs=_ref(0, 1.0, 0.5))],
        "a reference that is not a site": [q, _site(N, _c(0.0), _c(1.0), observed=Gd, obs=_c(0.0))],
        "an integer-valued proposal for a float-valued site": [_site(B, _c(0.5), observed=P), x],
        "a mode beyond 3": [q, x, _site(N, _c(0.0), _c(1.0), observed=4, obs=_c(0.0))],
    }
    for what, step in bad.items():
        with pytest.raises(GjxError, match="gjx_smc_plan_create_guided failed: GJX_ERR_INVALID"):
            create(step)
            pytest.fail(what)


def test_table_walking_policy_refuses_guided_plans(ops, monkeypatch):
    """GJX_PLAN_JIT=0 selects the table-walking policy, which knows neither mode: refused before anything is launched."""
    plan = _lgssm_guided(ops)
    monkeypatch.setenv("GJX_PLAN_JIT", "0")
    import numpy as np

    sk = np.zeros((2, 2), dtype=np.uint32)
    cfg = ops.smc_config(1, 1024, 0, 1024, sk, sk)
    out = abi.SmcPop()
    rc = ops.lib._gjx_smc_plan_step(C.byref(cfg), plan.handle, 0, np.zeros(1, dtype=np.float32).ctypes.data_as(C.c_void_p), None,
                                    C.byref(out), None, None, None, None)
    assert rc == -2  # GJX_ERR_UNSUPPORTED


# ---- the generated kernels -----------------------------------------------------------------------------------------------
def _plans(ops):
    init, step = G.lgssm_model(R)
    tq, sq, _ = G.lgssm_optimal(R)
    gi, gs, gtq, gsq = G.gamma_scale_model()
    mi, ms, mtq = G.mixed_model()
    with use_ops(ops):
        return dict(lgssm=build_guided_plan(StateSpaceModel(init, step), Y, tq, sq)[0],
                    gamma=build_guided_plan(StateSpaceModel(gi, gs), Y, gtq, gsq)[0],
                    mixed=build_guided_plan(StateSpaceModel(mi, ms), Y, mtq)[0])


@pytest.mark.parametrize("impl", [0, 1])
def test_guided_plans_compile_for_both_generators(ops, impl):
    for name, plan in _plans(ops).items():
        assert plan.compile_check(impl) == 0, name
        src = plan.source(impl)
        assert "proposed" in src and "guided" in src and src.count("lp - lq") >= 1
    src = _plans(ops)["lgssm"].source(impl)
    step = src.split("struct GenPolicy")[1].split("extern \"C\"")[0]
    # per slot: one kept log-density per proposed site, one `lp - lq` per guided site; the quad form four of each
    per_slot = step.split("compute_quad")[0] if impl == 1 else step
    assert per_slot.count("const float lq0 = ") == 1 and per_slot.count("const float d = lp - lq0;") == 1
    if impl == 1:
        quad = step.split("compute_quad")[1]
        assert quad.count("const float d = lp - lq0") == 4 and len(re.findall(r"const float lq0[A-D] = ", quad)) == 4
        # the proposal's one-word draw is draw 0 of the quad's block, computed in prefetch() under the step's first loads
        pf = step.split("void prefetch")[1].split("compute_quad")[0]
        assert pf.count("philox4x32(") == 1 and ", 0u, kTagQuad" in pf and pf.count("bm_pair(") == 2
        assert "philox4x32(" not in quad  # (nothing is drawn twice: the guided site draws nothing)


def test_guided_step_kernel_has_no_scratch(ops, tmp_path):
    """The PHILOX step kernel of the guided LGSSM (quad form: lq of four slots lives from the proposal to its partner)
    against the bootstrap plan of the same model; figures in profiles/guided_summary.md."""
    init, step = G.lgssm_model(R)
    with use_ops(ops):
        boot = build_smc_plan(StateSpaceModel(init, step), Y)[0]
    guided = kernel_notes(_plans(ops)["lgssm"].source(1), tmp_path, "guided")
    plain = kernel_notes(boot.source(1), tmp_path, "bootstrap")
    for k in ("gjx_smc_step_kernel", "gjx_smc_step_kernel_adaptive", "gjx_smc_init_kernel"):
        print(f"{k}: guided {guided[k]}  bootstrap {plain[k]}")
    assert guided["gjx_smc_step_kernel"]["private_segment_fixed_size"] == 0
    assert guided["gjx_smc_step_kernel_adaptive"]["private_segment_fixed_size"] == 0
    assert guided["gjx_smc_init_kernel"]["private_segment_fixed_size"] == 0
