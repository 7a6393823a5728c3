"""Backward-simulation smoothing without a GPU: the lowering of a model's transition to a site table and what it refuses,
include/gjx_backsim.h as a fourth header (libgjx_hip.so exports it, the oracle does not), the creators' validation, the
generated kernels compiled for gfx950 offline (libgjx_hip.so loaded without a device), and the reference of
tests/backsim_ref.py held against exact smoothers."""

import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import torch

import backsim_ref as B
import genjax
from genjax import ChoiceMapBuilder as Cm, gen, normal
from genjax._amd import abi, workloads as W
from genjax._amd.abi import GjxError
from genjax._amd.plan import PlanUnsupported
from genjax._amd.runtime import use_ops
from genjax._amd.smc_models import HmmFilter, LgssmFilter
from genjax._amd.smc_plan import build_smc_plan, build_transition_table
from genjax.inference.smc import BootstrapSMC, DiscreteHMM, LinearGaussianSSM, StateSpaceModel
from offline import kernel_notes, llvm_tool, ops, source_shape  # noqa: F401

Y = [("y",)]


def _table(ops, model, addrs=Y):
    with use_ops(ops):
        return build_transition_table(StateSpaceModel(*model), addrs)


# ---- the header (that it is exported by the HIP library only: test_paths_abi.py, with the other optional headers) ---------
def test_oracle_bound_ops_raise_unavailable(oracle_ops):
    y = W.lgssm_data(6)
    alg = BootstrapSMC(LinearGaussianSSM(), y, 512, record_history=True)
    with use_ops(oracle_ops):
        res = alg.run(genjax.random.key(1, "philox"))
        with pytest.raises(abi.BacksimUnavailable, match="gjx_backsim") as e:
            alg.backward_simulate(res, genjax.random.key(2, "philox"), n_paths=8)
    assert isinstance(e.value, GjxError) and e.value.code == -2
    with pytest.raises(abi.BacksimUnavailable):
        oracle_ops.backsim_plan_create(_table(oracle_ops, B.lgssm_model()))
    with pytest.raises(abi.BacksimUnavailable, match="gjx_backsim_run"):
        oracle_ops.lib.call("gjx_backsim_run", None, None, None, 0, None)


def test_a_result_without_history_raises(oracle_ops):
    alg = BootstrapSMC(LinearGaussianSSM(), W.lgssm_data(4), 256)
    with use_ops(oracle_ops):
        res = alg.run(genjax.random.key(1))
        with pytest.raises(ValueError, match="record_history"):
            alg.backward_simulate(res, genjax.random.key(2), n_paths=4)


# ---- lowering ----------------------------------------------------------------------------------------------------------
def test_lowering_of_a_one_component_normal_carry(ops):
    t = _table(ops, B.lgssm_model())
    assert (t.n_state, t.n_obs, len(t.sites)) == (1, 1, 1)  # "y" reads the new state alone: constant in i, dropped
    (x,) = t.sites
    assert B.site_fields(x) == (abi.DIST_NORMAL, 1, -1, 0, 0, 0, (abi.ARG_STATE, 0, pytest.approx(B.A), 0.0),
                                (abi.ARG_CONST, 0, 0.0, B.Q), (abi.ARG_NEXT, 0, 1.0, 0.0))


def test_lowering_of_a_two_component_carry(ops):
    t = _table(ops, B.two_component_model())
    assert (t.n_state, len(t.sites)) == (2, 2)
    v, p = t.sites
    # `return p2, v2`: v2 (site 0) is component 1, p2 (site 1) component 0
    assert B.arg_fields(v.obs) == (abi.ARG_NEXT, 1, 1.0, 0.0) and B.arg_fields(p.obs) == (abi.ARG_NEXT, 0, 1.0, 0.0)
    assert v.observed == p.observed == 1
    # `p + 0.5 * v2` reads the old state AND the first site (whose value is now the next state's component 1)
    assert p.arg[0].kind == abi.ARG_EXPR
    prog = [(o.op, o.ref) for o in (abi.ExprOp * p.arg[0].ref).from_address(p.arg[0].table)]
    assert (abi.EXPR_STATE, 0) in prog and (abi.EXPR_SITE, 0) in prog


def test_lowering_of_a_gamma_carry(ops):
    t = _table(ops, B.gamma_model())
    (g,) = t.sites
    assert g.dist == abi.DIST_GAMMA and g.observed == 1 and B.arg_fields(g.obs) == (abi.ARG_NEXT, 0, 1.0, 0.0)
    assert B.arg_fields(g.arg[0])[0] == abi.ARG_CONST and g.arg[1].kind == abi.ARG_EXPR  # 4.0 / g: a program over the state


def test_lowering_of_a_user_hmm(oracle_ops):
    trans, emit = B.hmm_tables(8)
    t = _table(oracle_ops, B.hmm_model(trans, emit), [("x",)])  # (lowered under the oracle's ops: its tables are CPU tensors)
    (z,) = t.sites  # the emission reads the new state alone: dropped
    assert B.site_fields(z) == (abi.DIST_CATEGORICAL, 1, -1, 8, 8, 0, (abi.ARG_STATE, 0, 1.0, 0.0), None, (abi.ARG_NEXT, 0, 1.0, 0.0))
    kept = [k for k in t.keep if isinstance(k, torch.Tensor) and k.data_ptr() == z.logits]
    assert len(kept) == 1 and torch.equal(kept[0], trans)


def test_an_observed_site_that_reads_the_old_state_is_kept(ops):
    t = _table(ops, B.increment_model(), [("u",), ("d",)])
    assert (t.n_state, t.n_obs, len(t.sites)) == (2, 2, 3)  # "u" dropped; v, p, d kept
    v, p, d = t.sites
    assert B.arg_fields(v.obs) == (abi.ARG_NEXT, 1, 1.0, 0.0) and B.arg_fields(p.obs) == (abi.ARG_NEXT, 0, 1.0, 0.0)
    assert B.arg_fields(d.obs) == (abi.ARG_OBS, 1, 1.0, 0.0)  # the observation COLUMN keeps its number
    progs = [[(o.op, o.ref) for o in (abi.ExprOp * s.arg[0].ref).from_address(s.arg[0].table)] for s in (p, d)]
    # site references moved with the shortened table: v2 was site 1 and is site 0, p2 was site 2 and is site 1
    assert (abi.EXPR_SITE, 0) in progs[0] and (abi.EXPR_SITE, 1) in progs[1] and (abi.EXPR_STATE, 0) in progs[1]
    ops.backsim_plan_create(t)  # ... and the creator accepts the renumbered table


def test_the_fixed_kinds_tables_equal_their_user_written_equivalents(oracle_ops):
    mdl = LinearGaussianSSM()
    fixed, obs = LgssmFilter(oracle_ops, abi.Lgssm(mdl.x0_loc, mdl.x0_scale, mdl.a, mdl.q, mdl.r), W.lgssm_data(4)).transition_table()
    user = _table(oracle_ops, B.lgssm_model())
    assert obs is None and (fixed.n_state, fixed.n_obs) == (1, 0)
    assert [B.site_fields(s) for s in fixed.sites] == [B.site_fields(s) for s in user.sites]
    trans, emit = B.hmm_tables(8)
    fixed, obs = HmmFilter(oracle_ops, 8, 0, trans.contiguous(), emit.contiguous(), [0, 1, 2]).transition_table()
    user = _table(oracle_ops, B.hmm_model(trans, emit), [("x",)])
    assert obs is None and [B.site_fields(s) for s in fixed.sites] == [B.site_fields(s) for s in user.sites]
    assert fixed.sites[0].logits == trans.data_ptr()


def test_the_transition_plan_is_built_once_per_filter_object(oracle_ops):
    alg = BootstrapSMC(LinearGaussianSSM(), W.lgssm_data(4), 64, record_history=True)
    assert alg._transition is None  # (filled by the first backward_simulate, like _plan by the first run)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_a_carry_expression_is_refused_as_degenerate(ops):
    with pytest.raises(PlanUnsupported, match=r"carry component 0 .*degenerate"):
        _table(ops, B.track_model())


def test_a_latent_that_is_not_returned_is_refused(ops):
    @gen
    def init():
        x = normal(0.0, 1.0) @ "x"
        normal(x, 0.5) @ "y"
        return x

    @gen
    def step(x):
        e = normal(0.0, 1.0) @ "noise"
        x2 = normal(0.9 * x + e, 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2

    with pytest.raises(PlanUnsupported, match=r"'noise' is not returned"):
        _table(ops, (init, step))


def test_a_latent_returned_twice_is_refused(ops):
    @gen
    def init():
        x = normal(0.0, 1.0) @ "x"
        normal(x, 0.5) @ "y"
        return x, x

    @gen
    def step(c):
        x2 = normal(0.9 * c[0], 1.0) @ "x"
        normal(x2, 0.5) @ "y"
        return x2, x2

    with pytest.raises(PlanUnsupported, match=r"'x' is returned twice"):
        _table(ops, (init, step))


def test_a_nested_call_is_refused(ops):
    @gen
    def inner(x):
        return normal(0.9 * x, 1.0) @ "x"

    @gen
    def init():
        x = normal(0.0, 1.0) @ "x"
        normal(x, 0.5) @ "y"
        return x

    @gen
    def step(x):
        x2 = inner(x) @ "sub"
        normal(x2, 0.5) @ "y"
        return x2

    with pytest.raises(PlanUnsupported, match=r"nested `@gen` call at address 'sub'"):
        _table(ops, (init, step))
    with use_ops(ops):  # (the filter itself runs such a model: only its transition table is refused)
        build_smc_plan(StateSpaceModel(init, step), Y)


# ---- creators ----------------------------------------------------------------------------------------------------------
def _create(ops, sites, n_state=1, n_obs=1, flags=0):
    arr = (abi.Site * max(1, len(sites)))(*sites)
    h = C.c_void_p()
    rc = ops.lib._gjx_backsim_plan_create(arr, len(sites), n_state, n_obs, flags, C.byref(h))
    if rc == 0:
        ops.lib.call("gjx_backsim_plan_destroy", h)
    return rc


def _normal_site(obs, loc=None):
    s = abi.Site()
    s.dist, s.observed, s.out_col = abi.DIST_NORMAL, 1, -1
    s.arg[0] = loc or abi.Arg(abi.ARG_STATE, 0, 0.9, 0.0, None)
    s.arg[1] = abi.Arg(abi.ARG_CONST, 0, 0.0, 1.0, None)
    s.obs = obs
    return s


def test_the_creator_validates_its_table(ops):
    nxt = abi.Arg(abi.ARG_NEXT, 0, 1.0, 0.0, None)
    assert _create(ops, [_normal_site(nxt)]) == 0
    assert _create(ops, [_normal_site(abi.Arg(abi.ARG_OBS, 0, 1.0, 0.0, None))]) == 0
    bad = [
        [_normal_site(abi.Arg(abi.ARG_NEXT, 1, 1.0, 0.0, None))],     # component out of range
        [_normal_site(abi.Arg(abi.ARG_NEXT, -1, 1.0, 0.0, None))],
        [_normal_site(abi.Arg(abi.ARG_NEXT, 0, 2.0, 0.0, None))],     # not a plain reference
        [_normal_site(abi.Arg(abi.ARG_NEXT, 0, 1.0, 0.5, None))],
        [_normal_site(abi.Arg(abi.ARG_OBS, 1, 1.0, 0.0, None))],      # observation column out of range
        [_normal_site(nxt, abi.Arg(abi.ARG_STATE, 1, 1.0, 0.0, None))],  # state component out of range
        [_normal_site(nxt, abi.Arg(abi.ARG_SITE, 0, 1.0, 0.0, None))],   # a site reads itself
        [_normal_site(nxt, abi.Arg(abi.ARG_INPUT, 0, 1.0, 0.0, None))],  # importance-plan kinds
        [_normal_site(nxt, abi.Arg(abi.ARG_PARAM, 0, 1.0, 0.0, None))],
        [_normal_site(nxt, nxt)],                                     # GJX_ARG_NEXT is a VALUE kind, not an argument
        [],
    ]
    for sites in bad:
        assert _create(ops, sites) == -1, [B.site_fields(s) for s in sites]
    for observed in (0, abi.SITE_PROPOSED, abi.SITE_GUIDED, 4):  # every site of a transition table is constrained
        s = _normal_site(nxt)
        s.observed = observed
        assert _create(ops, [s]) == -1, observed
    assert _create(ops, [_normal_site(nxt)], n_state=0) == -1 and _create(ops, [_normal_site(nxt)], n_state=5) == -1
    assert _create(ops, [_normal_site(nxt)], n_obs=-1) == -1 and _create(ops, [_normal_site(nxt)], n_obs=9) == -1
    assert _create(ops, [_normal_site(nxt)], flags=1) == -1
    assert ops.lib._gjx_backsim_plan_create(None, 1, 1, 1, 0, C.byref(C.c_void_p())) == -1


def test_the_creators_of_gjx_h_reject_the_new_kind(ops, oracle_ops):
    nxt = abi.Arg(abi.ARG_NEXT, 0, 1.0, 0.0, None)
    site = _normal_site(nxt)
    latent = _normal_site(nxt)
    latent.observed = 0
    for o in (ops, oracle_ops):
        for bad in (site, _normal_site(abi.Arg(abi.ARG_CONST, 0, 0.0, 0.0, None), loc=nxt)):
            with pytest.raises(GjxError, match="GJX_ERR_INVALID"):
                o.plan_create([bad])
            const = abi.Arg(abi.ARG_CONST, 0, 0.0, 0.0, None)
            with pytest.raises(GjxError, match="GJX_ERR_INVALID"):
                o.smc_plan_create([latent if bad is site else bad], [bad], [const], [const], 1)
            with pytest.raises(GjxError, match="GJX_ERR_INVALID"):
                o.scan_plan_create([bad], [const], 1)
    with pytest.raises(GjxError, match="GJX_ERR_INVALID"):
        ops.smc_plan_create([site], [site], [abi.Arg(abi.ARG_CONST, 0, 0.0, 0.0, None)], [abi.Arg(abi.ARG_CONST, 0, 0.0, 0.0, None)], 1,
                            guided=True)


# ---- offline compilation -----------------------------------------------------------------------------------------------
def inner_loop_instructions(code_object, kernel="gjx_backsim_step_kernel"):
    """Lane-instructions per candidate-trajectory PAIR, counted from the disassembly: the candidate loop is the smallest
    backward branch of the kernel whose body holds the cipher's multiplies; one trip serves 2 candidates x kBacksimBlock
    trajectories.  Every instruction of the body is counted once, the rarely taken special-case blocks of the spec's
    logarithm included: an upper bound on what a trip issues.  -> dict(per_pair, valu, mad_u64 (the cipher's multiplies),
    salu, memory, pairs), or None without llvm-objdump."""
    dump = llvm_tool("llvm-objdump")
    if dump is None:
        return None
    txt = subprocess.run([dump, "-d", "--no-show-raw-insn", code_object], capture_output=True, text=True, timeout=120).stdout
    head = re.search(rf"^([0-9a-f]+) <{kernel}>:$", txt, flags=re.M)
    base = int(head.group(1), 16)
    lines = [ln for ln in txt[head.end():].split("\n\n")[0].splitlines() if re.match(r"\s+\S.*//\s*[0-9A-Fa-f]+:", ln)]
    ins = [re.match(r"\s+(\S.*?)\s*//", ln).group(1) for ln in lines]
    at_addr = {int(re.search(r"//\s*([0-9A-Fa-f]+):", ln).group(1), 16): k for k, ln in enumerate(lines)}
    best = None
    for at, ln in enumerate(lines):
        m = re.search(rf"s_c?branch\w*\s.*<{kernel}\+0x([0-9a-f]+)>", ln)
        lo = at_addr.get(base + int(m.group(1), 16)) if m else None
        if lo is None or lo > at:
            continue
        if sum("v_mad_u64_u32" in t for t in ins[lo:at + 1]) >= 20 and (best is None or at - lo < best[1] - best[0]):
            best = (lo, at)
    if best is None:
        return None
    loop = ins[best[0]:best[1] + 1]
    pairs = 2 * 4  # two candidates per lane x kBacksimBlock trajectories per trip
    valu = [t for t in loop if t.startswith("v_")]
    return dict(per_pair=len(valu) / pairs, valu=len(valu), mad_u64=sum(t.startswith("v_mad_u64_u32") for t in valu),
                salu=sum(t.startswith("s_") for t in loop), memory=sum(t.startswith(("global_", "buffer_", "flat_", "ds_")) for t in loop),
                pairs=pairs)


def test_generated_kernels_compile_offline(ops, oracle_ops, tmp_path):
    trans, emit = B.hmm_tables(8)
    tables = dict(lgssm=_table(ops, B.lgssm_model()), two=_table(ops, B.two_component_model()), gamma=_table(ops, B.gamma_model()),
                  increment=_table(ops, B.increment_model(), [("u",), ("d",)]),
                  # (compile-only: the categorical tables are never read, host tensors will do)
                  hmm=_table(oracle_ops, B.hmm_model(trans, emit), [("x",)]))
    for name, t in tables.items():
        plan = ops.backsim_plan_create(t)
        for impl in (0, 1):
            src = plan.source(impl)
            assert "gjx_backsim_step_kernel" in src and "gjx_backsim_last_kernel" in src and "trans_lp(" in src
            # the generator is baked into the source: both entry points instantiate their body for it, the other's streams are absent
            entries = src.split('extern "C"')[1:]
            assert src.count("nx_") > 0 and len(entries) == 2 and all(f"backsim_body<{impl}," in e for e in entries)
            assert f"Stream<{1 - impl}>" not in src
            assert plan.compile_check(impl) == 0, (name, impl)
    # the lowered distributions are the spec's own device functions
    assert "logpdf_normal_pre(" in ops.backsim_plan_create(tables["lgssm"]).source(1)
    assert "logpdf_gamma(" in ops.backsim_plan_create(tables["gamma"]).source(1)
    assert "jrow_lse(" in ops.backsim_plan_create(tables["hmm"]).source(1)  # (offline: no derived table yet)


def test_generated_source_is_the_table_walk_and_two_instantiations(ops):
    plan = ops.backsim_plan_create(_table(ops, B.lgssm_model()))
    for impl in (0, 1):
        structs, kernels, rest = source_shape(plan.source(impl))
        assert structs == ["GenTrans"] and kernels == ["gjx_backsim_step_kernel", "gjx_backsim_last_kernel"]
        for fixed in ("for (", "while (", "__shared__", "atomic"):  # the fixed body is gjx_device.hpp backsim_body
            assert fixed not in rest, (impl, fixed, rest)
        assert rest.count("\n") == 3, rest  # `using namespace gjx;` and one line per entry point


def test_the_device_header_compiles_without_a_body_user(ops):
    """The fixed bodies are templates over device-only calls (wave scans, a 64-bit atomic maximum, LDS): a source that
    instantiates none of them — every importance, scan and filter kernel — still compiles against the header."""
    assert ops.lib._gjx_jit_compile_source(b'#include "gjx_device.hpp"\nextern "C" __global__ void k() {}\n') == 0


def test_philox_lgssm_kernel_occupancy_and_inner_loop(ops, tmp_path):
    plan = ops.backsim_plan_create(_table(ops, B.lgssm_model()))
    metas = kernel_notes(plan.source(1), tmp_path, "backsim_lgssm")
    co = str(tmp_path / "backsim_lgssm.co")
    print("PHILOX LGSSM backward-simulation step kernel:", metas)
    assert "gjx_backsim_step_kernel" in metas and "gjx_backsim_last_kernel" in metas
    meta = metas["gjx_backsim_step_kernel"]
    assert meta["private_segment_fixed_size"] == 0 and meta["agpr_count"] == 0, meta
    assert meta["vgpr_count"] <= 128, meta  # four waves per SIMD of 512 registers
    loop = inner_loop_instructions(co)
    print("inner loop (lane-instructions per candidate-trajectory pair):", loop)
    if loop is not None:
        assert loop["mad_u64"] > 0 and loop["memory"] <= 8, loop  # the cipher is in the loop; candidate data is loaded once per trip


# ---- the reference is a smoother ---------------------------------------------------------------------------------------
N_REF, M_REF, R_REF, T_REF = 8192, 512, 16, 8


def test_the_reference_is_a_smoother_lgssm(oracle_ops):
    y = W.lgssm_data(T_REF)
    alg = BootstrapSMC(LinearGaussianSSM(), y, N_REF, record_history=True)
    table = _table(oracle_ops, B.lgssm_model())
    means, variances = [], []
    for r in range(R_REF):  # a run = a filter of its own and a backward pass over it: the spread holds both errors
        with use_ops(oracle_ops):
            res = alg.run(genjax.random.key(500 + r, "philox"))
        _, (paths,) = B.backsim_ref(oracle_ops, table, genjax.random.key(100 + r, "philox"), [res.history], res.log_weight_history, None,
                                    M_REF)
        p = paths.double().numpy()
        means.append(p.mean(1))
        variances.append(p.var(1))
    means, variances = np.asarray(means), np.asarray(variances)
    ms, ps = B.lgssm_rts(y)
    se = means.std(0, ddof=1) / np.sqrt(R_REF)
    z = (means.mean(0) - ms) / se
    ratio = variances.mean(0) / ps
    print("LGSSM smoothing mean z-scores:", np.round(z, 2), "variance ratios:", np.round(ratio, 3))
    assert np.all(np.abs(z) <= 4.0), z
    assert np.all(np.abs(ratio - 1.0) <= 0.10), ratio


def test_the_reference_is_a_smoother_hmm(oracle_ops):
    K = 8
    trans, emit = B.hmm_tables(K)
    rng = np.random.default_rng(7)
    pt, pe = torch.softmax(trans.double(), 1).numpy(), torch.softmax(emit.double(), 1).numpy()
    zs, ys = 0, []
    for t in range(T_REF):
        if t > 0:
            zs = rng.choice(K, p=pt[zs])
        ys.append(int(rng.choice(K, p=pe[zs])))
    alg = BootstrapSMC(DiscreteHMM(trans, emit, 0), np.asarray(ys, dtype=np.int32), N_REF, record_history=True)
    table = _table(oracle_ops, B.hmm_model(trans, emit), [("x",)])
    freqs = []
    for r in range(R_REF):
        with use_ops(oracle_ops):
            res = alg.run(genjax.random.key(600 + r, "philox"))
        _, (paths,) = B.backsim_ref(oracle_ops, table, genjax.random.key(200 + r, "philox"), [res.history], res.log_weight_history, None,
                                    M_REF)
        freqs.append(np.stack([(paths.numpy() == k).mean(1) for k in range(K)], axis=1))  # [T, K]
    freqs = np.asarray(freqs)
    exact = B.hmm_marginals(trans, emit, 0, ys)
    mean, sd = freqs.mean(0), freqs.std(0, ddof=1)
    # a state the smoother gives (next to) no mass has no spread to measure: held to an absolute 1e-3 instead
    live = sd > 0
    z = np.where(live, (mean - exact) / np.where(live, sd / np.sqrt(R_REF), 1.0), 0.0)
    print("HMM state-frequency z-scores: max |z| =", float(np.abs(z).max()))
    assert np.all(np.abs(z) <= 4.0), z
    assert np.all(np.abs(mean - exact)[~live] <= 1e-3), (mean, exact)
