"""The importance kernels' indexing by a two-dimensional grid against the oracle, bit for bit.

A launch of L passes is a grid of (rows of a pass, L) workgroups: the generated kernel takes its pass from blockIdx.y — and
with it the pass's parent key, its output offset and its slot of row sums — and its row from blockIdx.x; the Box-Muller
tables are staged for a workgroup size that is a constant of the source (gjx_device.hpp bm_stage).  The smallest shapes at
which that can go wrong: the three PHILOX forms (four, two and one particle per lane, chosen by the alignment of the output
columns), one lane / one full row / a partial second row / five rows, 1, 2, 3 and 32 passes per launch with a parent key of
its own each, a nonzero first particle and a nonzero slot of row sums, the estimate-only kernel (four rows per workgroup:
three dead rows at the end of every pass), the in-launch fold three times on the same tickets, and one scan plan for the
shared table staging."""

import ctypes as C

import pytest
import torch

from genjax._amd import abi, prng, workloads as W

pytestmark = pytest.mark.gpu

SEED = 77
POPULATIONS = [4, 256, 260, 1028]  # one lane / one full row / a partial second row / five rows (four full + one lane)
PASSES = [1, 2, 3, 32]
FORMS = {4: 0, 2: 2, 1: 1}  # particles per lane -> the columns' offset in floats (16- / 8- / 4-byte aligned)
DTYPES = [torch.float32] * W.G10_LATENTS


def same(a, b, what):
    a, b = a.cpu(), b.cpu()
    ok = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
    assert ok, f"{what}: {int((a != b).sum())} of {a.numel()} differ"


def keys_of(p, n, first=0):
    return W.importance_particle_keys(prng.key(SEED + p, 1), n, first)  # (a parent key of its own per pass)


def estimate_sites():
    sites = W.gaussian10_sites(W.gaussian10_data())
    for s in sites:
        s.out_col = -1  # no value column: the estimate-only kernel
    return sites


@pytest.fixture(scope="module")
def plans(hip_ops, oracle_ops):
    sites = W.gaussian10_sites(W.gaussian10_data())
    return hip_ops.plan_create(sites), oracle_ops.plan_create(sites)


@pytest.fixture(scope="module")
def estimate_plans(hip_ops, oracle_ops):
    return hip_ops.plan_create(estimate_sites()), oracle_ops.plan_create(estimate_sites())


_REF = {}


def reference(oracle_ops, plan, p, n, estimate=False):
    """The oracle's pass p over n particles (computed once, shared, never modified)."""
    k = (p, n, estimate)
    if k not in _REF:
        vals, score, logw, mp, rows = oracle_ops.importance_run(plan, keys_of(p, n), n, [], [] if estimate else DTYPES, want_rows=True)
        lse, e, q = oracle_ops.lse_rows(rows)
        _REF[k] = dict(values=vals, score=score, logw=logw, mp=mp, row_e=rows.e, row_s=rows.s, lse=lse, e=e, q=q)
    return _REF[k]


def columns(ops, L, stride, off):
    """A column of L passes, `stride` apart, that starts `off` floats into its (16-byte aligned) buffer."""
    return ops.empty(L * stride + 4, torch.float32)[off:off + L * stride].view(L, stride)


def launch(ops, plan, n, L, form=4, fused=False):
    stride, R = -(-n // 256) * 256, ops.num_max_partials(n)
    off = FORMS[form]
    o = dict(values=[columns(ops, L, stride, off) for _ in range(W.G10_LATENTS)], score=columns(ops, L, stride, off),
             logw=columns(ops, L, stride, off), mp=ops.empty((L, R), torch.float32), row_e=ops.empty((L, R), torch.int32),
             row_s=ops.empty((L, R), torch.int64), lse=ops.empty(L, torch.float32), e=ops.empty(L, torch.int32), q=ops.empty(L, torch.int64))
    keys = (abi.Keys * L)(*[ops._keys(keys_of(p, n), n) for p in range(L)])
    ins = (C.c_void_p * 1)()
    outs = (C.c_void_p * W.G10_LATENTS)(*[t.data_ptr() for t in o["values"]])
    tail = (ops._p(o["mp"]), ops._p(o["row_e"]), ops._p(o["row_s"]))
    score, logw = C.c_void_p(o["score"].data_ptr()), C.c_void_p(o["logw"].data_ptr())
    if fused:
        assert L == 1
        lse = abi.LseOut(o["e"].data_ptr(), o["q"].data_ptr(), o["lse"].data_ptr(), None, ops.tickets().data_ptr())
        ops.lib.call("gjx_importance_run", plan.handle, keys, ins, 0, outs, W.G10_LATENTS, score, logw, n, *tail, C.byref(lse), ops.stream())
    else:
        ops.lib.call("gjx_importance_run_batch", plan.handle, keys, L, stride, R, ins, 0, outs, W.G10_LATENTS, score, logw, n, *tail,
                     ops.stream())
    return o


def check(o, oracle_ops, oplan, n, L, what=""):
    for p in range(L):
        ref = reference(oracle_ops, oplan, p, n)
        tag = f"{what} n={n} pass {p} of {L}"
        for c in range(W.G10_LATENTS):
            same(o["values"][c][p, :n], ref["values"][c], f"column {c}, {tag}")
        same(o["score"][p, :n], ref["score"], f"score, {tag}")
        same(o["logw"][p, :n], ref["logw"], f"logw, {tag}")
        same(o["mp"][p], ref["mp"], f"row maxima, {tag}")
        same(o["row_e"][p], ref["row_e"], f"row anchors e, {tag}")
        same(o["row_s"][p], ref["row_s"], f"row sums S, {tag}")


@pytest.mark.parametrize("L", PASSES)
@pytest.mark.parametrize("n", POPULATIONS)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_pass_and_row_of_the_grid(hip_ops, oracle_ops, plans, form, n, L):
    """Every pass of the launch (pass 31 of 32 among them) draws from its own parent key and lands in its own slice."""
    hplan, oplan = plans
    check(launch(hip_ops, hplan, n, L, form), oracle_ops, oplan, n, L, what=f"{form} per lane")


def test_forms_are_chosen_by_alignment(hip_ops):
    """The launches above do run three kernels: columns offset by 8 and by 4 bytes build the pair and one-particle forms."""
    sites = W.gaussian10_sites(W.gaussian10_data())[:4]
    sites[1].arg[1] = abi.Arg(abi.ARG_CONST, 0, 0.0, 0.6789, None)  # a structure no other test compiles
    plan = hip_ops.plan_create(sites)
    n, L = 260, 2
    stride = 512
    keys = (abi.Keys * L)(*[hip_ops._keys(keys_of(p, n), n) for p in range(L)])
    ins = (C.c_void_p * 1)()
    got = {}
    for form, off in FORMS.items():
        vals = [columns(hip_ops, L, stride, off) for _ in range(2)]
        score, logw = columns(hip_ops, L, stride, off), columns(hip_ops, L, stride, off)
        outs = (C.c_void_p * 2)(*[t.data_ptr() for t in vals])
        c0 = hip_ops.jit_stats()["compiles"]
        hip_ops.lib.call("gjx_importance_run_batch", plan.handle, keys, L, stride, 2, ins, 0, outs, 2, C.c_void_p(score.data_ptr()),
                         C.c_void_p(logw.data_ptr()), n, None, None, None, hip_ops.stream())
        assert hip_ops.jit_stats()["compiles"] == c0 + 1, f"{form} particle(s) per lane: a kernel of its own"
        got[form] = logw[:, :n].clone()
    same(got[2], got[4], "pairs == quads")
    same(got[1], got[4], "one particle per lane == quads")


def test_nonzero_first_and_slot_offset(hip_ops, oracle_ops):
    """launch_passes(done, c) with done > 0: the passes' row sums go to slots done .. done + c - 1; particles 1024 ..."""
    n, first, L = 1028, 1024, 3
    wl = W.Gaussian10(hip_ops, 1, seed=SEED, n_local=n, first=first)
    prep = wl.prepare(fold_batch=2 * L, passes=L)
    prep.row_e_all.fill_(-12345)
    prep.launch_passes(L, L)
    for p in range(L):
        ref = W.Gaussian10(oracle_ops, 1, seed=SEED + p, n_local=n, first=first).step()
        same(prep.logw_all[p, :n], ref["logw"], f"logw pass {p}")
        same(prep.score_all[p, :n], ref["score"], f"score pass {p}")
        for c, col in enumerate(ref["values"]):
            same(prep.values_all[c][p, :n], col, f"column {c} pass {p}")
        same(prep.row_e_all[L + p], ref["rows"].e, f"row anchors, slot {L + p}")
        same(prep.row_s_all[L + p], ref["rows"].s, f"row sums, slot {L + p}")
    assert bool((prep.row_e_all[:L] == -12345).all()), "the slots in front of `done` are not written"


def test_estimate_only_dead_rows_stay_inert(hip_ops, oracle_ops, estimate_plans):
    """No value column: four one-wave rows per workgroup.  n = 1028 is five rows per pass, so the second workgroup of every
    pass has three dead rows — they must write nothing, neither into the next pass's slot nor behind the last one."""
    hplan, oplan = estimate_plans
    n, L = 1028, 3
    R = hip_ops.num_max_partials(n)
    assert R == 5
    guard = 8
    row_e = torch.full((L * R + guard,), -12345, dtype=torch.int32, device=hip_ops.device())
    row_s = torch.full((L * R + guard,), -12345, dtype=torch.int64, device=hip_ops.device())
    keys = (abi.Keys * L)(*[hip_ops._keys(keys_of(p, n), n) for p in range(L)])
    ins, outs = (C.c_void_p * 1)(), (C.c_void_p * 1)()
    hip_ops.lib.call("gjx_importance_run_batch", hplan.handle, keys, L, 1280, R, ins, 0, outs, 0, None, None, n, None,
                     C.c_void_p(row_e.data_ptr()), C.c_void_p(row_s.data_ptr()), hip_ops.stream())
    for p in range(L):
        ref = reference(oracle_ops, oplan, p, n, estimate=True)
        same(row_e[p * R:(p + 1) * R], ref["row_e"], f"row anchors, pass {p}")
        same(row_s[p * R:(p + 1) * R], ref["row_s"], f"row sums, pass {p}")
    assert bool((row_e[L * R:] == -12345).all()) and bool((row_s[L * R:] == -12345).all()), "a dead row wrote behind the last pass"


def test_fused_tail_three_times_on_the_same_tickets(hip_ops, oracle_ops, plans):
    """The in-launch fold counts one ticket per workgroup of the grid and leaves the tickets zero for the next launch."""
    hplan, oplan = plans
    n = 1028
    ref = reference(oracle_ops, oplan, 0, n)
    first = None
    for k in range(3):
        o = launch(hip_ops, hplan, n, 1, fused=True)
        check(o, oracle_ops, oplan, n, 1, what=f"fused tail, launch {k}")
        got = (o["lse"].cpu().clone(), o["e"].cpu().clone(), o["q"].cpu().clone())
        if first is None:
            first = got
            for a, name in zip(got, ("lse", "e", "q")):
                same(a, ref[name], f"folded {name} == the oracle's")
        for a, b, name in zip(got, first, ("lse", "e", "q")):
            same(a, b, f"folded {name}, launch {k} == launch 0")
        assert bool((hip_ops.tickets() == 0).all()), f"tickets after launch {k}"
    # the fold itself: the same rows folded by the separate launch
    o2 = launch(hip_ops, hplan, n, 1)
    hip_ops.lib.call("gjx_lse_rows_batch", hip_ops._p(o2["row_e"]), hip_ops._p(o2["row_s"]), o2["row_e"].shape[1], 1, o2["row_e"].shape[1],
                     hip_ops._p(o2["e"]), hip_ops._p(o2["q"]), hip_ops._p(o2["lse"]), None, hip_ops.stream())
    for a, b, name in zip(first, (o2["lse"], o2["e"], o2["q"]), ("lse", "e", "q")):
        same(a, b, f"in-launch fold == separate fold, {name}")


def test_scan_plan_shares_the_table_staging(hip_ops, oracle_ops):
    """LGSSM as a scan, n = 260 (a partial second row), T = 3: the quad scan kernel stages the tables the same way."""
    n, T = 260, 3
    got, ref = W.lgssm_scan(hip_ops, 1, SEED, n, T), W.lgssm_scan(oracle_ops, 1, SEED, n, T)
    for k in ("x", "logw", "score", "carry", "max_partials", "row_e", "row_s"):
        same(got[k], ref[k], f"scan {k}")
